// The facade's bridgeContours (G2 and G4 give the same) against known answers: a horizontal dashed line in row 16, seven dashes of six
// pixels from x = 2 with gaps of three.  Every gap gets one bridge of five points -- the two end pixels and the three missing ones --, the
// bridged ends read as junctions, and stitchContours over the partners bridgeContours names gives the whole line, 60 pixels in order.
// Built and run by tests/test_gpu_bridges.py.  Prints "bridges OK ..." and exits 0.
#include <cvsteer/SteerableFiltersG2.h>
#include <cvsteer/SteerableFiltersG4.h>

#include <cstdio>
#include <stdexcept>
#include <vector>

int main()
{
    const int dashes = 7, dash = 6, gap = 3, row = 16, x0 = 2;
    std::vector<std::vector<fa::Point> > chains((size_t)dashes);
    for (int d = 0; d < dashes; ++d)
        for (int k = 0; k < dash; ++k) chains[(size_t)d].push_back(fa::Point(x0 + d * (dash + gap) + k, row));
    const std::vector<int> flags((size_t)dashes, 0);

    fa::Mat1f image(16, 16);
    for (int r = 0; r < 16; ++r)
        for (int c = 0; c < 16; ++c) image(r, c) = 0.0f;
    fa::SteerableFiltersG2 f2(image);
    fa::SteerableFiltersG4 f4(image);
    std::vector<std::vector<fa::Point> > bridged, bridged4, bridged0;
    std::vector<int> bflags, bflags4, bflags0, partners, partners4;
    const int n = f2.bridgeContours(chains, &flags, 8, 4, 0.8f, bridged, bflags, &partners);
    if (n != dashes - 1 || f4.bridgeContours(chains, 0, 8, 4, 0.8f, bridged4, bflags4, &partners4) != n) return 3;
    if (f2.bridgeContours(chains, &flags, 8, 4, 0.8f, bridged0, bflags0) != n) return 3;   // without the optional output
    if (bridged.size() != (size_t)(2 * dashes - 1) || bflags.size() != bridged.size() || partners.size() != 2 * bridged.size()) return 3;
    if (bflags4 != bflags || partners4 != partners || bflags0 != bflags || bridged4.size() != bridged.size() || bridged0.size() != bridged.size()) return 3;
    for (size_t c = 0; c < bridged.size(); ++c) {
        if (bridged[c].size() != bridged4[c].size() || bridged[c].size() != bridged0[c].size()) return 4;
        for (size_t k = 0; k < bridged[c].size(); ++k)
            if (bridged[c][k].x != bridged4[c][k].x || bridged[c][k].y != bridged4[c][k].y || bridged[c][k].x != bridged0[c][k].x ||
                bridged[c][k].y != bridged0[c][k].y)
                return 4;
    }
    // the known answers
    for (int d = 0; d < dashes; ++d) {
        if (bridged[(size_t)d].size() != (size_t)dash) return 5;
        for (int k = 0; k < dash; ++k)
            if (bridged[(size_t)d][(size_t)k].x != chains[(size_t)d][(size_t)k].x || bridged[(size_t)d][(size_t)k].y != row) return 5;
        const int want = (d > 0 ? 2 : 0) | (d < dashes - 1 ? 4 : 0);   // CVS_CHAIN_HEAD_JUNCTION, CVS_CHAIN_TAIL_JUNCTION
        if (bflags[(size_t)d] != want) return 5;
    }
    for (int b = 0; b < dashes - 1; ++b) {
        const std::vector<fa::Point>& line = bridged[(size_t)(dashes + b)];
        if (line.size() != (size_t)(gap + 2) || bflags[(size_t)(dashes + b)] != 6) return 6;
        for (int k = 0; k < gap + 2; ++k)
            if (line[(size_t)k].x != x0 + b * (dash + gap) + dash - 1 + k || line[(size_t)k].y != row) return 6;
        // the tail of dash b continues into the bridge's head, the bridge's tail into the head of dash b + 1
        if (partners[(size_t)(2 * b + 1)] != 2 * (dashes + b) || partners[(size_t)(2 * (dashes + b))] != 2 * b + 1) return 7;
        if (partners[(size_t)(2 * (b + 1))] != 2 * (dashes + b) + 1 || partners[(size_t)(2 * (dashes + b) + 1)] != 2 * (b + 1)) return 7;
    }
    if (partners[0] != -1 || partners[(size_t)(2 * dashes - 1)] != -1) return 7;
    std::vector<std::vector<fa::Point> > paths;
    std::vector<int> pathFlags;
    if (f2.stitchContours(bridged, &bflags, partners, paths, &pathFlags) != 1 || paths.size() != 1 || pathFlags[0] != 0) return 8;
    const size_t whole = (size_t)(dashes * (dash + gap) - gap);
    if (paths[0].size() != whole) return 8;
    for (size_t k = 0; k < whole; ++k)
        if (paths[0][k].x != x0 + (int)k || paths[0][k].y != row) return 8;
    // a gap too wide for maxGap: no bridge, the chains as they are
    if (f2.bridgeContours(chains, &flags, 8, 3, 0.8f, bridged0, bflags0, &partners4) != 0 || bridged0.size() != (size_t)dashes) return 9;
    for (size_t e = 0; e < partners4.size(); ++e)
        if (partners4[e] != -1) return 9;
    // flags of another length and a maxGap outside 2 .. 32 are refused
    int thrown = 0;
    std::vector<int> few(flags.begin(), flags.end());
    few.push_back(0);
    try {
        f2.bridgeContours(chains, &few, 8, 4, 0.8f, bridged0, bflags0);
    } catch (const std::runtime_error&) {
        ++thrown;
    }
    try {
        f2.bridgeContours(chains, &flags, 8, 1, 0.8f, bridged0, bflags0);
    } catch (const std::runtime_error&) {
        ++thrown;
    }
    try {
        f4.bridgeContours(chains, &flags, 8, 33, 0.8f, bridged0, bflags0);
    } catch (const std::runtime_error&) {
        ++thrown;
    }
    if (thrown != 3) return 10;
    std::printf("bridges OK (%d dashes, %d bridges, %d path of %d points)\n", dashes, n, (int)paths.size(), (int)paths[0].size());
    return 0;
}
