// The facade's stitchContours (G2 and G4 give the same) on chains and partners read from files, written back for the caller to compare.
// Built and run by tests/test_gpu_paths.py: `test_paths chains partners out`.
// chains: int32 n_chains, then per chain int32 length, int32 flags and length (x, y) pairs.  partners: 2 * n_chains int32, as joinContours
// returns them.  out: int32 n_paths, then per path int32 flags, int32 n_members, the members (2 * chain + reversed), int32 n_points and the
// (x, y) pairs.  Prints "paths OK" and exits 0.
#include <cvsteer/SteerableFiltersG2.h>
#include <cvsteer/SteerableFiltersG4.h>

#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <stdint.h>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    FILE* fp = std::fopen(argv[1], "rb");
    int32_t nc = 0;
    if (!fp || std::fread(&nc, sizeof(int32_t), 1, fp) != 1 || nc < 0) return 2;
    std::vector<std::vector<fa::Point> > chains((size_t)nc);
    std::vector<int> flags((size_t)nc);
    for (int c = 0; c < nc; ++c) {
        int32_t head[2] = {0, 0};
        if (std::fread(head, sizeof(int32_t), 2, fp) != 2 || head[0] < 1) return 2;
        std::vector<int32_t> xy((size_t)head[0] * 2);
        if (std::fread(xy.data(), sizeof(int32_t), xy.size(), fp) != xy.size()) return 2;
        for (int k = 0; k < head[0]; ++k) chains[(size_t)c].push_back(fa::Point(xy[2 * (size_t)k], xy[2 * (size_t)k + 1]));
        flags[(size_t)c] = head[1];
    }
    std::fclose(fp);
    std::vector<int32_t> words(2 * (size_t)nc);
    fp = std::fopen(argv[2], "rb");
    if (!fp || std::fread(words.data(), sizeof(int32_t), words.size(), fp) != words.size()) return 2;
    std::fclose(fp);
    const std::vector<int> partners(words.begin(), words.end());

    fa::Mat1f image(16, 16);
    for (int r = 0; r < 16; ++r)
        for (int c = 0; c < 16; ++c) image(r, c) = 0.0f;
    fa::SteerableFiltersG2 f2(image);
    fa::SteerableFiltersG4 f4(image);
    std::vector<std::vector<fa::Point> > paths, paths0, paths4;
    std::vector<int> pathFlags, pathFlags4;
    std::vector<std::vector<int> > members, members4;
    const int n = f2.stitchContours(chains, &flags, partners, paths, &pathFlags, &members);
    if (f2.stitchContours(chains, &flags, partners, paths0) != n) return 3;                  // without the optional outputs
    if (f4.stitchContours(chains, &flags, partners, paths4, &pathFlags4, &members4) != n) return 3;
    if (paths.size() != (size_t)n || pathFlags.size() != (size_t)n || members.size() != (size_t)n || paths0.size() != (size_t)n) return 3;
    if (pathFlags4 != pathFlags || members4 != members || paths4.size() != (size_t)n) return 3;
    size_t total = 0;
    for (size_t p = 0; p < paths.size(); ++p) {
        if (paths[p].size() != paths0[p].size() || paths[p].size() != paths4[p].size() || members[p].empty()) return 4;
        for (size_t k = 0; k < paths[p].size(); ++k)
            if (paths[p][k].x != paths0[p][k].x || paths[p][k].y != paths0[p][k].y || paths[p][k].x != paths4[p][k].x ||
                paths[p][k].y != paths4[p][k].y)
                return 4;
        total += members[p].size();
    }
    if (total != (size_t)nc) return 4;                                                       // every chain is in exactly one path

    // flags or partners of another length are refused
    int thrown = 0;
    std::vector<int> few(flags.begin(), flags.end());
    few.push_back(0);
    try {
        f2.stitchContours(chains, &few, partners, paths0);
    } catch (const std::runtime_error&) {
        ++thrown;
    }
    std::vector<int> odd(partners.begin(), partners.end());
    odd.push_back(-1);
    try {
        f2.stitchContours(chains, &flags, odd, paths0);
    } catch (const std::runtime_error&) {
        ++thrown;
    }
    if (thrown != 2) return 6;

    fp = std::fopen(argv[3], "wb");
    if (!fp) return 7;
    std::vector<int32_t> out;
    out.push_back(n);
    for (size_t p = 0; p < paths.size(); ++p) {
        out.push_back(pathFlags[p]);
        out.push_back((int32_t)members[p].size());
        for (size_t k = 0; k < members[p].size(); ++k) out.push_back(members[p][k]);
        out.push_back((int32_t)paths[p].size());
        for (size_t k = 0; k < paths[p].size(); ++k) {
            out.push_back(paths[p][k].x);
            out.push_back(paths[p][k].y);
        }
    }
    if (std::fwrite(out.data(), sizeof(int32_t), out.size(), fp) != out.size()) return 7;
    std::fclose(fp);
    std::printf("paths OK (%d chains, %d paths)\n", (int)nc, n);
    return 0;
}
