// The facade's joinContours (G2; and that a G4 object without orientation state throws) on an image and chains read from files, written
// back for the caller to compare.  Built and run by tests/test_gpu_joins.py: `test_joins image rows cols chains radius min_cos out`.
// image: raw f32, rows x cols, setup image and response in one.  chains: int32 n_chains, then per chain int32 length, int32 flags and
// length (x, y) pairs.  out: per chain end f32 partner, cos (NaN where the partner is -1), in end order.  Prints "joins OK" and exits 0.
#include <cvsteer/SteerableFiltersG2.h>
#include <cvsteer/SteerableFiltersG4.h>

#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <stdint.h>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 8) return 2;
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), radius = std::atoi(argv[5]);
    const float min_cos = (float)std::atof(argv[6]);
    fa::Mat1f image(rows, cols);
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) return 2;
    for (int r = 0; r < rows; ++r)
        if (std::fread(image.ptr(r), sizeof(float), cols, fp) != (size_t)cols) return 2;
    std::fclose(fp);
    fp = std::fopen(argv[4], "rb");
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

    fa::SteerableFiltersG2 f2(image);
    std::vector<int> partners, partners0;
    std::vector<float> cosines;
    const int n = f2.joinContours(image, chains, &flags, radius, min_cos, partners, &cosines);
    if (f2.joinContours(image, chains, &flags, radius, min_cos, partners0) != n) return 3;   // no cosines
    if (partners.size() != 2 * (size_t)nc || cosines.size() != 2 * (size_t)nc || partners0 != partners) return 3;
    int pairs = 0;
    for (size_t e = 0; e < partners.size(); ++e) {
        const int p = partners[e];
        if (p < 0) {
            if (cosines[e] == cosines[e]) return 4;                                          // NaN without a mutual join
            continue;
        }
        if ((size_t)p >= partners.size() || (size_t)p == e || partners[(size_t)p] != (int)e) return 4;   // an involution
        if (!(cosines[e] >= min_cos) || cosines[e] != cosines[(size_t)p]) return 4;
        if ((size_t)p > e) ++pairs;
    }
    if (pairs != n) return 3;

    // flags of another length and a radius out of range are refused, and a G4 object (no orientation state) has no theta to refine on
    int thrown = 0;
    std::vector<int> few(flags.begin(), flags.end());
    few.push_back(0);
    try {
        f2.joinContours(image, chains, &few, radius, min_cos, partners0);
    } catch (const std::runtime_error&) {
        ++thrown;
    }
    try {
        f2.joinContours(image, chains, &flags, 65, min_cos, partners0);
    } catch (const std::runtime_error&) {
        ++thrown;
    }
    fa::SteerableFiltersG4 f4(image);
    try {
        f4.joinContours(image, chains, &flags, radius, min_cos, partners0);
    } catch (const std::runtime_error&) {
        ++thrown;
    }
    if (thrown != 3) return 6;

    fp = std::fopen(argv[7], "wb");
    if (!fp) return 7;
    for (size_t e = 0; e < partners.size(); ++e) {
        const float rec[2] = {(float)partners[e], cosines[e]};
        if (std::fwrite(rec, sizeof(float), 2, fp) != 2) return 7;
    }
    std::fclose(fp);
    std::printf("joins OK (%d chains, %d mutual joins)\n", (int)nc, n);
    return 0;
}
