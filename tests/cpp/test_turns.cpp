// The facade's cornerContours (G2; and that a G4 object without orientation state throws) on an image and chains read from files, written
// back for the caller to compare.  Built and run by tests/test_gpu_turns.py: `test_turns image rows cols chains radius max_cos out`.
// image: raw f32, rows x cols, setup image and response in one.  chains: int32 n_chains, then per chain int32 length, int32 flags and
// length (x, y) pairs.  out: per corner f32 chain, offset into the chain, cos, in chain and offset order.  Prints "turns OK" and exits 0.
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
    const float max_cos = (float)std::atof(argv[6]);
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
    std::vector<std::vector<int> > corners, corners0;
    std::vector<std::vector<float> > cosines;
    const int n = f2.cornerContours(image, chains, &flags, radius, max_cos, corners, &cosines);
    if (f2.cornerContours(image, chains, &flags, radius, max_cos, corners0) != n) return 3;   // no cosines
    if (corners.size() != (size_t)nc || cosines.size() != (size_t)nc || corners0 != corners) return 3;
    int total = 0;
    for (int c = 0; c < nc; ++c) {
        if (corners[(size_t)c].size() != cosines[(size_t)c].size()) return 3;
        for (size_t k = 0; k < corners[(size_t)c].size(); ++k) {
            const int at = corners[(size_t)c][k];
            if (at < 0 || at >= (int)chains[(size_t)c].size() || (k > 0 && at <= corners[(size_t)c][k - 1])) return 4;   // offsets, ascending
            if (!(cosines[(size_t)c][k] <= max_cos)) return 4;
        }
        total += (int)corners[(size_t)c].size();
    }
    if (total != n) return 3;

    // flags of another length and a radius out of range are refused, and a G4 object (no orientation state) has no theta to refine on
    int thrown = 0;
    std::vector<int> few(flags.begin(), flags.end());
    few.push_back(0);
    try {
        f2.cornerContours(image, chains, &few, radius, max_cos, corners0);
    } catch (const std::runtime_error&) {
        ++thrown;
    }
    try {
        f2.cornerContours(image, chains, &flags, 65, max_cos, corners0);
    } catch (const std::runtime_error&) {
        ++thrown;
    }
    fa::SteerableFiltersG4 f4(image);
    try {
        f4.cornerContours(image, chains, &flags, radius, max_cos, corners0);
    } catch (const std::runtime_error&) {
        ++thrown;
    }
    if (thrown != 3) return 6;

    fp = std::fopen(argv[7], "wb");
    if (!fp) return 7;
    for (int c = 0; c < nc; ++c)
        for (size_t k = 0; k < corners[(size_t)c].size(); ++k) {
            const float rec[3] = {(float)c, (float)corners[(size_t)c][k], cosines[(size_t)c][k]};
            if (std::fwrite(rec, sizeof(float), 3, fp) != 3) return 7;
        }
    std::fclose(fp);
    std::printf("turns OK (%d chains, %d corners)\n", (int)nc, n);
    return 0;
}
