// The facade's fitSegments (G2; and that a G4 object without orientation state throws) on an image and chains read from files, written back
// for the caller to compare.  Built and run by tests/test_gpu_segments.py: `test_segments image rows cols chains eps out`.  image: raw f32,
// rows x cols, setup image and response in one.  chains: int32 n_chains, then per chain int32 length, int32 flags and length (x, y) pairs.
// out: per segment f32 chain, x0, y0, x1, y1, rms, in chain and span order.  Prints "segments OK" and exits 0.
#include <cvsteer/SteerableFiltersG2.h>
#include <cvsteer/SteerableFiltersG4.h>

#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <stdint.h>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 7) return 2;
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
    const float eps = (float)std::atof(argv[5]);
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
    std::vector<std::vector<float> > lines, rms, lines0;
    const int n = f2.fitSegments(image, chains, &flags, eps, lines, &rms);
    if (f2.fitSegments(image, chains, &flags, eps, lines0) != n) return 3;   // no rms
    if (lines.size() != (size_t)nc || rms.size() != (size_t)nc || lines0.size() != (size_t)nc) return 3;
    int total = 0;
    for (int c = 0; c < nc; ++c) {
        if (lines[(size_t)c].size() != 4 * rms[(size_t)c].size() || lines0[(size_t)c] != lines[(size_t)c]) return 3;
        total += (int)rms[(size_t)c].size();
    }
    if (total != n) return 3;

    // flags of another length are refused, and a G4 object (no orientation state) has no theta to refine on: both throw
    int thrown = 0;
    std::vector<int> few(flags.begin(), flags.end());
    few.push_back(0);
    try {
        f2.fitSegments(image, chains, &few, eps, lines0);
    } catch (const std::runtime_error&) {
        ++thrown;
    }
    fa::SteerableFiltersG4 f4(image);
    try {
        f4.fitSegments(image, chains, &flags, eps, lines0);
    } catch (const std::runtime_error&) {
        ++thrown;
    }
    if (thrown != 2) return 6;

    fp = std::fopen(argv[6], "wb");
    if (!fp) return 7;
    for (int c = 0; c < nc; ++c)
        for (size_t k = 0; k < rms[(size_t)c].size(); ++k) {
            const float* p = &lines[(size_t)c][4 * k];
            const float rec[6] = {(float)c, p[0], p[1], p[2], p[3], rms[(size_t)c][k]};
            if (std::fwrite(rec, sizeof(float), 6, fp) != 6) return 7;
        }
    std::fclose(fp);
    std::printf("segments OK (%d chains, %d segments)\n", (int)nc, n);
    return 0;
}
