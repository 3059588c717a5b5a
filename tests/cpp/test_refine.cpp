// The facade's refineContours against the C ABI's cvs_chain_refine on the same object, bit for bit, on an image and chains read from files.
// Built and run by tests/test_gpu_refine.py: `test_refine image rows cols chains out`.  image: raw f32, rows x cols, setup image and response
// in one.  chains: int32 n_chains, then per chain int32 length and length (x, y) pairs.  out: per point f32 xs, ys, strength, in chain
// order.  Prints "refine OK" and exits 0.
#include <cvsteer/SteerableFiltersG2.h>
#include <cvsteer/SteerableFiltersG4.h>

#include "cvsteer_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <stdint.h>
#include <vector>

static bool same(float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; }

int main(int argc, char** argv)
{
    if (argc != 6) return 2;
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
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
    std::vector<int32_t> flat;
    for (int c = 0; c < nc; ++c) {
        int32_t len = 0;
        if (std::fread(&len, sizeof(int32_t), 1, fp) != 1 || len < 1) return 2;
        std::vector<int32_t> xy((size_t)len * 2);
        if (std::fread(xy.data(), sizeof(int32_t), xy.size(), fp) != xy.size()) return 2;
        for (int k = 0; k < len; ++k) chains[(size_t)c].push_back(fa::Point(xy[2 * (size_t)k], xy[2 * (size_t)k + 1]));
        flat.insert(flat.end(), xy.begin(), xy.end());
    }
    std::fclose(fp);
    const int np = (int)(flat.size() / 2);

    fa::SteerableFiltersG2 f2(image);
    std::vector<std::vector<float> > xs, ys, st, xs0, ys0;
    if (f2.refineContours(image, chains, xs, ys, &st) != np) return 3;
    if (f2.refineContours(image, chains, xs0, ys0) != np) return 3;   // no strength
    if (xs.size() != (size_t)nc || ys.size() != (size_t)nc || st.size() != (size_t)nc || xs0.size() != (size_t)nc) return 3;

    // the same through the C ABI, on the object's own handle and its own theta
    std::vector<float> dense((size_t)rows * cols), xy((size_t)np * 2), str((size_t)np);
    for (int r = 0; r < rows; ++r) std::memcpy(&dense[(size_t)r * cols], image.ptr(r), (size_t)cols * sizeof(float));
    cvs_plane pm = {dense.data(), rows, cols, (size_t)cols * sizeof(float), CVS_MEM_HOST};
    if (cvs_chain_refine(f2.handle(), &pm, 0, flat.data(), np, xy.data(), str.data(), CVS_MEM_HOST) != CVS_OK) return 4;
    long bad = 0, moved = 0;
    size_t at = 0;
    for (int c = 0; c < nc; ++c) {
        const size_t len = chains[(size_t)c].size();
        if (xs[(size_t)c].size() != len || ys[(size_t)c].size() != len || st[(size_t)c].size() != len || xs0[(size_t)c].size() != len) return 3;
        for (size_t k = 0; k < len; ++k, ++at) {
            bad += !same(xs[(size_t)c][k], xy[2 * at]) || !same(ys[(size_t)c][k], xy[2 * at + 1]) || !same(st[(size_t)c][k], str[at]);
            bad += !same(xs0[(size_t)c][k], xy[2 * at]) || !same(ys0[(size_t)c][k], xy[2 * at + 1]);
            moved += xs[(size_t)c][k] != (float)chains[(size_t)c][k].x || ys[(size_t)c][k] != (float)chains[(size_t)c][k].y;
        }
    }
    if (bad != 0 || (np > 100 && moved == 0)) {
        std::printf("refine MISMATCH: %ld of %d points differ, %ld moved\n", bad, np, moved);
        return 5;
    }

    // a point outside the image is refused, and a G4 object (no orientation state) has no theta of its own: both throw
    int thrown = 0;
    std::vector<std::vector<fa::Point> > outside(1, std::vector<fa::Point>(1, fa::Point(cols, 0)));
    try {
        f2.refineContours(image, outside, xs0, ys0);
    } catch (const std::runtime_error&) {
        ++thrown;
    }
    fa::SteerableFiltersG4 f4(image);
    try {
        f4.refineContours(image, chains, xs0, ys0);
    } catch (const std::runtime_error&) {
        ++thrown;
    }
    if (thrown != 2) return 6;

    fp = std::fopen(argv[5], "wb");
    if (!fp) return 7;
    for (int c = 0; c < nc; ++c)
        for (size_t k = 0; k < chains[(size_t)c].size(); ++k) {
            const float rec[3] = {xs[(size_t)c][k], ys[(size_t)c][k], st[(size_t)c][k]};
            if (std::fwrite(rec, sizeof(float), 3, fp) != 3) return 7;
        }
    std::fclose(fp);
    std::printf("refine OK (%d chains, %d points)\n", (int)nc, np);
    return 0;
}
