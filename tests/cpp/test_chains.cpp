// The facade's traceContours (both classes) against the C ABI's arrays on a handle of its own, point for point.
// Built and run by tests/test_gpu_chains.py with a 0 / 255 mask as raw f32 (path rows cols); prints "chains OK" and exits 0.
#include <cvsteer/SteerableFiltersG2.h>
#include <cvsteer/SteerableFiltersG4.h>

#include "cvsteer_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
    fa::Mat1f mask(rows, cols);
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) return 2;
    for (int r = 0; r < rows; ++r)
        if (std::fread(mask.ptr(r), sizeof(float), cols, fp) != (size_t)cols) return 2;
    std::fclose(fp);

    fa::SteerableFiltersG2 f2(mask);
    fa::SteerableFiltersG4 f4(mask);
    std::vector<std::vector<fa::Point> > c2, c4;
    std::vector<int> fl2, fl4;
    const int n2 = f2.traceContours(mask, c2, &fl2);
    const int n4 = f4.traceContours(mask, c4, &fl4);
    std::vector<std::vector<fa::Point> > plain;
    if (f2.traceContours(mask, plain) != n2 || plain.size() != c2.size()) return 5;

    // the same through the C ABI: a dense copy on a handle of its own
    cvs_handle hd = 0;
    if (cvs_create(CVS_KIND_G2, 4, 0.67f, 0, &hd) != CVS_OK) return 3;
    std::vector<float> dense((size_t)rows * cols);
    for (int r = 0; r < rows; ++r) std::memcpy(&dense[(size_t)r * cols], mask.ptr(r), (size_t)cols * sizeof(float));
    cvs_plane pm = {dense.data(), rows, cols, (size_t)cols * sizeof(float), CVS_MEM_HOST};
    if (cvs_setup(hd, &pm, CVS_SETUP_BASIS) != CVS_OK) return 3;
    int np = -1, nc = -1;
    if (cvs_contour_chains(hd, &pm, 0, 0, 0, 0, CVS_MEM_HOST, &np, &nc) != CVS_E_SIZE || np <= 0 || nc <= 0) return 4;
    std::vector<int32_t> pts((size_t)np * 2);
    std::vector<cvs_chain> tab((size_t)nc);
    if (cvs_contour_chains(hd, &pm, pts.data(), np, tab.data(), nc, CVS_MEM_HOST, &np, &nc) != CVS_OK) return 4;
    cvs_destroy(hd);

    long bad = 0, total = 0;
    if (n2 != nc || n4 != nc || (int)c2.size() != nc || (int)c4.size() != nc || (int)fl2.size() != nc || (int)fl4.size() != nc) bad = -1;
    for (int c = 0; c < nc && bad == 0; ++c) {
        const cvs_chain& t = tab[(size_t)c];
        if ((int)c2[(size_t)c].size() != t.length || (int)c4[(size_t)c].size() != t.length || plain[(size_t)c].size() != c2[(size_t)c].size() ||
            fl2[(size_t)c] != t.flags || fl4[(size_t)c] != t.flags || t.start != total || t.reserved != 0) {
            ++bad;
            break;
        }
        for (int k = 0; k < t.length; ++k) {
            const int x = pts[2 * (size_t)(t.start + k)], y = pts[2 * (size_t)(t.start + k) + 1];
            const fa::Point a = c2[(size_t)c][(size_t)k], b = c4[(size_t)c][(size_t)k], p = plain[(size_t)c][(size_t)k];
            bad += a.x != x || a.y != y || b.x != x || b.y != y || p.x != x || p.y != y;
            bad += !(mask(y, x) > 0.0f);
        }
        total += t.length;
    }
    if (bad || total != np) {
        std::printf("chains: %ld mismatches; chains %d / %d / %d, points %ld / %d\n", bad, n2, n4, nc, total, np);
        return 1;
    }
    std::printf("chains OK (%d chains, %d points)\n", nc, np);
    return 0;
}
