// The facade's approxContours (both classes) on chains read from a file, written back for the caller to compare.
// Built and run by tests/test_gpu_polylines.py: `test_polylines in out eps`.  in: int32 n_chains, then per chain int32 length, flags and
// length (x, y) pairs.  out: int32 n_vertices, then per chain int32 length and its (x, y) pairs.  Prints "polylines OK" and exits 0.
#include <cvsteer/SteerableFiltersG2.h>
#include <cvsteer/SteerableFiltersG4.h>

#include <cstdio>
#include <cstdlib>
#include <stdint.h>
#include <vector>

static bool get(FILE* fp, int32_t* v, size_t n) { return std::fread(v, sizeof(int32_t), n, fp) == n; }
static bool put(FILE* fp, const int32_t* v, size_t n) { return std::fwrite(v, sizeof(int32_t), n, fp) == n; }

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const float eps = (float)std::atof(argv[3]);
    FILE* fp = std::fopen(argv[1], "rb");
    int32_t nc = 0;
    if (!fp || !get(fp, &nc, 1) || nc < 0) return 2;
    std::vector<std::vector<fa::Point> > chains((size_t)nc);
    std::vector<int> flags((size_t)nc);
    bool any_flag = false;
    for (int c = 0; c < nc; ++c) {
        int32_t hd[2];
        if (!get(fp, hd, 2) || hd[0] < 1) return 2;
        flags[(size_t)c] = hd[1];
        any_flag = any_flag || hd[1] != 0;
        std::vector<int32_t> xy((size_t)hd[0] * 2);
        if (!get(fp, xy.data(), xy.size())) return 2;
        for (int k = 0; k < hd[0]; ++k) chains[(size_t)c].push_back(fa::Point(xy[2 * (size_t)k], xy[2 * (size_t)k + 1]));
    }
    std::fclose(fp);

    fa::Mat1f image(16, 16);
    for (int r = 0; r < 16; ++r)
        for (int c = 0; c < 16; ++c) image(r, c) = (float)((r * 5 + c * 3) % 7);
    fa::SteerableFiltersG2 f2(image);
    fa::SteerableFiltersG4 f4(image);
    std::vector<std::vector<fa::Point> > p2, p4, open2;
    const int n2 = f2.approxContours(chains, &flags, eps, p2);
    const int n4 = f4.approxContours(chains, &flags, eps, p4);
    const int n0 = f2.approxContours(chains, 0, eps, open2);   // no flags: every chain open
    if (n2 != n4 || p2.size() != (size_t)nc || p4.size() != (size_t)nc || open2.size() != (size_t)nc) return 3;
    long total = 0, total0 = 0;
    for (int c = 0; c < nc; ++c) {
        if (p2[(size_t)c].size() != p4[(size_t)c].size()) return 3;
        for (size_t k = 0; k < p2[(size_t)c].size(); ++k)
            if (p2[(size_t)c][k].x != p4[(size_t)c][k].x || p2[(size_t)c][k].y != p4[(size_t)c][k].y) return 3;
        total += (long)p2[(size_t)c].size();
        total0 += (long)open2[(size_t)c].size();
    }
    if (total != n2 || total0 != n0 || (!any_flag && n0 != n2)) return 3;

    fp = std::fopen(argv[2], "wb");
    const int32_t nv = n2;
    if (!fp || !put(fp, &nv, 1)) return 4;
    for (int c = 0; c < nc; ++c) {
        const int32_t len = (int32_t)p2[(size_t)c].size();
        if (!put(fp, &len, 1)) return 4;
        for (int32_t k = 0; k < len; ++k) {
            const int32_t xy[2] = {p2[(size_t)c][(size_t)k].x, p2[(size_t)c][(size_t)k].y};
            if (!put(fp, xy, 2)) return 4;
        }
    }
    std::fclose(fp);
    std::printf("polylines OK (%d chains, %d vertices)\n", (int)nc, n2);
    return 0;
}
