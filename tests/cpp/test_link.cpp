// The facade's linkContours against hysteresis + pruneContours of the same object, and against cvs_link through the C ABI on a handle of
// its own, bit for bit.  Built and run by tests/test_gpu_link.py with the fish image as raw f32 (path rows cols); prints "link OK" and
// exits 0.
#include <cvsteer/SteerableFiltersG2.h>
#include <cvsteer/SteerableFiltersG4.h>

#include "cvsteer_hip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static long rows_differ(const fa::Mat1f& a, const fa::Mat1f& b)
{
    if (a.rows != b.rows || a.cols != b.cols) return -1;
    long bad = 0;
    for (int r = 0; r < a.rows; ++r) bad += std::memcmp(a.ptr(r), b.ptr(r), (size_t)a.cols * sizeof(float)) != 0;
    return bad;
}

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
    fa::Mat1f img(rows, cols);
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) return 2;
    for (int r = 0; r < rows; ++r)
        if (std::fread(img.ptr(r), sizeof(float), cols, fp) != (size_t)cols) return 2;
    std::fclose(fp);

    fa::SteerableFiltersG2 f(img);
    fa::Mat1f g, h, e, m, p, edges, dark, bright;
    f.pipeline(img, g, h, e, m, p, edges, dark, bright);
    fa::Mat1f thin, linked, pruned, both, plain, both4;
    f.nonMaxSuppression(edges, thin);
    f.hysteresis(thin, 10.0f, 40.0f, linked);
    f.pruneContours(linked, thin, 8, 60.0f, pruned);
    f.linkContours(thin, 10.0f, 40.0f, 8, 60.0f, both);
    f.linkContours(thin, 10.0f, 40.0f, 0, -INFINITY, plain);   // no prune: hysteresis itself
    fa::SteerableFiltersG4 f4(img);                            // the G4 class carries the same member; it reads the plane passed
    f4.linkContours(thin, 10.0f, 40.0f, 8, 60.0f, both4);

    // the same through the C ABI: a dense copy on a handle of its own
    cvs_handle hd = 0;
    if (cvs_create(CVS_KIND_G2, 4, 0.67f, 0, &hd) != CVS_OK) return 3;
    const size_t n = (size_t)rows * cols;
    std::vector<float> in(n), out(n), dense(n);
    for (int r = 0; r < rows; ++r) {
        std::memcpy(&in[(size_t)r * cols], thin.ptr(r), (size_t)cols * sizeof(float));
        std::memcpy(&dense[(size_t)r * cols], img.ptr(r), (size_t)cols * sizeof(float));
    }
    cvs_plane pimg = {dense.data(), rows, cols, (size_t)cols * sizeof(float), CVS_MEM_HOST};
    if (cvs_setup(hd, &pimg, CVS_SETUP_BASIS) != CVS_OK) return 3;
    cvs_plane pi = {in.data(), rows, cols, (size_t)cols * sizeof(float), CVS_MEM_HOST};
    cvs_plane po = {out.data(), rows, cols, (size_t)cols * sizeof(float), CVS_MEM_HOST};
    if (cvs_link(hd, 1, &pi, 10.0f, 40.0f, 8, 60.0f, &po, 0) != CVS_OK) return 4;
    cvs_destroy(hd);

    long abi = 0, on = 0, on_plain = 0;
    for (int r = 0; r < rows; ++r) {
        abi += std::memcmp(both.ptr(r), &out[(size_t)r * cols], (size_t)cols * sizeof(float)) != 0;
        for (int c = 0; c < cols; ++c) {
            on += both(r, c) == 255.0f;
            on_plain += plain(r, c) == 255.0f;
        }
    }
    const long d_prune = rows_differ(both, pruned), d_hyst = rows_differ(plain, linked), d_g4 = rows_differ(both4, both);
    if (d_prune || d_hyst || d_g4 || abi || on == 0 || on >= on_plain) {
        std::printf("link: rows that differ -- from hysteresis + prune %ld, from hysteresis %ld, G4 %ld, C ABI %ld; %ld / %ld pixels on\n",
                    d_prune, d_hyst, d_g4, abi, on, on_plain);
        return 1;
    }
    std::printf("link OK (%ld of %ld linked pixels kept)\n", on, on_plain);
    return 0;
}
