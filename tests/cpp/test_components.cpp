// The facade's contour-component members (pruneContours, countComponents) against the C ABI on a handle of its own, bit for bit.
// Built and run by tests/test_gpu_components.py with the fish image as raw f32 (path rows cols); prints "components OK" and exits 0.
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
    fa::Mat1f img(rows, cols);
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) return 2;
    for (int r = 0; r < rows; ++r)
        if (std::fread(img.ptr(r), sizeof(float), cols, fp) != (size_t)cols) return 2;
    std::fclose(fp);

    fa::SteerableFiltersG2 f(img);
    fa::Mat1f g, h, e, m, p, edges, dark, bright;
    f.pipeline(img, g, h, e, m, p, edges, dark, bright);
    fa::Mat1f thin, linked, pruned, by_area;
    f.nonMaxSuppression(edges, thin);
    f.hysteresis(thin, 10.0f, 40.0f, linked);
    const int all = f.countComponents(linked);
    const int kept = f.pruneContours(linked, thin, 8, 60.0f, pruned);
    const int kept_area = f.pruneContours(linked, fa::Mat1f(), 8, 0.0f, by_area);
    fa::SteerableFiltersG4 f4(img);   // the G4 class carries the same members; they read the planes passed, not the object's state
    fa::Mat1f pruned4;
    if (f4.countComponents(linked) != all || f4.pruneContours(linked, thin, 8, 60.0f, pruned4) != kept) return 5;

    // the same through the C ABI: dense copies on a handle of its own
    cvs_handle hd = 0;
    if (cvs_create(CVS_KIND_G2, 4, 0.67f, 0, &hd) != CVS_OK) return 3;
    const size_t n = (size_t)rows * cols;
    std::vector<float> mask(n), weight(n), out(n);
    std::vector<int32_t> labels(n);
    for (int r = 0; r < rows; ++r) {
        std::memcpy(&mask[(size_t)r * cols], linked.ptr(r), (size_t)cols * sizeof(float));
        std::memcpy(&weight[(size_t)r * cols], thin.ptr(r), (size_t)cols * sizeof(float));
    }
    cvs_plane pimg = {reinterpret_cast<float*>(img.data), rows, cols, (size_t)cols * sizeof(float), CVS_MEM_HOST};
    fa::Mat1f img_dense(rows, cols);
    for (int r = 0; r < rows; ++r) std::memcpy(img_dense.ptr(r), img.ptr(r), (size_t)cols * sizeof(float));
    pimg.data = reinterpret_cast<float*>(img_dense.data);
    if (cvs_setup(hd, &pimg, CVS_SETUP_BASIS) != CVS_OK) return 3;
    cvs_plane pm = {mask.data(), rows, cols, (size_t)cols * sizeof(float), CVS_MEM_HOST};
    cvs_plane pw = {weight.data(), rows, cols, (size_t)cols * sizeof(float), CVS_MEM_HOST};
    cvs_plane po = {out.data(), rows, cols, (size_t)cols * sizeof(float), CVS_MEM_HOST};
    cvs_plane pl = {reinterpret_cast<float*>(labels.data()), rows, cols, (size_t)cols * sizeof(int32_t), CVS_MEM_HOST | CVS_DEPTH_S32};
    int count = -1, k2 = -1;
    if (cvs_label(hd, &pm, &pl, &count) != CVS_OK) return 4;
    if (cvs_contour_prune(hd, 1, &pm, &pw, 8, 60.0f, &po, &k2) != CVS_OK) return 4;
    std::vector<cvs_component> table((size_t)(count > 0 ? count : 1));
    if (cvs_component_stats(hd, &pl, count, &pw, table.data(), CVS_MEM_HOST) != CVS_OK) return 4;
    cvs_destroy(hd);

    long bad = 0, on = 0, big = 0, strong = 0;
    for (int r = 0; r < rows; ++r) {
        bad += std::memcmp(pruned.ptr(r), &out[(size_t)r * cols], (size_t)cols * sizeof(float)) != 0;
        bad += std::memcmp(pruned4.ptr(r), &out[(size_t)r * cols], (size_t)cols * sizeof(float)) != 0;
        for (int c = 0; c < cols; ++c) on += pruned(r, c) == 255.0f;
    }
    for (int k = 0; k < count; ++k) {
        big += table[(size_t)k].area >= 8;
        strong += table[(size_t)k].area >= 8 && table[(size_t)k].peak >= 60.0f;
    }
    if (bad || count != all || k2 != kept || strong != kept || big != kept_area || all <= 0 || kept <= 0 || kept > all || on == 0) {
        std::printf("components: %ld rows differ; components %d / %d, kept %d / %d / %ld, by area %d / %ld, %ld pixels on\n", bad, all, count,
                    kept, k2, strong, kept_area, big, on);
        return 1;
    }
    std::printf("components OK (%d components, %d kept, %ld pixels)\n", all, kept, on);
    return 0;
}
