// The facade's contour members (nonMaxSuppression, hysteresis) against the C ABI on the same object, bit for bit.
// Built and run by tests/test_gpu_contours.py with the fish image as raw f32 (path rows cols); prints "contours OK" and exits 0.
#include <cvsteer/SteerableFiltersG2.h>

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
    fa::Mat1f thin, linked;
    f.nonMaxSuppression(edges, thin);
    f.hysteresis(thin, 10.0f, 40.0f, linked);

    // the same through the C ABI: a handle of its own, theta passed explicitly as the facade's getDominantOrientationAngle()
    cvs_handle hd = 0;
    if (cvs_create(CVS_KIND_G2, 4, 0.67f, 0, &hd) != CVS_OK) return 3;
    auto view = [](const fa::Mat1f& a) {
        cvs_plane q;
        q.data = const_cast<float*>(reinterpret_cast<const float*>(a.data));
        q.rows = a.rows;
        q.cols = a.cols;
        q.step = (size_t)a.cols * sizeof(float);
        q.mem = CVS_MEM_HOST;
        return q;
    };
    cvs_plane pimg = view(img);
    if (cvs_setup(hd, &pimg, CVS_SETUP_FULL) != CVS_OK) return 3;
    const fa::Mat1f& theta = f.getDominantOrientationAngle();
    std::vector<float> t2((size_t)rows * cols), l2((size_t)rows * cols);
    fa::Mat1f edges_dense(rows, cols);
    for (int r = 0; r < rows; ++r) std::memcpy(edges_dense.ptr(r), edges.ptr(r), (size_t)cols * sizeof(float));
    fa::Mat1f theta_dense(rows, cols);
    for (int r = 0; r < rows; ++r) std::memcpy(theta_dense.ptr(r), theta.ptr(r), (size_t)cols * sizeof(float));
    cvs_plane pe = view(edges_dense), pt = view(theta_dense);
    cvs_plane pt2 = {t2.data(), rows, cols, (size_t)cols * sizeof(float), CVS_MEM_HOST};
    cvs_plane pl2 = {l2.data(), rows, cols, (size_t)cols * sizeof(float), CVS_MEM_HOST};
    if (cvs_nonmax(hd, &pt, 1, &pe, &pt2) != CVS_OK) return 4;
    if (cvs_hysteresis(hd, 1, &pt2, 10.0f, 40.0f, &pl2, 0) != CVS_OK) return 4;
    cvs_destroy(hd);

    long bad = 0, kept = 0;
    for (int r = 0; r < rows; ++r) {
        bad += std::memcmp(thin.ptr(r), &t2[(size_t)r * cols], (size_t)cols * sizeof(float)) != 0;
        bad += std::memcmp(linked.ptr(r), &l2[(size_t)r * cols], (size_t)cols * sizeof(float)) != 0;
        for (int c = 0; c < cols; ++c) kept += linked(r, c) == 255.0f;
    }
    if (bad || kept == 0) {
        std::printf("contours: %ld rows differ, %ld pixels kept\n", bad, kept);
        return 1;
    }
    std::printf("contours OK (%ld pixels kept)\n", kept);
    return 0;
}
