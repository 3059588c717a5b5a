// The facade's vector steer overloads (cvs_steer_bank) against the per-angle Mat1f& overloads on the same object, bit for bit.
// Built and run by tests/test_gpu_steer_bank.py; prints "steer_bank OK" and exits 0 when every plane matches.
#include <cvsteer/SteerableFiltersG2.h>
#include <cvsteer/SteerableFiltersG4.h>

#include <cstdio>
#include <cstring>
#include <vector>

static bool same(const fa::Mat1f& a, const fa::Mat1f& b)
{
    if (a.rows != b.rows || a.cols != b.cols) return false;
    for (int r = 0; r < a.rows; ++r)
        if (std::memcmp(a.ptr(r), b.ptr(r), (size_t)a.cols * sizeof(float))) return false;
    return true;
}

int main()
{
    const int rows = 97, cols = 130;
    fa::Mat1f img(rows, cols);
    unsigned s = 12345u;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            s = s * 1664525u + 1013904223u;
            img(r, c) = (float)(s >> 8) / 16777216.0f;
        }
    const std::vector<float> thetas = {0.f, 0.3f, -1.2f, 3.14159265f, 5.0f};
    int bad = 0;

    fa::SteerableFiltersG2 f2(img);
    std::vector<fa::Mat1f> g, h, e, m, p;
    f2.steer(thetas, g, h);
    for (size_t k = 0; k < thetas.size(); ++k) {
        fa::Mat1f g1, h1;
        f2.steer(thetas[k], g1, h1);
        bad += !same(g[k], g1) + !same(h[k], h1);
    }
    f2.steer(thetas, g, h, e, m, p);
    for (size_t k = 0; k < thetas.size(); ++k) {
        fa::Mat1f g1, h1, e1, m1, p1;
        f2.steer(thetas[k], g1, h1, e1, m1, p1);
        bad += !same(g[k], g1) + !same(h[k], h1) + !same(e[k], e1) + !same(m[k], m1) + !same(p[k], p1);
    }

    fa::SteerableFiltersG4 f4(img);
    std::vector<fa::Mat1f> g4, h4;
    f4.steer(thetas, g4, h4);
    for (size_t k = 0; k < thetas.size(); ++k) {
        fa::Mat1f g1, h1;
        f4.steer(thetas[k], g1, h1);
        bad += !same(g4[k], g1) + !same(h4[k], h1);
    }
    if (g.size() != thetas.size() || g4.size() != thetas.size()) ++bad;
    if (bad) {
        std::printf("steer_bank: %d planes differ\n", bad);
        return 1;
    }
    std::printf("steer_bank OK\n");
    return 0;
}
