// The facade's orientationPeaks (cvs_orientation_peaks) on G2 and G4 objects against the C call on the same handle, bit for bit, and its
// return value against the count plane.  Built and run by tests/test_gpu_peaks.py; prints "peaks OK" and exits 0 when everything matches.
#include <cvsteer/SteerableFiltersG2.h>
#include <cvsteer/SteerableFiltersG4.h>
#include <cvsteer_hip.h>

#include <cstdio>
#include <cstring>
#include <vector>

// the C call into dense host planes of its own
struct Direct {
    std::vector<float> angles, energies;
    std::vector<unsigned char> count;
    int status, most;
};

static Direct direct(cvs_handle h, int rows, int cols, int K, int M, float minEnergy, float minRatio, float minContrast)
{
    Direct d;
    const size_t plane = (size_t)rows * cols;
    d.angles.assign(plane * M, 7.f);
    d.energies.assign(plane * M, 7.f);
    d.count.assign(plane, 7);
    cvs_peaks_cfg cfg;
    cfg.struct_size = (unsigned)sizeof(cfg);
    cfg.n_angles = K;
    cfg.max_peaks = M;
    cfg.min_energy = minEnergy;
    cfg.min_ratio = minRatio;
    cfg.min_contrast = minContrast;
    std::vector<cvs_plane> pa(M), pe(M);
    for (int s = 0; s < M; ++s) {
        cvs_plane p;
        p.rows = rows;
        p.cols = cols;
        p.step = (size_t)cols * sizeof(float);
        p.mem = CVS_MEM_HOST;
        p.data = d.angles.data() + plane * s;
        pa[s] = p;
        p.data = d.energies.data() + plane * s;
        pe[s] = p;
    }
    cvs_plane pc;
    pc.data = reinterpret_cast<float*>(d.count.data());
    pc.rows = rows;
    pc.cols = cols;
    pc.step = (size_t)cols;
    pc.mem = CVS_MEM_HOST | CVS_DEPTH_U8;
    d.status = cvs_orientation_peaks(h, &cfg, pa.data(), pe.data(), &pc);
    d.most = 0;
    for (size_t i = 0; i < plane; ++i) d.most = d.count[i] > d.most ? d.count[i] : d.most;
    return d;
}

static bool same(const fa::Mat1f& a, const float* b, int rows, int cols)
{
    if (a.rows != rows || a.cols != cols) return false;
    for (int r = 0; r < rows; ++r)
        if (std::memcmp(a.ptr(r), b + (size_t)r * cols, (size_t)cols * sizeof(float))) return false;
    return true;
}

template <class F>
static int check(F& f, int rows, int cols, int K, int M, float minEnergy, float minRatio, float minContrast, bool defaults)
{
    std::vector<fa::Mat1f> angles, energies;
    const int most = defaults ? f.orientationPeaks(angles, energies) : f.orientationPeaks(angles, energies, K, M, minEnergy, minRatio, minContrast);
    const Direct d = direct(f.handle(), rows, cols, K, M, minEnergy, minRatio, minContrast);
    int bad = d.status != CVS_OK;
    bad += (int)angles.size() != M || (int)energies.size() != M;
    for (int s = 0; s < M && !bad; ++s)
        bad += !same(angles[s], d.angles.data() + (size_t)rows * cols * s, rows, cols) + !same(energies[s], d.energies.data() + (size_t)rows * cols * s, rows, cols);
    bad += most != d.most || most < 1 || most > M;
    return bad;
}

int main()
{
    const int rows = 97, cols = 130;
    fa::Mat1f img(rows, cols);
    unsigned s = 12345u;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            s = s * 1664525u + 1013904223u;
            img(r, c) = (float)(s >> 8) / 65536.0f;
        }
    int bad = 0;
    fa::SteerableFiltersG2 f2(img);
    bad += check(f2, rows, cols, 16, 2, 0.f, 0.25f, 1e-3f, true);
    bad += check(f2, rows, cols, 32, 4, 10.f, 0.5f, 0.01f, false);
    bad += check(f2, rows, cols, 5, 1, 0.f, 0.f, 0.f, false);
    fa::SteerableFiltersG4 f4(img);
    bad += check(f4, rows, cols, 16, 2, 0.f, 0.25f, 1e-3f, true);
    bad += check(f4, rows, cols, 8, 3, 0.f, 0.f, 0.f, false);
    // a refused call throws, as every facade call does
    bool threw = false;
    try {
        std::vector<fa::Mat1f> a, e;
        f2.orientationPeaks(a, e, 3);
    } catch (const std::exception&) {
        threw = true;
    }
    bad += !threw;
    if (bad) {
        std::printf("peaks: %d checks failed\n", bad);
        return 1;
    }
    std::printf("peaks OK\n");
    return 0;
}
