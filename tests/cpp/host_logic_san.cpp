// host_logic_san.cpp -- the host logic of libcvsteer_hip.so that needs no device, under AddressSanitizer +
// UndefinedBehaviorSanitizer: argument checks (check_plane), the overlap rules of include/cvsteer_hip.h (planes_overlap against
// a byte-for-byte model on random views; find_overlap, the contour tail's sorted check, against the plain loop over planes_overlap), the
// CVS_OPTS parser on hostile strings, the state layout arithmetic (layout_state on
// every kind / size / grouping: offsets inside the block, no two planes sharing an element), the plane-run and one-resource classifier
// of cvs_layout.h (a table of layouts with the answer every call site gave before it existed) and the tap generator.  A cvs_context is
// a plain struct: it is built here without a HIP call; no entry point that touches the device is called.
// Built and run by tools/run_sanitizers.sh and tests/test_sanitizers_cpu.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Icvsteer_amd/csrc -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       tests/cpp/host_logic_san.cpp cvsteer_amd/csrc/{cvs_handle,cvs_tune,cvs_state,cvs_taps}.cpp -L/opt/rocm/lib -lamdhip64 -lpthread
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "cvs_context.h"
#include "cvs_layout.h"

namespace cvs {
// the two kernel-side symbols the host objects refer to (never reached here)
hipError_t launch_u8_to_f32(const uint8_t*, size_t, int, int, float*, size_t, hipStream_t) { return hipErrorUnknown; }
bool basis_fast_path(int, int, const float (*)[kMaxTaps]) { return true; }
}  // namespace cvs

static unsigned long long rs = 0x2545f4914f6cdd1dull;
static unsigned rnd()
{
    rs ^= rs << 13;
    rs ^= rs >> 7;
    rs ^= rs << 17;
    return (unsigned)(rs >> 20);
}
#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::fprintf(stderr, "host_logic_san: %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

int main()
{
    using namespace cvs;
    cvs_context ctx;
    cvs_handle h = &ctx;
    // ---- check_plane ----
    alignas(16) static float buf[64 * 64];
    cvs_plane ok{buf, 8, 8, 8 * sizeof(float), CVS_MEM_HOST};
    REQUIRE(check_plane(h, &ok, "p") == CVS_OK);
    REQUIRE(check_plane(h, nullptr, "p") == CVS_E_BADARG);
    cvs_plane p = ok; p.rows = 0; REQUIRE(check_plane(h, &p, "p") == CVS_E_SIZE);
    p = ok; p.cols = -3; REQUIRE(check_plane(h, &p, "p") == CVS_E_SIZE);
    p = ok; p.data = nullptr; REQUIRE(check_plane(h, &p, "p") == CVS_E_BADARG);
    p = ok; p.step = 7 * sizeof(float); REQUIRE(check_plane(h, &p, "p") == CVS_E_SIZE);
    p = ok; p.step = 8 * sizeof(float) + 2; REQUIRE(check_plane(h, &p, "p") == CVS_E_SIZE);
    p = ok; p.mem = 7; REQUIRE(check_plane(h, &p, "p") == CVS_E_BADARG);
    p = ok; p.mem = CVS_MEM_HOST | CVS_DEPTH_U8; REQUIRE(check_plane(h, &p, "p") == CVS_E_BADARG && check_plane(h, &p, "p", true) == CVS_OK);
    p = ok; p.mem = CVS_MEM_HOST | 0x1000; REQUIRE(check_plane(h, &p, "p") == CVS_E_BADARG);
    p = ok; p.data = reinterpret_cast<float*>(reinterpret_cast<char*>(buf) + 2); REQUIRE(check_plane(h, &p, "p") == CVS_E_BADARG);
    p = ok; p.mem = CVS_MEM_HOST | CVS_DEPTH_U8; p.step = 7; REQUIRE(check_plane(h, &p, "p", true) == CVS_E_SIZE);

    // ---- planes_overlap against a byte model: random f32 / 8-bit views into one 4 KiB arena ----
    static unsigned char arena[4096];
    for (int it = 0; it < 20000; ++it) {
        cvs_plane v[2];
        std::set<size_t> bytes[2];
        for (int k = 0; k < 2; ++k) {
            const bool u8 = rnd() & 1;
            const int es = u8 ? 1 : 4;
            const int rows = 1 + rnd() % 6, cols = 1 + rnd() % 6;
            const size_t step = (size_t)(cols + rnd() % 5) * es;
            const size_t span = (size_t)(rows - 1) * step + (size_t)cols * es;
            const size_t off = (rnd() % (sizeof arena - span)) / es * es;
            v[k] = cvs_plane{reinterpret_cast<float*>(arena + off), rows, cols, step, CVS_MEM_HOST | (u8 ? CVS_DEPTH_U8 : 0)};
            for (int r = 0; r < rows; ++r)
                for (size_t b = 0; b < (size_t)cols * es; ++b) bytes[k].insert(off + r * step + b);
        }
        bool share = false;
        for (size_t b : bytes[0]) share = share || bytes[1].count(b);
        const bool said = planes_overlap(&v[0], &v[1]);
        REQUIRE(said == planes_overlap(&v[1], &v[0]));
        if (share) REQUIRE(said);                                   // a shared byte is never missed
        if (v[0].step == v[1].step && !share) REQUIRE(!said);       // equal steps are compared exactly
    }
    const cvs_plane* outs[3] = {&ok, nullptr, &ok};
    REQUIRE(check_no_overlap(h, nullptr, outs, 3) == CVS_E_BADARG);   // an output given twice
    REQUIRE(check_point_overlaps(h, {&ok}, {&ok}) == CVS_OK);          // in place: an output may BE an input

    // ---- find_overlap (the contour tail's rule) against the quadratic loop over planes_overlap: random views into the arena and into a second
    // arena "of the other memory kind" (addresses of the two kinds may interleave, their planes never overlap), some without data ----
    {
        static unsigned char other[4096];
        const char* const kIn = "an output plane overlaps an input plane";
        const char* const kOut = "two output planes overlap each other";
        auto same = [](const char* a, const char* b) { return (!a && !b) || (a && b && !std::strcmp(a, b)); };
        auto view = [&]() {
            const bool u8 = rnd() & 1, dev = rnd() % 4 == 0;
            const int es = u8 ? 1 : 4;
            const int rows = 1 + rnd() % 6, cols = 1 + rnd() % 6;
            const size_t step = (size_t)(cols + rnd() % 5) * es;
            const size_t span = (size_t)(rows - 1) * step + (size_t)cols * es;
            // one time in three near the start of the arena, so that cases with several overlaps are common
            const size_t off = (rnd() % (rnd() % 3 ? sizeof arena - span : 256)) / es * es;
            cvs_plane v{reinterpret_cast<float*>((dev ? other : arena) + off), rows, cols, step, (dev ? CVS_MEM_DEVICE : CVS_MEM_HOST) | (u8 ? CVS_DEPTH_U8 : 0)};
            if (rnd() % 8 == 0) v.data = nullptr;
            return v;
        };
        int refused = 0, both = 0;
        for (int it = 0; it < 6000; ++it) {
            cvs_plane ins[4], outs[4];
            const size_t n_in = rnd() % 5, n_out = 1 + rnd() % 4;
            for (size_t k = 0; k < n_in; ++k) ins[k] = view();
            for (size_t k = 0; k < n_out; ++k) outs[k] = view();
            bool with_in = false, with_out = false;
            for (size_t k = 0; k < n_out; ++k) {
                for (size_t j = 0; j < n_in; ++j) with_in = with_in || planes_overlap(&outs[k], &ins[j]);
                for (size_t j = k + 1; j < n_out; ++j) with_out = with_out || planes_overlap(&outs[k], &outs[j]);
            }
            const char* msg = find_overlap(ins, n_in, outs, n_out);
            REQUIRE((msg != nullptr) == (with_in || with_out));
            if (with_in != with_out) REQUIRE(same(msg, with_in ? kIn : kOut));
            if (msg) REQUIRE(same(msg, kIn) || same(msg, kOut));
            REQUIRE(check_disjoint(h, ins, n_in, outs, n_out) == (msg ? CVS_E_BADARG : CVS_OK));
            refused += msg != nullptr;
            both += with_in && with_out;
        }
        REQUIRE(refused > 600 && refused < 5400 && both > 60);   // (the generator exercises every verdict)
        // the cases the three former call sites were written for
        const cvs_plane twice[2] = {ok, ok};
        REQUIRE(same(find_overlap(nullptr, 0, twice, 2), kOut));                      // an output given twice
        REQUIRE(same(find_overlap(&ok, 1, &ok, 1), kIn));                             // an output that IS an input: refused here
        cvs_plane apart = ok;
        apart.data = buf + 1024;
        REQUIRE(find_overlap(twice, 2, &apart, 1) == nullptr);                        // two inputs that are the same plane
        const cvs_plane left{buf, 8, 8, 16 * sizeof(float), CVS_MEM_HOST}, right{buf + 8, 8, 8, 16 * sizeof(float), CVS_MEM_HOST};
        REQUIRE(find_overlap(&left, 1, &right, 1) == nullptr);                        // side-by-side ROI views with one step
        const cvs_plane lr[2] = {left, right};
        REQUIRE(find_overlap(nullptr, 0, lr, 2) == nullptr);
        cvs_plane none = ok;
        none.data = nullptr;
        REQUIRE(find_overlap(&none, 1, &ok, 1) == nullptr && find_overlap(&ok, 1, &none, 1) == nullptr);   // planes without data are skipped
    }

    // ---- CVS_OPTS: hostile strings ----
    const char* opts[] = {"", ",", "=", "autotune", "autotune=", "=3", "autotune=0,layout=9,pyr_strip=-4,batch_ways=99999999999999999999,read_ahead=x",
                          "nt_stores=1,,,,verbose=1,pool_mb=-5", "unknown=1", "autotune=0,autotune=1", ",,,,=,=,=", "layout=2\n", "pool_mb=18446744073709551616"};
    for (const char* o : opts) {
        setenv("CVS_OPTS", o, 1);
        const EnvOpts e = env_opts();
        REQUIRE(e.layout >= -1 && e.layout <= 3 && e.autotune >= -1 && e.autotune <= 1 && e.batch_ways >= -1);
    }
    for (int it = 0; it < 3000; ++it) {
        std::string s;
        const char alphabet[] = "autonelyprsbchwdv_=,0123456789-x \n";
        for (int k = rnd() % 48; k > 0; --k) s += alphabet[rnd() % (sizeof alphabet - 1)];
        setenv("CVS_OPTS", s.c_str(), 1);
        (void)env_opts();
    }
    unsetenv("CVS_OPTS");

    // ---- state layout: every plane inside the block, no two planes sharing an element ----
    for (int kind : {CVS_KIND_G2, CVS_KIND_G4})
        for (int layout : {0, 1, 2})
            for (int merged : {0, 1})
                for (int it = 0; it < 40; ++it) {
                    cvs_context c;
                    c.kind = kind;
                    c.nb = kind == CVS_KIND_G2 ? 7 : 11;
                    c.width = kind == CVS_KIND_G2 ? 4 : 6;
                    c.layout = layout;
                    c.rows = 1 + rnd() % 40;
                    c.cols = 1 + rnd() % 300;
                    c.dense_pitch = round_up((size_t)c.cols, 64);
                    c.layout_stride = round_up(c.dense_pitch * c.rows, 64);
                    const size_t elems = c.layout_stride * (size_t)(c.nb + 5);
                    std::vector<float> block(elems);
                    c.state = block.data();
                    c.state_elems = elems;
                    layout_state(&c, merged != 0);
                    REQUIRE(c.frame_stride <= elems);
                    std::vector<unsigned char> used(elems, 0);
                    for (int idx = 0; idx < c.nb + 5; ++idx) {
                        const PlaneRef r = state_ref(&c, idx);
                        REQUIRE(r.p >= block.data());
                        for (int y = 0; y < c.rows; ++y)
                            for (int x = 0; x < c.cols; ++x) {
                                const size_t o = (size_t)(r.p - block.data()) + (size_t)y * r.pitch + x;
                                REQUIRE(o < elems);
                                REQUIRE(!used[o]);
                                used[o] = 1;
                            }
                    }
                    BasisArgs a{};
                    fill_state_args(&c, a, true);
                    REQUIRE(a.basis == block.data() && a.state_bytes == c.frame_stride * sizeof(float));
                    c.strip_rows = 0;
                    const int sr = default_strip_rows(&c, 1 + rnd() % 9000, 1 + rnd() % 9000, rnd() & 1);
                    REQUIRE(sr >= 2 * (2 * c.width + 1) - 2 * c.width && sr <= 4 * (2 * c.width + 1));
                }

    // ---- plane runs and one-resource spans (cvs_layout.h): made-up addresses, nothing is dereferenced ----
    // One row per layout of n frames x K planes, plane k of frame i at base + i * fstride + k * pstride (+ the row's twist).  `want` is
    // what each call site's own loop answered before the classifier existed: F = g4_pipeline_frames (stride > 0 once n > 1), R =
    // batch_run's regular block, quantize_planes and to_u8_batch (stride >= 0), G = batch_run's gain mode (stride > 0, and frame 0 one
    // resource), U = g4_u8_fused (stride >= 0), B = cvs_steer_bank (stride >= 0 and a whole number of floats).
    {
        enum Twist { NONE, FRAME2_PLUS_1, F1_K1_PLUS_4, STEP_F1_K1, ABSENT_F0_K1, ABSENT_K1 };
        struct Row {
            const char* name;
            int n, K;
            size_t step;
            ptrdiff_t pstride, fstride;
            Twist twist;
            const char* want;   // F R G U B: 'y' / 'n'
            ptrdiff_t stride;   // where accepted
        };
        const int rows = 16;
        const uintptr_t base = 0x40000000u;
        const Row table[] = {
            {"dense [4][3][16][64] f32", 4, 3, 256, 4096, 12288, NONE, "yyyyy", 12288},
            {"the same with padded rows", 4, 3, 320, 5120, 15360, NONE, "yyyyy", 15360},
            {"frames further apart than their planes need", 4, 3, 256, 4096, 65536, NONE, "yyyyy", 65536},
            {"frame 2 moved by one byte", 4, 3, 256, 4096, 12288, FRAME2_PLUS_1, "nnnnn", 0},
            {"plane 1 alone at another stride than planes 0 and 2 (frame 1 of 2 moved by 4 bytes)", 2, 3, 256, 4096, 12288, F1_K1_PLUS_4, "nnnnn", 0},
            {"the same with four frames", 4, 3, 256, 4096, 12288, F1_K1_PLUS_4, "nnnnn", 0},
            {"frame 1, plane 1 with another step", 4, 3, 256, 4096, 12288, STEP_F1_K1, "nnnnn", 0},
            {"plane 1 absent in frame 0 only", 4, 3, 256, 4096, 12288, ABSENT_F0_K1, "nnnnn", 0},
            {"plane 1 absent in every frame", 4, 3, 256, 4096, 12288, ABSENT_K1, "yyyyy", 12288},
            {"stride 0: every frame the same planes", 3, 3, 256, 4096, 0, NONE, "nynyy", 0},
            {"negative stride", 3, 3, 256, 4096, -12288, NONE, "nnnnn", 0},
            {"byte planes, stride not a multiple of 4", 3, 3, 64, 1024, 3074, NONE, "yyyyn", 3074},
            {"n = 1", 1, 3, 256, 4096, 0, NONE, "yyyyy", 0},
            {"n = 2", 2, 3, 256, 4096, 12288, NONE, "yyyyy", 12288},
        };
        const bool zero_ok[5] = {false, true, false, true, true};
        const ptrdiff_t divisor[5] = {1, 1, 1, 1, 4};
        for (const Row& r : table) {
            auto at = [&](int i, int k) {
                PlaneAt p{base + (uintptr_t)(i * r.fstride + k * r.pstride), r.step};
                if (r.twist == FRAME2_PLUS_1 && i == 2) p.addr += 1;
                if (r.twist == F1_K1_PLUS_4 && i == 1 && k == 1) p.addr += 4;
                if (r.twist == STEP_F1_K1 && i == 1 && k == 1) p.step += 64;
                if ((r.twist == ABSENT_F0_K1 && i == 0 && k == 1) || (r.twist == ABSENT_K1 && k == 1)) p = {0, 0};
                return p;
            };
            for (int s = 0; s < 5; ++s) {
                const PlaneRun run = plane_run(r.n, r.K, at, zero_ok[s], divisor[s]);
                if (run.ok != (r.want[s] == 'y') || (run.ok && run.stride != r.stride)) {
                    std::fprintf(stderr, "host_logic_san: plane_run: \"%s\", site %c: ok %d stride %td\n", r.name, "FRGUB"[s], (int)run.ok, run.stride);
                    return 1;
                }
            }
            // frame 0 as one resource: the lowest base, offsets k * pstride, the span up to the end of the last plane
            PlaneAt p0[8] = {};
            for (int k = 0; k < r.K; ++k) p0[k] = at(0, k);
            const OneResource res = one_resource(p0, rows, kMaxResourceBytes);
            REQUIRE(res.ok && res.base == base && res.step == r.step && res.span == (size_t)(r.K - 1) * r.pstride + rows * r.step);
            for (int k = 0; k < r.K; ++k) REQUIRE(!p0[k].addr ? !(res.mask >> k & 1) : (res.mask >> k & 1) && res.off[k] == (unsigned)(k * r.pstride));
        }
        // three planes in any order, the highest ending exactly at the limit of a buffer resource, then one byte beyond it; two steps
        // in one frame; no plane at all
        const size_t plane = (size_t)rows * 1024;
        PlaneAt p[8] = {{base + 4096, 1024}, {0, 0}, {base, 1024}, {0, 0}, {0, 0}, {base + kMaxResourceBytes - plane, 1024}, {0, 0}, {0, 0}};
        OneResource res = one_resource(p, rows, kMaxResourceBytes);
        REQUIRE(res.ok && res.span == kMaxResourceBytes && res.base == base && res.mask == 0x25u && res.off[0] == 4096 && res.off[2] == 0 &&
                res.off[5] == (unsigned)(kMaxResourceBytes - plane));
        p[5].addr += 1;
        res = one_resource(p, rows, kMaxResourceBytes);
        REQUIRE(!res.ok && res.span == kMaxResourceBytes + 1);
        p[5] = {base + 2 * plane, 2048};
        REQUIRE(!one_resource(p, rows, kMaxResourceBytes).ok);
        const PlaneAt none[8] = {};
        res = one_resource(none, rows, kMaxResourceBytes);
        REQUIRE(res.ok && res.mask == 0 && res.span == 0 && res.base == 0);
        static_assert(kMaxResourceBytes == 0x7ffffff0u, "the host's limit is kMaxPlaneBytes of cvs_kernels_basis.hip");
    }

    // ---- taps ----
    float t[kMaxTaps];
    REQUIRE(host_make_taps(CVS_KIND_G2, 0, 4, 0.67f, t) == 0 && t[4] < 0.f && t[0] == t[8]);
    REQUIRE(host_make_taps(CVS_KIND_G4, 10, 6, 0.5f, t) == 0);
    REQUIRE(host_make_taps(7, 0, 4, 0.67f, t) != 0 && host_make_taps(CVS_KIND_G2, 7, 4, 0.67f, t) != 0 && host_make_taps(CVS_KIND_G2, 0, kMaxWidth + 1, 0.67f, t) != 0);
    float w[kMaxBasis];
    for (float th : {0.f, 0.3f, -1.2f, 3.1415927f}) REQUIRE(host_steer_weights(CVS_KIND_G2, th, w) == 0 && host_steer_weights(CVS_KIND_G4, th, w) == 0);
    std::printf("host_logic_san: argument checks, 20000 + 6000 overlap cases, CVS_OPTS fuzz, 480 state layouts, 14 plane layouts, taps: no sanitizer report\n");
    return 0;
}
