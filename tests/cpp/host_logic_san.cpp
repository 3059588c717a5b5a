// host_logic_san.cpp -- the host logic of libcvsteer_hip.so that needs no device, under AddressSanitizer +
// UndefinedBehaviorSanitizer: argument checks (check_plane), the overlap rules of include/cvsteer_hip.h (planes_overlap against
// a byte-for-byte model on random views; find_overlap, the contour tail's sorted check, against the plain loop over planes_overlap), the
// CVS_OPTS parser on hostile strings, the state layout arithmetic (layout_state on
// every kind / size / grouping: offsets inside the block, no two planes sharing an element), the plane-run and one-resource classifier
// of cvs_layout.h (a table of layouts with the answer every call site gave before it existed), what the overlapped host paths share
// (cvs_overlap.h: the run walker against a plane-by-plane copy on random layouts, the chunk schedule, the shard blocks, the worker gate
// between two threads) and the tap generator.  A cvs_context is a plain struct: it is built here without a HIP call; no entry point
// that touches the device is called.
// Built and run by tools/run_sanitizers.sh and tests/test_sanitizers_cpu.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Icvsteer_amd/csrc -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       tests/cpp/host_logic_san.cpp cvsteer_amd/csrc/{cvs_handle,cvs_tune,cvs_state,cvs_taps}.cpp -L/opt/rocm/lib -lamdhip64 -lpthread
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "cvs_context.h"
#include "cvs_layout.h"
#include "cvs_overlap.h"

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

// ---- cvs_overlap.h: the run walker against a plane-by-plane, row-by-row copy ----
// The host copies of the batch layer on memcpy: a "device" arena holds n = frames x K planes back to back, a "host" arena holds them where
// the draw put them -- right behind each other, behind a hole, with padded rows, in descending order, frame by frame descending -- and is
// reached as cvs_batch.cpp reaches it, through a table of eight planes per frame.  Both directions, 1- and 4-byte elements.  The arenas are
// heap blocks of exactly the size in use (ASan sees a copy that leaves them) and carry a marker wherever no plane lies.
static int check_walk_runs()
{
    using namespace cvs;
    const unsigned char kMark = 0xa5;
    int long_runs = 0, across_frames = 0, padded_planes = 0, descending = 0;
    for (int it = 0; it < 6000; ++it) {
        const size_t esz = rnd() & 1 ? 4 : 1;
        const int rows = 1 + rnd() % 4, cols = 1 + rnd() % 6, K = 1 + rnd() % 3, frames = 1 + rnd() % 5;
        const size_t n = (size_t)K * frames, rowb = cols * esz, plane = rows * rowb;
        const bool up = rnd() & 1;
        // n places in ascending address order; the next place starts where this one ends unless a hole is drawn in front of it
        struct Place { size_t off, step; };
        std::vector<Place> place(n);
        size_t cur = 16;
        for (Place& p : place) {
            const unsigned kind = rnd() % 8;
            if (kind == 0) cur += esz * (1 + rnd() % 9);
            p = {cur, rowb + (kind == 1 || kind == 2 ? esz * (1 + rnd() % 3) : 0)};
            cur += rows * p.step;
        }
        std::vector<unsigned char> host(cur + 16), dev(16 + n * plane + 16);
        // which place plane i takes: in order, all descending, or the frames descending with each frame's planes in order
        const unsigned mode = rnd() % 4;
        int sel[3];
        for (int j = 0; j < K; ++j) sel[j] = 2 * j + (rnd() & 1);
        std::vector<PlaneAt> table((size_t)frames * 8, PlaneAt{0, 0});
        for (size_t i = 0; i < n; ++i) {
            const Place& p = place[mode == 2 ? n - 1 - i : mode == 3 ? (frames - 1 - i / K) * K + i % K : i];
            table[i / K * 8 + sel[i % K]] = {reinterpret_cast<uintptr_t>(host.data()) + p.off, p.step};
        }
        auto at = [&](size_t i) { return table[i / K * 8 + sel[i % K]]; };
        for (unsigned char& b : (up ? host : dev)) b = (unsigned char)rnd();
        for (unsigned char& b : (up ? dev : host)) b = kMark;
        // the model: every plane on its own, row by row
        std::vector<unsigned char> want_host = host, want_dev = dev;
        for (size_t i = 0; i < n; ++i)
            for (int r = 0; r < rows; ++r) {
                const size_t h = at(i).addr - reinterpret_cast<uintptr_t>(host.data()) + r * at(i).step, d = 16 + i * plane + r * rowb;
                if (up) std::memcpy(&want_dev[d], &host[h], rowb);
                else std::memcpy(&want_host[h], &dev[d], rowb);
            }
        // the maximal runs of dense planes lying back to back, counted on their own
        size_t runs = 0, pitched_want = 0;
        for (size_t i = 0; i < n; ++i) {
            if (at(i).step != rowb) ++pitched_want;
            else if (i == 0 || at(i - 1).step != rowb || at(i).addr != at(i - 1).addr + plane) ++runs;
        }
        size_t linear_calls = 0, pitched_calls = 0, linear_planes = 0;
        unsigned char* staged = dev.data() + 16;
        const bool done = walk_runs(
            n, plane, rowb, at,
            [&](size_t first, size_t count, uintptr_t addr) {
                ++linear_calls;
                linear_planes += count;
                long_runs += count > 1;
                across_frames += first / K != (first + count - 1) / K;
                if (up) std::memcpy(staged + first * plane, reinterpret_cast<void*>(addr), count * plane);
                else std::memcpy(reinterpret_cast<void*>(addr), staged + first * plane, count * plane);
                return true;
            },
            [&](size_t i, uintptr_t addr, size_t step) {
                ++pitched_calls;
                for (int r = 0; r < rows; ++r) {
                    if (up) std::memcpy(staged + i * plane + r * rowb, reinterpret_cast<void*>(addr + r * step), rowb);
                    else std::memcpy(reinterpret_cast<void*>(addr + r * step), staged + i * plane + r * rowb, rowb);
                }
                return true;
            });
        REQUIRE(done);
        REQUIRE(host == want_host && dev == want_dev);   // the planes, and every marker byte around and between them
        REQUIRE(linear_calls == runs && pitched_calls == pitched_want && linear_planes + pitched_calls == n);
        padded_planes += (int)pitched_want;
        descending += mode >= 2 && frames > 1;
    }
    REQUIRE(long_runs > 1500 && across_frames > 500 && padded_planes > 3000 && descending > 1500);   // (the generator reaches every case)

    // fixed layouts on made-up addresses: the calls themselves
    struct Call {
        char what;
        size_t i, count;
        uintptr_t addr;
        size_t step;
        bool operator==(const Call& o) const { return what == o.what && i == o.i && count == o.count && addr == o.addr && step == o.step; }
    };
    const size_t rowb = 64, plane = 4 * rowb, pstep = 80, pplane = 4 * pstep;
    const uintptr_t base = 0x40000000u;
    bool ok = false;
    auto calls = [&](const std::vector<PlaneAt>& planes, size_t fail_at = 0) {
        std::vector<Call> log;
        ok = walk_runs(
            planes.size(), plane, rowb, [&](size_t i) { return planes[i]; },
            [&](size_t first, size_t count, uintptr_t addr) { log.push_back({'L', first, count, addr, 0}); return log.size() != fail_at; },
            [&](size_t i, uintptr_t addr, size_t step) { log.push_back({'P', i, 1, addr, step}); return log.size() != fail_at; });
        return log;
    };
    typedef std::vector<Call> Log;
    std::vector<PlaneAt> dense5, padded5;
    for (size_t i = 0; i < 5; ++i) {
        dense5.push_back({base + i * plane, rowb});
        padded5.push_back({base + i * pplane, pstep});
    }
    REQUIRE(calls(dense5) == (Log{{'L', 0, 5, base, 0}}) && ok);                                    // all dense: one call
    Log all_padded = calls(padded5);
    REQUIRE(ok && all_padded.size() == 5);                                                           // all padded: no linear call
    for (size_t i = 0; i < 5; ++i) REQUIRE(all_padded[i] == (Call{'P', i, 1, base + i * pplane, pstep}));
    REQUIRE(calls({{base, rowb}}) == (Log{{'L', 0, 1, base, 0}}) && ok);                            // a single plane
    REQUIRE(calls({{base, pstep}}) == (Log{{'P', 0, 1, base, pstep}}) && ok);
    REQUIRE(calls({}).empty() && ok);
    // a dense plane right in front of a padded one and right behind it: three calls, in order
    REQUIRE(calls({{base, rowb}, {base + plane, pstep}, {base + plane + pplane, rowb}}) ==
            (Log{{'L', 0, 1, base, 0}, {'P', 1, 1, base + plane, pstep}, {'L', 2, 1, base + plane + pplane, 0}}) && ok);
    // a padded plane ends the run for good: the dense plane behind it does not join it, even where its address continues it
    REQUIRE(calls({{base, rowb}, {base + 16 * plane, pstep}, {base + plane, rowb}}) ==
            (Log{{'L', 0, 1, base, 0}, {'P', 1, 1, base + 16 * plane, pstep}, {'L', 2, 1, base + plane, 0}}) && ok);
    // two planes that are the same plane, and a step back by one plane: no run
    REQUIRE(calls({{base, rowb}, {base, rowb}, {base - plane, rowb}}).size() == 3 && ok);
    // a callback that fails: false, and nothing is called after it -- L(0,2) P(2) L(3,2) P(5) is the whole walk
    const std::vector<PlaneAt> mixed = {{base, rowb}, {base + plane, rowb}, {base + 8 * plane, pstep}, {base + 20 * plane, rowb}, {base + 21 * plane, rowb},
                                        {base + 30 * plane, pstep}};
    const Log whole = calls(mixed);
    REQUIRE(ok && whole == (Log{{'L', 0, 2, base, 0}, {'P', 2, 1, base + 8 * plane, pstep}, {'L', 3, 2, base + 20 * plane, 0}, {'P', 5, 1, base + 30 * plane, pstep}}));
    for (size_t fail_at = 1; fail_at <= 4; ++fail_at) {
        const Log cut = calls(mixed, fail_at);
        REQUIRE(!ok && cut == Log(whole.begin(), whole.begin() + fail_at));
    }
    REQUIRE(calls(dense5, 1).size() == 1 && !ok);   // (the run that is still open when the planes end)
    return 0;
}

// ---- cvs_overlap.h: the chunk schedule of a shard and the blocks of the ranks ----
static int check_chunks_and_shards()
{
    using namespace cvs;
    // computed from the expression host_rank held before chunk_starts existed
    const struct { int n; std::vector<int> starts; } pinned[] = {
        {1, {0, 1}}, {2, {0, 1, 2}}, {3, {0, 1, 3}}, {4, {0, 1, 4}}, {5, {0, 1, 3, 5}}, {8, {0, 1, 3, 8}}, {16, {0, 1, 3, 7, 16}},
        {31, {0, 1, 3, 7, 15, 31}}, {32, {0, 1, 3, 7, 15, 32}}, {33, {0, 1, 3, 7, 15, 33}}, {64, {0, 2, 6, 14, 30, 64}},
        {100, {0, 3, 9, 21, 45, 100}}, {1000, {0, 31, 93, 217, 465, 1000}}};
    for (const auto& p : pinned) REQUIRE(chunk_starts(p.n, false) == p.starts);
    for (int n = 1; n <= 4096; ++n) {
        const std::vector<int> c = chunk_starts(n, false);
        REQUIRE(c.size() >= 2 && c.size() <= 6 && c.front() == 0 && c.back() == n);
        for (size_t k = 1; k < c.size(); ++k) REQUIRE(c[k] > c[k - 1]);
        REQUIRE(chunk_starts(n, true) == (std::vector<int>{0, n}));
    }
    for (int n = 0; n <= 200; ++n)
        for (int world = 1; world <= 17; ++world) {
            int next = 0;
            for (int rank = 0; rank < world; ++rank) {
                int lo = -1, hi = -1;
                shard_range(n, world, rank, &lo, &hi);
                REQUIRE(lo == next && hi >= lo);   // the blocks tile [0, n) in rank order
                for (int f = lo; f < hi; ++f) REQUIRE(f * world / n == rank);
                next = hi;
            }
            REQUIRE(next == n);
        }
    return 0;
}

// ---- cvs_overlap.h: the gate between the thread that queues and the worker ----
// Every wait below is bounded: a wake-up that gets lost fails the check (the worker is then released by stop() and joined) instead of
// hanging it; only a stop() that releases nobody cannot be joined, and ends the program.
static bool reaches(const std::atomic<int>& v, int want)
{
    const auto until = std::chrono::steady_clock::now() + std::chrono::seconds(20);
    while (v.load() < want && std::chrono::steady_clock::now() < until) std::this_thread::sleep_for(std::chrono::microseconds(200));
    return v.load() >= want;
}

static int check_gate()
{
    using namespace cvs;
    for (int round = 0; round < 20; ++round) {
        // the worker takes items 0 ... kItems - 1 as they are published, one or several at a time, and sees each exactly once, in order
        const int kItems = 200;
        Gate gate;
        std::atomic<int> taken(0);
        std::vector<int> seen;
        bool stopped_early = false;
        std::thread worker([&] {
            for (int k = 0; k < kItems; ++k) {
                if (!gate.wait(k)) { stopped_early = true; return; }
                seen.push_back(k);
                taken.store(k + 1);
            }
        });
        for (int k = 0; k < kItems;) {
            k = std::min(kItems, k + 1 + (int)(rnd() % 3));
            gate.publish(k);
            if (rnd() % 4 == 0) REQUIRE(reaches(taken, k) || (gate.stop(), worker.join(), false));   // the worker blocks again behind item k - 1
        }
        const bool all = reaches(taken, kItems);
        gate.stop();   // after everything was published: nothing for a worker that has finished
        worker.join();
        REQUIRE(all && !stopped_early && (int)seen.size() == kItems);
        for (int k = 0; k < kItems; ++k) REQUIRE(seen[k] == k);
        REQUIRE(!gate.wait(0));   // stopped stays stopped
    }
    // stop() releases a worker that waits for an item that never comes, and wait() says so
    for (int published : {0, 3}) {
        Gate gate;
        std::atomic<int> stage(0);
        bool got = true;
        gate.publish(published);
        std::thread worker([&] {
            bool before = true;
            for (int k = 0; k < published; ++k) before = before && gate.wait(k);
            stage.store(before ? 1 : -100);
            got = gate.wait(published);
            stage.store(2);
        });
        REQUIRE(reaches(stage, 1) || (gate.stop(), worker.join(), false));
        std::this_thread::sleep_for(std::chrono::milliseconds(2));   // (the worker is most likely inside wait() now; either way it must come back)
        REQUIRE(stage.load() == 1);
        gate.stop();
        if (!reaches(stage, 2)) {
            std::fprintf(stderr, "host_logic_san: Gate::stop() did not release the waiting worker\n");
            std::_Exit(1);
        }
        worker.join();
        REQUIRE(!got);
    }
    return 0;
}

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

    if (check_walk_runs() || check_chunks_and_shards() || check_gate()) return 1;

    // ---- taps ----
    float t[kMaxTaps];
    REQUIRE(host_make_taps(CVS_KIND_G2, 0, 4, 0.67f, t) == 0 && t[4] < 0.f && t[0] == t[8]);
    REQUIRE(host_make_taps(CVS_KIND_G4, 10, 6, 0.5f, t) == 0);
    REQUIRE(host_make_taps(7, 0, 4, 0.67f, t) != 0 && host_make_taps(CVS_KIND_G2, 7, 4, 0.67f, t) != 0 && host_make_taps(CVS_KIND_G2, 0, kMaxWidth + 1, 0.67f, t) != 0);
    float w[kMaxBasis];
    for (float th : {0.f, 0.3f, -1.2f, 3.1415927f}) REQUIRE(host_steer_weights(CVS_KIND_G2, th, w) == 0 && host_steer_weights(CVS_KIND_G4, th, w) == 0);
    std::printf("host_logic_san: argument checks, 20000 + 6000 overlap cases, CVS_OPTS fuzz, 480 state layouts, 14 plane layouts, 6000 copy walks, chunk schedule, shards, gate, taps: no sanitizer report\n");
    return 0;
}
