// cvs_kernels_polyline.hip -- contour polylines (extension beyond the reference): Ramer-Douglas-Peucker simplification of all chains of a
// chain table at once (cvs_chain_polylines), for gfx950.
//
// The recursion of the split rule has a depth that depends on the shape of a contour, so it lives INSIDE a kernel: the lanes that own a chain
// walk its segments from left to right with no stack -- a byte (or bit) of keep flags per point, lo = 0, and per step hi = the next kept
// index after lo, the lanes stride over (lo, hi) and reduce (largest value, smallest index); a split marks that index and goes on with the
// same lo (the new hi is the split point), no split moves lo to hi.  The kept set does not depend on the order of the visits, so this is the
// recursion's result.  The launch sequence depends on (n_points, n_chains) alone:
//
//   1  k_pl_keep_wave    one wave per chain of <= kPlWaveMax points: points and flags in registers, shuffles only
//      k_pl_keep_block   one workgroup per longer chain: flags in memory, the reduction through LDS
//   2  k_pl_count, k_scan_partials (cvs_kernels_components.hip), k_pl_apply   first vertex of every chain, the table, the total
//   3  k_pl_emit_wave, k_pl_emit_block   vertex k of chain c at first[c] + k: ranks from ballots with a running offset
//
// All values are int64 (exact for |x|, |y| < 2^28); the one floating-point test is two double multiplications and a comparison.  Stores are
// plain vector stores at positions that come from the scan; there is no atomic.  A table entry that does not lie inside `points` is an
// empty chain, so no load or store leaves the arrays whatever a device table holds; coordinates are never used as addresses.
#include <hip/hip_runtime.h>

#include "cvs_chain_device.h"
#include "cvs_polyline.h"

namespace cvs {

// v(i) of the split rule for the point (qx, qy) against the segment a -> b: |cross| for a != b, the squared distance from a otherwise.
// For coordinates beyond the contract's range the products wrap instead of overflowing and the sign bit is dropped: a value is never negative,
// so a segment with an interior point always has a split candidate inside it.
__device__ __forceinline__ long long pl_value(int ax, int ay, int bx, int by, int qx, int qy)
{
    typedef unsigned long long u64;
    const u64 top = ~0ull >> 1;
    const long long px = (long long)qx - ax, py = (long long)qy - ay;
    if (ax == bx && ay == by) return (long long)(((u64)px * (u64)px + (u64)py * (u64)py) & top);
    const long long dx = (long long)bx - ax, dy = (long long)by - ay;
    const u64 v = (u64)dx * (u64)py - (u64)dy * (u64)px;
    return (long long)(((long long)v < 0 ? 0ull - v : v) & top);
}

// the contract's test on the largest value of a segment: num > e2 * den, one rounding per operation
__device__ __forceinline__ bool pl_split(long long v, int ax, int ay, int bx, int by, double e2)
{
    typedef unsigned long long u64;
    if (ax == bx && ay == by) return (double)v > e2 * 1.0;
    const long long dx = (long long)bx - ax, dy = (long long)by - ay;
    const double dv = (double)v, den = (double)(long long)((u64)dx * (u64)dx + (u64)dy * (u64)dy);
    return dv * dv > e2 * den;
}

// (largest value, smallest index) over the wave; every lane gets the result
__device__ __forceinline__ void pl_wave_best(long long& v, int& i)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const long long ov = __shfl_xor(v, d, 64);
        const int oi = __shfl_xor(i, d, 64);
        if (ov > v || (ov == v && oi < i)) {
            v = ov;
            i = oi;
        }
    }
}

// ---------------------------------------------------------------------------------------
// Step 1, short chains.  Lane l holds the points l, l + 64, ... of its wave's chain; the keep flags are kPlWaveWords 64-bit words, the same in
// every lane.  Points and flags are named registers (PlQuad, PlMask), chosen by selects: an array indexed at run time would leave the
// registers.
// ---------------------------------------------------------------------------------------
static_assert(kPlWaveWords == 4, "PlQuad and PlMask hold four words");
struct PlQuad {
    int a, b, c, d;
};
struct PlMask {
    unsigned long long a, b, c, d;
};

__device__ __forceinline__ int pl_sel(const PlQuad& q, int k) { return k == 0 ? q.a : (k == 1 ? q.b : (k == 2 ? q.c : q.d)); }

// point i of the chain, from the lane that holds it
__device__ __forceinline__ int pl_point(const PlQuad& q, int i) { return __shfl(pl_sel(q, i >> 6), i & 63, 64); }

__device__ __forceinline__ void pl_set(PlMask& m, int i)
{
    const unsigned long long bit = 1ull << (i & 63);
    const int w = i >> 6;
    m.a |= w == 0 ? bit : 0ull;
    m.b |= w == 1 ? bit : 0ull;
    m.c |= w == 2 ? bit : 0ull;
    m.d |= w == 3 ? bit : 0ull;
}

// the smallest set bit above lo, `none` if there is none
__device__ __forceinline__ int pl_next(const PlMask& m, int lo, int none)
{
    const int w = lo >> 6, sh = (lo & 63) + 1;
    const unsigned long long above = sh == 64 ? 0ull : ~0ull << sh;
    const unsigned long long a = m.a & (w == 0 ? above : 0ull), b = m.b & (w == 1 ? above : (w < 1 ? ~0ull : 0ull));
    const unsigned long long c = m.c & (w == 2 ? above : (w < 2 ? ~0ull : 0ull)), d = m.d & (w == 3 ? above : (w < 3 ? ~0ull : 0ull));
    if (a) return __ffsll((long long)a) - 1;
    if (b) return 64 + __ffsll((long long)b) - 1;
    if (c) return 128 + __ffsll((long long)c) - 1;
    if (d) return 192 + __ffsll((long long)d) - 1;
    return none;
}

// the lane's candidate among its own four points: the largest value inside (lo, hi), the earlier point on a tie
__device__ __forceinline__ void pl_try(int i, int lo, int hi, long long v, long long& bv, int& bi)
{
    if (i > lo && i < hi && v > bv) {
        bv = v;
        bi = i;
    }
}

__global__ __launch_bounds__(256) void k_pl_keep_wave(const int32_t* points, int n_points, const int32_t* chains, int n_chains, double e2,
                                                      uint8_t* keep, int32_t* count)
{
    const int lane = threadIdx.x & 63;
    const long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= n_chains) return;
    const ChainEntry t = chain_or_empty(chains, c, n_points);   // (a broken entry: an empty chain)
    if (t.len > kPlWaveMax) return;   // k_pl_keep_block's
    if (t.len == 0) {
        if (lane == 0) count[c] = 0;
        return;
    }
    const int L = t.len, closed = t.flags & kChainClosed, n = L + closed;   // n: points of the virtual list
    const int32_t* P = points + 2 * (size_t)t.start;
    const int i0 = lane, i1 = 64 + lane, i2 = 128 + lane, i3 = 192 + lane;
    PlQuad px, py;
    px.a = i0 < L ? P[2 * i0] : 0, py.a = i0 < L ? P[2 * i0 + 1] : 0;
    px.b = i1 < L ? P[2 * i1] : 0, py.b = i1 < L ? P[2 * i1 + 1] : 0;
    px.c = i2 < L ? P[2 * i2] : 0, py.c = i2 < L ? P[2 * i2 + 1] : 0;
    px.d = i3 < L ? P[2 * i3] : 0, py.d = i3 < L ? P[2 * i3 + 1] : 0;
    PlMask m = {1ull, 0ull, 0ull, 0ull};
    if (!closed || L <= 2) pl_set(m, L - 1);   // (L <= 2: every point is kept)
    if (L > 2) {
        int lo = 0, hi = pl_next(m, 0, n - 1);
        while (lo < n - 1) {
            if (hi - lo >= 2) {
                const int ib = hi == L ? 0 : hi;   // the virtual last point of a closed chain is its first
                const int ax = pl_point(px, lo), ay = pl_point(py, lo), bx = pl_point(px, ib), by = pl_point(py, ib);
                long long bv = -1;
                int bi = 0x7fffffff;
                pl_try(i0, lo, hi, pl_value(ax, ay, bx, by, px.a, py.a), bv, bi);
                pl_try(i1, lo, hi, pl_value(ax, ay, bx, by, px.b, py.b), bv, bi);
                pl_try(i2, lo, hi, pl_value(ax, ay, bx, by, px.c, py.c), bv, bi);
                pl_try(i3, lo, hi, pl_value(ax, ay, bx, by, px.d, py.d), bv, bi);
                pl_wave_best(bv, bi);
                if (bi < hi && pl_split(bv, ax, ay, bx, by, e2)) {   // (bi < hi: always)
                    pl_set(m, bi);
                    hi = bi;
                    continue;
                }
            }
            lo = hi;
            hi = pl_next(m, lo, n - 1);
        }
    }
    uint8_t* K = keep + (size_t)t.start;
    if (i0 < L) K[i0] = (uint8_t)((m.a >> lane) & 1ull);
    if (i1 < L) K[i1] = (uint8_t)((m.b >> lane) & 1ull);
    if (i2 < L) K[i2] = (uint8_t)((m.c >> lane) & 1ull);
    if (i3 < L) K[i3] = (uint8_t)((m.d >> lane) & 1ull);
    if (lane == 0) count[c] = __popcll(m.a) + __popcll(m.b) + __popcll(m.c) + __popcll(m.d);
}

// ---------------------------------------------------------------------------------------
// Step 1, long chains.  The flags are the chain's own bytes of KEEP.  A split is marked by one lane and read again only behind a barrier (the
// one in front of every search for the next kept point).  That search is done by every wave on its own, 64 flags at a time; the last point of
// the virtual list counts as kept without being read, so the search ends whatever the bytes hold.
// ---------------------------------------------------------------------------------------
struct PlBest {
    long long v[2][4];
    int i[2][4];
};

__device__ __forceinline__ int pl_scan_next(const uint8_t* keep, int lo, int last)
{
    const int lane = threadIdx.x & 63;
    for (int base = lo + 1;; base += 64) {
        const int i = base + lane;
        const bool f = i >= last || keep[i] != 0;
        const unsigned long long b = __ballot(f);
        if (b) return base + __ffsll((long long)b) - 1;
    }
}

__global__ __launch_bounds__(256) void k_pl_keep_block(const int32_t* points, int n_points, const int32_t* chains, int n_chains, double e2,
                                                       uint8_t* keep, int32_t* count)
{
    __shared__ unsigned long long lm[4];
    __shared__ PlBest best;
    long_chains(chains, n_chains, n_points, kPlWaveMax, lm, [&](long long c, const ChainEntry& t) {
        const int tid = threadIdx.x, wave = tid >> 6;
        const int L = t.len, closed = t.flags & kChainClosed, last = L + closed - 1;   // last: index of the last point of the virtual list
        const int32_t* P = points + 2 * (size_t)t.start;
        uint8_t* K = keep + (size_t)t.start;
        for (int i = tid; i < L; i += 256) K[i] = (uint8_t)((i == 0 || (!closed && i == L - 1)) ? 1 : 0);
        __syncthreads();   // `best` is free again: the chain before has been read to its end
        int lo = 0, hi = last, kept = closed ? 1 : 2, par = 0;
        while (lo < last) {
            if (hi - lo >= 2) {
                const int ib = hi == L ? 0 : hi;
                const int ax = P[2 * (size_t)lo], ay = P[2 * (size_t)lo + 1], bx = P[2 * (size_t)ib], by = P[2 * (size_t)ib + 1];
                long long bv = -1;
                int bi = 0x7fffffff;
                for (int i = lo + 1 + tid; i < hi; i += 256) {   // ascending: a later tie does not replace an earlier one
                    const long long v = pl_value(ax, ay, bx, by, P[2 * (size_t)i], P[2 * (size_t)i + 1]);
                    if (v > bv) {
                        bv = v;
                        bi = i;
                    }
                }
                pl_wave_best(bv, bi);
                if ((tid & 63) == 0) {
                    best.v[par][wave] = bv;
                    best.i[par][wave] = bi;
                }
                __syncthreads();
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const long long ov = best.v[par][w];
                    const int oi = best.i[par][w];
                    if (ov > bv || (ov == bv && oi < bi)) {
                        bv = ov;
                        bi = oi;
                    }
                }
                par ^= 1;   // the next step writes the other half: one barrier per step
                if (bi < hi && pl_split(bv, ax, ay, bx, by, e2)) {   // (bi < hi: always)
                    if (tid == 0) K[bi] = 1;
                    ++kept;
                    hi = bi;
                    continue;
                }
            }
            lo = hi;
            if (lo < last) {
                __syncthreads();   // the marks made so far
                hi = pl_scan_next(K, lo, last);
            }
        }
        if (tid == 0) count[c] = kept;
    });
}

// ---------------------------------------------------------------------------------------
// Step 2.  The exclusive scan of the counts in table order: a lane owns 4 consecutive chains.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ int pl_block_scan(int v, int* ws, int& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) ws[wave] = incl;
    __syncthreads();
    int pre = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int t = ws[w];
        pre += w < wave ? t : 0;
        total += t;
    }
    __syncthreads();   // ws may be used again
    return pre + incl - v;
}

__global__ __launch_bounds__(256) void k_pl_count(const int32_t* count, int n_chains, int32_t* partials)
{
    __shared__ int ws[4];
    const long long c0 = (long long)blockIdx.x * kPlScanBlock + threadIdx.x * 4;
    int s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += c0 + k < n_chains ? count[c0 + k] : 0;
    int total;
    (void)pl_block_scan(s, ws, total);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_pl_apply(int32_t* count, int n_chains, const int32_t* partials, const int32_t* chains, int capacity,
                                                  int32_t* polylines)
{
    __shared__ int ws[4];
    const long long c0 = (long long)blockIdx.x * kPlScanBlock + threadIdx.x * 4;
    int n[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        n[k] = c0 + k < n_chains ? count[c0 + k] : 0;
        s += n[k];
    }
    int total;
    int start = partials[blockIdx.x] + pl_block_scan(s, ws, total);
    const bool table = polylines && (unsigned)partials[gridDim.x] <= (unsigned)capacity;   // the total fits: the table may be written
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (c0 + k >= n_chains) continue;
        if (table) {
            int32_t* t = polylines + 4 * (c0 + k);   // struct cvs_chain: four 4-byte fields
            t[0] = start;
            t[1] = n[k];
            t[2] = chains[4 * (c0 + k) + 2];
            t[3] = 0;
        }
        count[c0 + k] = start;   // from here on: the chain's first vertex
        start += n[k];
    }
}

// ---------------------------------------------------------------------------------------
// Step 3.  The rank of a kept point inside its chain: kept points in the lanes below (a ballot), in the waves below (LDS, workgroup kernel
// only) and in the rounds before (the running offset).
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void pl_store(const int32_t* P, int start, int i, int at, int capacity, int32_t* vertices, int32_t* index)
{
    if ((unsigned)at >= (unsigned)capacity) return;
    vertices[2 * (size_t)at] = P[2 * (size_t)i];
    vertices[2 * (size_t)at + 1] = P[2 * (size_t)i + 1];
    if (index) index[at] = start + i;
}

__global__ __launch_bounds__(256) void k_pl_emit_wave(const int32_t* points, int n_points, const int32_t* chains, int n_chains,
                                                      const uint8_t* keep, const int32_t* first, const int32_t* partials, int blocks,
                                                      int capacity, int32_t* vertices, int32_t* index)
{
    const int lane = threadIdx.x & 63;
    const long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= n_chains || (unsigned)partials[blocks] > (unsigned)capacity) return;
    const ChainEntry t = chain_or_empty(chains, c, n_points);   // (a broken entry: an empty chain)
    if (t.len == 0 || t.len > kPlWaveMax) return;
    const int32_t* P = points + 2 * (size_t)t.start;
    const uint8_t* K = keep + (size_t)t.start;
    int at = first[c];
    for (int i0 = 0; i0 < t.len; i0 += 64) {
        const int i = i0 + lane;
        const bool f = i < t.len && K[i] != 0;
        const unsigned long long b = __ballot(f);
        if (f) pl_store(P, t.start, i, at + __popcll(b & ((1ull << lane) - 1ull)), capacity, vertices, index);
        at += __popcll(b);
    }
}

__global__ __launch_bounds__(256) void k_pl_emit_block(const int32_t* points, int n_points, const int32_t* chains, int n_chains,
                                                       const uint8_t* keep, const int32_t* first, const int32_t* partials, int blocks,
                                                       int capacity, int32_t* vertices, int32_t* index)
{
    __shared__ unsigned long long lm[4];
    __shared__ int wc[2][4];
    if ((unsigned)partials[blocks] > (unsigned)capacity) return;   // (the same for every lane of the launch)
    long_chains(chains, n_chains, n_points, kPlWaveMax, lm, [&](long long c, const ChainEntry& t) {
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        const int32_t* P = points + 2 * (size_t)t.start;
        const uint8_t* K = keep + (size_t)t.start;
        int at = first[c], par = 0;
        __syncthreads();   // wc is free again: the chain before has been read to its end
        for (int i0 = 0; i0 < t.len; i0 += 256) {
            const int i = i0 + tid;
            const bool f = i < t.len && K[i] != 0;
            const unsigned long long b = __ballot(f);
            if (lane == 0) wc[par][wave] = __popcll(b);
            __syncthreads();
            int pre = 0, tot = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int n = wc[par][w];
                pre += w < wave ? n : 0;
                tot += n;
            }
            par ^= 1;   // the next round writes the other half: one barrier per round
            if (f) pl_store(P, t.start, i, at + pre + __popcll(b & ((1ull << lane) - 1ull)), capacity, vertices, index);
            at += tot;
        }
    });
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
static unsigned wave_grid(int n_chains) { return (unsigned)(((long long)n_chains + 3) / 4); }
static unsigned block_grid(int n_chains)
{
    const long long slices = ((long long)n_chains + 255) / 256;
    return (unsigned)(slices < kPlMaxGrid ? slices : kPlMaxGrid);
}
static bool lists_ok(const int32_t* points, int n_points, const int32_t* chains, int n_chains)
{
    return n_points >= 0 && (points || n_points == 0) && chains && n_chains >= 1;
}

hipError_t launch_pl_keep_wave(const int32_t* points, int n_points, const int32_t* chains, int n_chains, double e2, uint8_t* keep,
                               int32_t* count, hipStream_t s)
{
    if (!lists_ok(points, n_points, chains, n_chains) || !keep || !count) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pl_keep_wave, dim3(wave_grid(n_chains)), dim3(256), 0, s, points, n_points, chains, n_chains, e2, keep, count);
    return hipGetLastError();
}

hipError_t launch_pl_keep_block(const int32_t* points, int n_points, const int32_t* chains, int n_chains, double e2, uint8_t* keep,
                                int32_t* count, hipStream_t s)
{
    if (!lists_ok(points, n_points, chains, n_chains) || !keep || !count) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pl_keep_block, dim3(block_grid(n_chains)), dim3(256), 0, s, points, n_points, chains, n_chains, e2, keep, count);
    return hipGetLastError();
}

hipError_t launch_pl_count(const int32_t* count, int n_chains, int32_t* partials, hipStream_t s)
{
    if (!count || n_chains < 1 || !partials) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pl_count, dim3(pl_scan_blocks(n_chains)), dim3(256), 0, s, count, n_chains, partials);
    return hipGetLastError();
}

hipError_t launch_pl_apply(int32_t* count, int n_chains, const int32_t* partials, const int32_t* chains, int capacity, int32_t* polylines,
                           hipStream_t s)
{
    if (!count || n_chains < 1 || !partials || !chains || capacity < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pl_apply, dim3(pl_scan_blocks(n_chains)), dim3(256), 0, s, count, n_chains, partials, chains, capacity, polylines);
    return hipGetLastError();
}

hipError_t launch_pl_emit_wave(const int32_t* points, int n_points, const int32_t* chains, int n_chains, const uint8_t* keep,
                               const int32_t* first, const int32_t* partials, int capacity, int32_t* vertices, int32_t* index, hipStream_t s)
{
    if (!lists_ok(points, n_points, chains, n_chains) || !keep || !first || !partials || capacity < 1 || !vertices) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pl_emit_wave, dim3(wave_grid(n_chains)), dim3(256), 0, s, points, n_points, chains, n_chains, keep, first, partials,
                       pl_scan_blocks(n_chains), capacity, vertices, index);
    return hipGetLastError();
}

hipError_t launch_pl_emit_block(const int32_t* points, int n_points, const int32_t* chains, int n_chains, const uint8_t* keep,
                                const int32_t* first, const int32_t* partials, int capacity, int32_t* vertices, int32_t* index, hipStream_t s)
{
    if (!lists_ok(points, n_points, chains, n_chains) || !keep || !first || !partials || capacity < 1 || !vertices) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pl_emit_block, dim3(block_grid(n_chains)), dim3(256), 0, s, points, n_points, chains, n_chains, keep, first, partials,
                       pl_scan_blocks(n_chains), capacity, vertices, index);
    return hipGetLastError();
}

}  // namespace cvs
