// cvs_kernels_segments.hip -- contour segments (extension beyond the reference): the total-least-squares line through the points of every
// polyline span (cvs_polyline_segments), one record per vertex, for gfx950.
//
// The split is that of the measures (cvs_kernels_refine.hip): one group of lanes per span of at most kPlWaveMax points, and one 256-lane
// workgroup per longer span on a bounded grid that finds its spans by ballot (ms_long_entries).  The group is kSgGroup = 16 lanes, four
// spans to a wave: the spans of real contours have a handful of points (3.4 on average on a 4096^2 noise frame, 23 at most), and a whole
// wave per span executes every instruction of the search, the derivation and the store for three points -- 8.0 ms against 2.7 ms there
// (tools/segments_probe.py times this build beside a 64-lane twin).  A lane adds the six terms of every 16th or
// 256th point in ascending order, the lanes are combined by a butterfly, the four waves of a workgroup through LDS in wave order: the order
// of the additions is fixed by the span's count alone.  The butterfly leaves the same six sums in EVERY lane of the group, bit for bit (IEEE
// addition commutes), so every lane derives the same line from them -- the finishing lane's values need no broadcast -- and all lanes make
// the second pass, for dmax, over points that are still in L2.  The group's first lane stores the record as words.  No atomic, no scratch,
// nothing read back.
// What the tables say is checked before it is used as an address (sg_span); coordinates are never addresses.
// Built with -ffp-contract=off: every product, sum and difference below rounds on its own, as the contract in include/cvsteer_hip.h says;
// the double divisions and square roots are the correctly rounded ones.
#include <hip/hip_runtime.h>

#include "cvs_chain_device.h"
#include "cvs_segments.h"

#ifndef CVS_SEG_GROUP
#define CVS_SEG_GROUP 16   // (64: the twin `make segwave` builds for tools/segments_probe.py)
#endif

namespace cvs {

namespace {

constexpr int kSgGroup = CVS_SEG_GROUP;   // lanes that share a span of at most kPlWaveMax points
static_assert(kSgGroup == 16 || kSgGroup == 32 || kSgGroup == 64, "a power of two that divides a wave, and a shuffle width");

// the span that starts at a vertex.  count == 0: no span (first and chain are still the record's)
struct SgSpan {
    int first, count, chain, flags;
    int start, len;   // the chain's range of `points`: position first + j wraps to start once it reaches start + len
};

__device__ __forceinline__ SgSpan sg_span(const SegmentArgs& a, long long k)
{
    const int i0 = a.index[k];
    const int lo = entry_of(a.polylines, a.n_chains, k);   // the polyline the vertex belongs to, if the table is what it should be
    SgSpan t{i0, 0, lo, 0, 0, 0};
    const ChainEntry ch = chain_entry(a.chains, lo, a.n_points);
    const int32_t* pl = a.polylines + 4 * (size_t)lo;
    const int S = ch.start, L = ch.len, F = ch.flags, vs = pl[0], vl = pl[1];
    const long long p_end = (long long)S + L, v_end = (long long)vs + vl;
    if (!CVS_INSIDE_POINTS(S, L, a.n_points)) return t;   // the chain does not lie inside points (ch.ok(), spelled on the locals: the
                                                          // form that keeps both kernels at their registers)
    if (vs < 0 || k < vs || k >= v_end) return t;                    // the vertex is not one of the polyline the search found
    if (i0 < S || i0 >= p_end) return t;
    t.start = S;
    t.len = L;
    if (k + 1 < v_end) {
        if (k + 1 >= a.n_vertices) return t;
        const int i1 = a.index[k + 1];
        if (i1 >= p_end || i1 <= i0) return t;
        t.count = i1 - i0 + 1;
    } else if (F & kChainClosed) {
        const int iv = a.index[vs];   // 0 <= vs <= k < n_vertices
        if (iv < S || iv > i0) return t;
        t.count = (S + L - i0) + (iv - S + 1);   // <= L + 1
        t.flags = kSegWraps;
    }
    return t;
}

// point j of a span: its weight and its offsets from the span's first pixel (x0, y0)
struct SgPoint {
    double w, dx, dy;
};

__device__ __forceinline__ SgPoint sg_point(const SegmentArgs& a, const SgSpan& t, int j, double x0, double y0)
{
    long long p = (long long)t.first + j;
    if (p >= (long long)t.start + t.len) p -= t.len;
    SgPoint q;
    if (a.xy) {
        const FloatPair v = reinterpret_cast<const FloatPair*>(a.xy)[p];
        q.dx = (double)v.x - x0;
        q.dy = (double)v.y - y0;
    } else {
        const IntPair v = reinterpret_cast<const IntPair*>(a.points)[p];
        q.dx = (double)v.x - x0;
        q.dy = (double)v.y - y0;
    }
    q.w = 1.0;
    if (a.strength) {
        const float s = a.strength[p];
        q.w = s > 0.0f ? (double)s : 0.0;   // (false for NaN)
    }
    return q;
}

struct SgSums {
    double w, sx, sy, sxx, sxy, syy;
};

__device__ __forceinline__ void sg_add(SgSums& a, const SgSums& o)
{
    a.w = a.w + o.w;
    a.sx = a.sx + o.sx;
    a.sy = a.sy + o.sy;
    a.sxx = a.sxx + o.sxx;
    a.sxy = a.sxy + o.sxy;
    a.syy = a.syy + o.syy;
}

// the terms of the points first, first + stride, ... of a span, added in ascending order
__device__ __forceinline__ SgSums sg_gather(const SegmentArgs& a, const SgSpan& t, int first, int stride, double x0, double y0)
{
    SgSums acc{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = first; j < t.count; j += stride) {
        const SgPoint q = sg_point(a, t, j, x0, y0);
        const double wx = q.w * q.dx, wy = q.w * q.dy;
        acc.w = acc.w + q.w;
        acc.sx = acc.sx + wx;
        acc.sy = acc.sy + wy;
        acc.sxx = acc.sxx + wx * q.dx;
        acc.sxy = acc.sxy + wx * q.dy;
        acc.syy = acc.syy + wy * q.dy;
    }
    return acc;
}

// the butterflies over a group of W consecutive lanes (W = 64: a wave); every lane of the group ends with the same value
template <int W>
__device__ __forceinline__ void sg_group_add(SgSums& a)
{
#pragma unroll
    for (int d = W / 2; d > 0; d >>= 1) {
        SgSums o;
        o.w = __shfl_xor(a.w, d, W);
        o.sx = __shfl_xor(a.sx, d, W);
        o.sy = __shfl_xor(a.sy, d, W);
        o.sxx = __shfl_xor(a.sxx, d, W);
        o.sxy = __shfl_xor(a.sxy, d, W);
        o.syy = __shfl_xor(a.syy, d, W);
        sg_add(a, o);
    }
}

template <int W>
__device__ __forceinline__ double sg_group_max(double m)
{
#pragma unroll
    for (int d = W / 2; d > 0; d >>= 1) {
        const double o = __shfl_xor(m, d, W);
        m = o > m ? o : m;
    }
    return m;
}

// the line of six sums: the derived sequence of the contract, operation for operation
struct SgLine {
    double mx, my, cx, cy, ux, uy, t0, t1, rms;
    bool degenerate;
};

__device__ __forceinline__ SgLine sg_line(const SgSums& s, const SgPoint& pf, const SgPoint& pl, double x0, double y0)
{
    SgLine g;
    g.mx = __ddiv_rn(s.sx, s.w);
    g.my = __ddiv_rn(s.sy, s.w);
    const double a = s.sxx - s.sx * g.mx, b = s.sxy - s.sx * g.my, c = s.syy - s.sy * g.my;
    const double d = a - c, e = b + b, r = __dsqrt_rn(d * d + e * e);
    const double vx = d >= 0.0 ? d + r : e, vy = d >= 0.0 ? e : r - d;   // the eigenvector of the larger eigenvalue, without cancellation
    const double hh = __dsqrt_rn(vx * vx + vy * vy);
    double ux = __ddiv_rn(vx, hh), uy = __ddiv_rn(vy, hh);
    const double qx = pl.dx - pf.dx, qy = pl.dy - pf.dy, along = ux * qx + uy * qy;
    if (along < 0.0 || (along == 0.0 && (ux < 0.0 || (ux == 0.0 && uy < 0.0)))) {   // from the first point towards the last
        ux = -ux;
        uy = -uy;
    }
    g.cx = x0 + g.mx;
    g.cy = y0 + g.my;
    g.t0 = ux * (pf.dx - g.mx) + uy * (pf.dy - g.my);
    g.t1 = ux * (pl.dx - g.mx) + uy * (pl.dy - g.my);
    const double lmin = 0.5 * ((a + c) - r);
    g.rms = __dsqrt_rn(__ddiv_rn(lmin > 0.0 ? lmin : 0.0, s.w));
    g.ux = ux;
    g.uy = uy;
    g.degenerate = !(s.w > 0.0) || !(hh > 0.0) || hh == INFINITY;
    if (g.degenerate) g.ux = g.uy = g.t0 = g.t1 = g.rms = __longlong_as_double(0x7ff8000000000000ll);
    return g;
}

// the largest distance from the line among the points first, first + stride, ... of a span
__device__ __forceinline__ double sg_far(const SegmentArgs& a, const SgSpan& t, const SgLine& g, int first, int stride, double x0, double y0)
{
    double m = 0.0;
    for (int j = first; j < t.count; j += stride) {
        const SgPoint q = sg_point(a, t, j, x0, y0);
        const double v = fabs(g.ux * (q.dy - g.my) - g.uy * (q.dx - g.mx));
        m = v > m ? v : m;
    }
    return m;
}

__device__ __forceinline__ void sg_put(uint32_t* r, int word, double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    r[word] = (uint32_t)u;
    r[word + 1] = (uint32_t)(u >> 32);
}

__device__ __forceinline__ void sg_store_empty(uint32_t* table, long long k, const SgSpan& t)
{
    uint32_t* r = table + (size_t)kSegmentWords * k;
    r[0] = (uint32_t)t.first;
    r[1] = 0u;
    r[2] = (uint32_t)t.chain;
#pragma unroll
    for (int i = 3; i < kSegmentWords; ++i) r[i] = 0u;
}

__device__ __forceinline__ void sg_store(uint32_t* table, long long k, const SgSpan& t, const SgSums& s, const SgLine& g, double dmax)
{
    uint32_t* r = table + (size_t)kSegmentWords * k;
    r[0] = (uint32_t)t.first;
    r[1] = (uint32_t)t.count;
    r[2] = (uint32_t)t.chain;
    r[3] = (uint32_t)(t.flags | (g.degenerate ? kSegDegenerate : 0));
    sg_put(r, 4, s.w);
    sg_put(r, 6, s.sx);
    sg_put(r, 8, s.sy);
    sg_put(r, 10, s.sxx);
    sg_put(r, 12, s.sxy);
    sg_put(r, 14, s.syy);
    sg_put(r, 16, g.cx);
    sg_put(r, 18, g.cy);
    sg_put(r, 20, g.ux);
    sg_put(r, 22, g.uy);
    sg_put(r, 24, g.t0);
    sg_put(r, 26, g.t1);
    sg_put(r, 28, g.rms);
    sg_put(r, 30, g.degenerate ? g.rms : dmax);
}

__device__ __forceinline__ void sg_origin(const SegmentArgs& a, const SgSpan& t, double& x0, double& y0)
{
    const IntPair o = reinterpret_cast<const IntPair*>(a.points)[t.first];
    x0 = (double)o.x;
    y0 = (double)o.y;
}

}  // namespace

__global__ __launch_bounds__(256) void k_segments_wave(const SegmentArgs a)
{
    // a group of kSgGroup lanes per vertex; what follows diverges between the groups of a wave and never inside one, and no shuffle
    // crosses a group
    const int lane = threadIdx.x & (kSgGroup - 1);
    const long long k = (long long)blockIdx.x * (256 / kSgGroup) + threadIdx.x / kSgGroup;
    if (k >= a.n_vertices) return;
    const SgSpan t = sg_span(a, k);
    if (t.count > kPlWaveMax) return;   // k_segments_block's
    if (t.count == 0) {
        if (lane == 0) sg_store_empty(a.table, k, t);
        return;
    }
    double x0, y0;
    sg_origin(a, t, x0, y0);
    SgSums s = sg_gather(a, t, lane, kSgGroup, x0, y0);
    sg_group_add<kSgGroup>(s);
    const SgLine g = sg_line(s, sg_point(a, t, 0, x0, y0), sg_point(a, t, t.count - 1, x0, y0), x0, y0);
    double far = 0.0;
    if (!g.degenerate) far = sg_group_max<kSgGroup>(sg_far(a, t, g, lane, kSgGroup, x0, y0));
    if (lane == 0) sg_store(a.table, k, t, s, g, far);
}

__global__ __launch_bounds__(256) void k_segments_block(const SegmentArgs a)
{
    __shared__ unsigned long long lm[4];
    __shared__ SgSums part[4];
    __shared__ double far4[4];
    ms_long_entries(
        a.n_vertices, lm, [&](long long k) { return sg_span(a, k).count > kPlWaveMax; },
        [&](long long k) {
            const int tid = threadIdx.x;
            const SgSpan t = sg_span(a, k);
            double x0, y0;
            sg_origin(a, t, x0, y0);
            SgSums s = sg_gather(a, t, tid, 256, x0, y0);
            sg_group_add<64>(s);
            __syncthreads();   // `part` and `far4` are free again: the span before has been read to its end
            if ((tid & 63) == 0) part[tid >> 6] = s;
            __syncthreads();
            s = part[0];   // every lane: the four waves in wave order
            sg_add(s, part[1]);
            sg_add(s, part[2]);
            sg_add(s, part[3]);
            const SgLine g = sg_line(s, sg_point(a, t, 0, x0, y0), sg_point(a, t, t.count - 1, x0, y0), x0, y0);
            double far = 0.0;
            if (!g.degenerate) far = sg_group_max<64>(sg_far(a, t, g, tid, 256, x0, y0));   // (a whole wave or none: the lanes hold the same sums)
            if ((tid & 63) == 0) far4[tid >> 6] = far;
            __syncthreads();
            if (tid == 0) {
#pragma unroll
                for (int w = 1; w < 4; ++w) far = far4[w] > far ? far4[w] : far;
                sg_store(a.table, k, t, s, g, far);
            }
        });
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
static bool segments_ok(const SegmentArgs& a)
{
    return a.n_points >= 0 && (a.points || a.n_points == 0) && a.n_chains >= 1 && a.chains && a.polylines && a.n_vertices >= 1 && a.index && a.table;
}

hipError_t launch_segments_wave(const SegmentArgs& a, hipStream_t s)
{
    if (!segments_ok(a)) return hipErrorInvalidValue;
    constexpr int per = 256 / kSgGroup;   // vertices per workgroup
    hipLaunchKernelGGL(k_segments_wave, dim3((unsigned)(((long long)a.n_vertices + per - 1) / per)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_segments_block(const SegmentArgs& a, hipStream_t s)
{
    if (!segments_ok(a)) return hipErrorInvalidValue;
    const long long slices = ((long long)a.n_vertices + 255) / 256;
    hipLaunchKernelGGL(k_segments_block, dim3((unsigned)(slices < kPlMaxGrid ? slices : kPlMaxGrid)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace cvs
