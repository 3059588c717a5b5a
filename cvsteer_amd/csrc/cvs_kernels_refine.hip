// cvs_kernels_refine.hip -- contour edgels (extension beyond the reference): the sub-pixel position and strength of every point of a chain
// list (cvs_chain_refine) and one record of measures per chain (cvs_chain_measures), for gfx950.
//
// k_chain_refine is a gather: one lane per point, the point read as one 8-byte pair, the 3 x 3 neighbourhood of the un-thinned map and theta
// read where the point says -- consecutive points of a chain are 8-neighbours, so the gathers of a wave fall on few lines.  The samples, the
// weight and the major axis are those of nonmax_body (cvs_kernels_contour.hip), operation for operation; the offset along the direction
// across the contour is the vertex of the parabola through (backward, m, forward).  A coordinate is an ADDRESS here: it is compared with
// rows / cols (unsigned) before any load, and a point outside the image stores NaN.
// The measures follow the split of cvs_kernels_polyline.hip: one wave per chain of at most kPlWaveMax points, one 256-lane workgroup per
// longer chain on a bounded grid.  A lane adds its points in ascending order, the lanes are combined by a butterfly, the waves in wave
// order: the order of the additions is fixed by the chain's length alone.  Plain vector stores only; there is no atomic.
// Built with -ffp-contract=off: every product and sum below rounds on its own, as the contract in include/cvsteer_hip.h says.
#include <hip/hip_runtime.h>

#include "cvs_chain_device.h"
#include "cvs_device_math.h"
#include "cvs_refine.h"

namespace cvs {

__global__ __launch_bounds__(256) void k_chain_refine(const RefineArgs a)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_points) return;
    const IntPair p = reinterpret_cast<const IntPair*>(a.points)[i];
    const int x = p.x, y = p.y;
    FloatPair* dst = reinterpret_cast<FloatPair*>(a.xy) + i;
    if ((unsigned)x >= (unsigned)a.cols || (unsigned)y >= (unsigned)a.rows) {   // not a pixel: no plane is read
        const float nan = __int_as_float(0x7fc00000);
        *dst = FloatPair{nan, nan};
        if (a.strength) a.strength[i] = nan;
        return;
    }
    auto at = [&](int r, int c) -> float {
        return ((unsigned)r < (unsigned)a.rows && (unsigned)c < (unsigned)a.cols) ? a.map.p[(size_t)r * a.map.pitch + c] : 0.0f;
    };
    // all ten loads before the first use: they do not depend on each other
    const float u_l = at(y - 1, x - 1), u_c = at(y - 1, x), u_r = at(y - 1, x + 1);
    const float m_l = at(y, x - 1), m = at(y, x), m_r = at(y, x + 1);
    const float d_l = at(y + 1, x - 1), d_c = at(y + 1, x), d_r = at(y + 1, x + 1);
    const float th = a.theta.p[(size_t)y * a.theta.pitch + x];

    float s, c;
    sincos_any(th, s, c);
    const float ax = fabsf(c), ay = fabsf(s);
    const bool major_x = ax >= ay;   // NaN: false, and w is NaN
    const float w = major_x ? __fdiv_rn(ay, ax) : __fdiv_rn(ax, ay);
    const float om = 1.0f - w;
    const bool cpos = c >= 0.0f;   // forward column step +1
    const bool spos = s >= 0.0f;   // forward row step -1 (the direction across the contour is (c, -s))
    const float f_l = spos ? u_l : d_l, f_c = spos ? u_c : d_c, f_r = spos ? u_r : d_r;
    const float b_l = spos ? d_l : u_l, b_c = spos ? d_c : u_c, b_r = spos ? d_r : u_r;
    const float diag_f = cpos ? f_r : f_l, diag_b = cpos ? b_l : b_r;
    const float side_f = major_x ? (cpos ? m_r : m_l) : f_c;
    const float side_b = major_x ? (cpos ? m_l : m_r) : b_c;
    const float vf = __fadd_rn(__fmul_rn(om, side_f), __fmul_rn(w, diag_f));
    const float vb = __fadd_rn(__fmul_rn(om, side_b), __fmul_rn(w, diag_b));

    const float da = __fsub_rn(m, vb), db = __fsub_rn(m, vf), diff = __fsub_rn(da, db);
    const bool keep = da > 0.0f && db >= 0.0f;   // the keep test of the thinning; false for NaN: then no offset, and the sample itself
    const float t = keep ? __fmul_rn(0.5f, __fdiv_rn(diff, __fadd_rn(da, db))) : 0.0f;
    const float tw = keep ? __fmul_rn(t, w) : 0.0f;
    const float tx = major_x ? t : tw, ty = major_x ? tw : t;
    *dst = FloatPair{__fadd_rn((float)x, cpos ? tx : -tx), __fadd_rn((float)y, spos ? -ty : ty)};
    if (a.strength) a.strength[i] = keep ? __fadd_rn(m, __fmul_rn(0.25f, __fmul_rn(diff, t))) : m;
}

// ---------------------------------------------------------------------------------------
// Measures.  What a lane, a wave and a workgroup have added up so far; two of them are merged by ms_merge, which is commutative bit for bit
// (integer sums, IEEE additions, and (value, index) pairs ordered by value first and index second).
// ---------------------------------------------------------------------------------------
constexpr int kMsNone = 0x7fffffff;   // index of "no point yet"

struct MsAcc {
    int axial, diagonal, other;
    float peak, weakest;
    int peak_i, weakest_i;   // index inside the chain
    double sum, length;
};

__device__ __forceinline__ MsAcc ms_zero() { return MsAcc{0, 0, 0, -INFINITY, INFINITY, kMsNone, kMsNone, 0.0, 0.0}; }

__device__ __forceinline__ void ms_merge(MsAcc& a, const MsAcc& o)
{
    a.axial += o.axial;
    a.diagonal += o.diagonal;
    a.other += o.other;
    if (o.peak > a.peak || (o.peak == a.peak && o.peak_i < a.peak_i)) {
        a.peak = o.peak;
        a.peak_i = o.peak_i;
    }
    if (o.weakest < a.weakest || (o.weakest == a.weakest && o.weakest_i < a.weakest_i)) {
        a.weakest = o.weakest;
        a.weakest_i = o.weakest_i;
    }
    a.sum = a.sum + o.sum;
    a.length = a.length + o.length;
}

__device__ __forceinline__ void ms_wave_merge(MsAcc& a)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        MsAcc o;
        o.axial = __shfl_xor(a.axial, d, 64);
        o.diagonal = __shfl_xor(a.diagonal, d, 64);
        o.other = __shfl_xor(a.other, d, 64);
        o.peak = __shfl_xor(a.peak, d, 64);
        o.weakest = __shfl_xor(a.weakest, d, 64);
        o.peak_i = __shfl_xor(a.peak_i, d, 64);
        o.weakest_i = __shfl_xor(a.weakest_i, d, 64);
        o.sum = __shfl_xor(a.sum, d, 64);
        o.length = __shfl_xor(a.length, d, 64);
        ms_merge(a, o);
    }
}

// the points first, first + stride, ... of chain t and the steps that leave them (step i goes from point i to point i + 1, the closing step of
// a closed chain from the last point to the first)
__device__ __forceinline__ MsAcc ms_gather(const MeasureArgs& a, const ChainEntry& t, int first, int stride)
{
    MsAcc acc = ms_zero();
    const int L = t.len, steps = L - 1 + ((t.flags & kChainClosed) ? 1 : 0);
    const IntPair* P = reinterpret_cast<const IntPair*>(a.points) + (size_t)t.start;
    const FloatPair* X = a.xy ? reinterpret_cast<const FloatPair*>(a.xy) + (size_t)t.start : nullptr;
    const float* S = a.strength ? a.strength + (size_t)t.start : nullptr;
    for (int i = first; i < L; i += stride) {
        if (S) {
            const float v = S[i];
            acc.sum = acc.sum + (double)v;
            if (v > acc.peak || (v == acc.peak && i < acc.peak_i)) {   // (false for NaN)
                acc.peak = v;
                acc.peak_i = i;
            }
            if (v < acc.weakest || (v == acc.weakest && i < acc.weakest_i)) {
                acc.weakest = v;
                acc.weakest_i = i;
            }
        }
        if (i >= steps) continue;
        const int j = i + 1 == L ? 0 : i + 1;
        const IntPair p = P[i], q = P[j];
        const long long dx = (long long)q.x - p.x, dy = (long long)q.y - p.y;
        const long long adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
        if (adx + ady == 1) ++acc.axial;
        else if (adx == 1 && ady == 1) ++acc.diagonal;
        else ++acc.other;
        double ex = (double)dx, ey = (double)dy;
        if (X) {
            const FloatPair xp = X[i], xq = X[j];
            ex = (double)xq.x - (double)xp.x;
            ey = (double)xq.y - (double)xp.y;
        }
        acc.length = acc.length + sqrt(ex * ex + ey * ey);
    }
    return acc;
}

__device__ __forceinline__ void ms_store(uint32_t* table, long long c, const ChainEntry& t, const MsAcc& acc)
{
    uint32_t* r = table + (size_t)kMeasureWords * c;
    if (t.len == 0) {
#pragma unroll
        for (int k = 0; k < kMeasureWords; ++k) r[k] = k == 3 ? 0xffffffffu : 0u;
        return;
    }
    const unsigned long long sum = (unsigned long long)__double_as_longlong(acc.sum);
    const unsigned long long len = (unsigned long long)__double_as_longlong(acc.length);
    r[0] = (uint32_t)acc.axial;
    r[1] = (uint32_t)acc.diagonal;
    r[2] = (uint32_t)acc.other;
    r[3] = (uint32_t)(acc.peak_i == kMsNone ? -1 : t.start + acc.peak_i);
    r[4] = __float_as_uint(acc.peak);
    r[5] = __float_as_uint(acc.weakest);
    r[6] = (uint32_t)sum;
    r[7] = (uint32_t)(sum >> 32);
    r[8] = (uint32_t)len;
    r[9] = (uint32_t)(len >> 32);
}

__global__ __launch_bounds__(256) void k_measure_wave(const MeasureArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= a.n_chains) return;
    const ChainEntry t = chain_or_empty(a.chains, c, a.n_points);   // (a broken entry: an empty chain, the all-zero record)
    if (t.len > kPlWaveMax) return;   // k_measure_block's
    MsAcc acc = ms_gather(a, t, lane, 64);
    ms_wave_merge(acc);
    if (lane == 0) ms_store(a.table, c, t, acc);
}

__global__ __launch_bounds__(256) void k_measure_block(const MeasureArgs a)
{
    __shared__ unsigned long long lm[4];
    __shared__ MsAcc part[4];
    long_chains(a.chains, a.n_chains, a.n_points, kPlWaveMax, lm, [&](long long c, const ChainEntry& t) {
        const int tid = threadIdx.x;
        MsAcc acc = ms_gather(a, t, tid, 256);
        ms_wave_merge(acc);
        __syncthreads();   // `part` is free again: the chain before has been read to its end
        if ((tid & 63) == 0) part[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) {
            MsAcc all = part[0];
            ms_merge(all, part[1]);
            ms_merge(all, part[2]);
            ms_merge(all, part[3]);
            ms_store(a.table, c, t, all);
        }
    });
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
hipError_t launch_chain_refine(const RefineArgs& a, hipStream_t s)
{
    if (a.rows <= 0 || a.cols <= 0 || !a.map.p || !a.theta.p || !a.points || a.n_points < 1 || !a.xy) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_chain_refine, dim3((unsigned)(((long long)a.n_points + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

static bool measure_ok(const MeasureArgs& a)
{
    return a.n_points >= 0 && (a.points || a.n_points == 0) && a.chains && a.n_chains >= 1 && a.table;
}

hipError_t launch_measure_wave(const MeasureArgs& a, hipStream_t s)
{
    if (!measure_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_measure_wave, dim3((unsigned)(((long long)a.n_chains + 3) / 4)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_measure_block(const MeasureArgs& a, hipStream_t s)
{
    if (!measure_ok(a)) return hipErrorInvalidValue;
    const long long slices = ((long long)a.n_chains + 255) / 256;
    hipLaunchKernelGGL(k_measure_block, dim3((unsigned)(slices < kPlMaxGrid ? slices : kPlMaxGrid)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace cvs
