// cvs_kernels_contour.hip -- contour thinning (extension beyond the reference): non-maximum suppression across the dominant
// orientation (cvs_nonmax) and 8-connected hysteresis linking (cvs_hysteresis), for gfx950.
//
// The reference's callers stop at the energy maps of findEdges / findDarkLines / findBrightLines (G2.cpp:194-212): every contour is a
// band several pixels wide.  These kernels thin those maps to the local maxima across the orientation theta (Freeman & Adelson's
// contour detector, Canny's interpolated suppression) and link the thinned maps by hysteresis, without the maps leaving the device.
// Built with -ffp-contract=off: every product and sum below rounds on its own, as the contract in include/cvsteer_hip.h says.
#include <hip/hip_runtime.h>

#include "cvs_contour.h"
#include "cvs_device_math.h"

namespace cvs {

// ---------------------------------------------------------------------------------------
// k_nonmax: one wave per 62-column tile and strip of rows.  Lane l reads column x0 - 1 + l with one dword load per map and row, so
// lanes 1..62 own the output columns and lanes 0 / 63 are the halo; the left / right neighbours come from the adjacent lanes
// (__shfl_up / __shfl_down), the rows above / below from a rolling three-row window in registers.  Each input row is loaded once per
// strip (plus the halo rows above and below it), the next row's loads are in flight while the current row is decided, and theta is
// read once for all NM maps.  Neighbours outside the image read as 0.0f.
// ---------------------------------------------------------------------------------------
constexpr int kNmsSpan = 62;   // output columns per wave (nonmax_grid in cvs_grid.h counts tiles of this width)

struct Row3 {
    float l, c, r;   // columns x - 1, x, x + 1
};

__device__ __forceinline__ Row3 spread(float v)
{
    return {__shfl_up(v, 1, 64), v, __shfl_down(v, 1, 64)};
}

template <int NM, bool NT>
__device__ __forceinline__ void nonmax_body(const NmsArgs& a)
{
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile * kNmsSpan >= a.cols) return;   // wave-uniform: the whole wave lies right of the image
    const int x = tile * kNmsSpan - 1 + lane;
    const bool xin = x >= 0 && x < a.cols;
    const bool own = lane >= 1 && lane <= kNmsSpan && x < a.cols;
    const int r0 = blockIdx.y * a.strip;
    const int r1 = min(r0 + a.strip, a.rows);
    auto load = [&](const PlaneRef& p, int r, bool want) -> float {
        return (want && xin && r >= 0 && r < a.rows) ? p.p[(size_t)r * p.pitch + x] : 0.0f;
    };
    Row3 up[NM], mid[NM];
    float next[NM];
#pragma unroll
    for (int k = 0; k < NM; ++k) {
        up[k] = spread(load(a.in[k], r0 - 1, true));
        mid[k] = spread(load(a.in[k], r0, true));
        next[k] = load(a.in[k], r0 + 1, true);
    }
    float th = load(a.theta, r0, true);
    for (int r = r0; r < r1; ++r) {
        Row3 dn[NM];
#pragma unroll
        for (int k = 0; k < NM; ++k) {
            dn[k] = spread(next[k]);
            next[k] = load(a.in[k], r + 2, r + 2 <= r1);   // the row after next: in flight while this row is decided
        }
        const float th_next = load(a.theta, r + 1, r + 1 < r1);
        float s, c;
        sincos_any(th, s, c);
        const float ax = fabsf(c), ay = fabsf(s);
        const bool major_x = ax >= ay;   // NaN: false, and w is NaN
        const float w = major_x ? __fdiv_rn(ay, ax) : __fdiv_rn(ax, ay);
        const float om = 1.0f - w;
        const bool cpos = c >= 0.0f;   // forward column step +1
        const bool spos = s >= 0.0f;   // forward row step -1 (the direction across the contour is (c, -s))
#pragma unroll
        for (int k = 0; k < NM; ++k) {
            const Row3 u = up[k], m = mid[k], d = dn[k];
            // the rows of the forward / backward step, as values (selects, no indexing of the window)
            const float f_l = spos ? u.l : d.l, f_c = spos ? u.c : d.c, f_r = spos ? u.r : d.r;
            const float b_l = spos ? d.l : u.l, b_c = spos ? d.c : u.c, b_r = spos ? d.r : u.r;
            const float diag_f = cpos ? f_r : f_l, diag_b = cpos ? b_l : b_r;
            const float side_f = major_x ? (cpos ? m.r : m.l) : f_c;
            const float side_b = major_x ? (cpos ? m.l : m.r) : b_c;
            const float vf = __fadd_rn(__fmul_rn(om, side_f), __fmul_rn(w, diag_f));
            const float vb = __fadd_rn(__fmul_rn(om, side_b), __fmul_rn(w, diag_b));
            const float v = m.c;
            const float o = (v > vb && v >= vf) ? v : 0.0f;
            if (own) {
                float* dst = a.out[k].p + (size_t)r * a.out[k].pitch + x;
                if constexpr (NT) __builtin_nontemporal_store(o, dst);
                else *dst = o;
            }
            up[k] = mid[k];
            mid[k] = dn[k];
        }
        th = th_next;
    }
}

template <int NM, bool NT>
__global__ __launch_bounds__(256) void k_nonmax(const NmsArgs a)
{
    nonmax_body<NM, NT>(a);
}

// the same body for every frame of a batch in one launch: blockIdx.z = frame, its planes those of frame 0 moved by z strides
template <int NM, bool NT>
__global__ __launch_bounds__(256) void k_nms_frames(const NmsArgs a0, const NmsBatch b)
{
    NmsArgs a = a0;
    const long long z = blockIdx.z;
    a.theta.p += z * b.theta_stride;
#pragma unroll
    for (int k = 0; k < NM; ++k) {
        a.in[k].p += z * b.in_stride[k];
        a.out[k].p += z * b.out_stride[k];
    }
    nonmax_body<NM, NT>(a);
}

template <int NM>
static void launch_nonmax_nm(const NmsArgs& a, dim3 grid, hipStream_t s)
{
    if (a.nt_stores) hipLaunchKernelGGL((k_nonmax<NM, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_nonmax<NM, false>), grid, dim3(256), 0, s, a);
}

template <int NM>
static void launch_nonmax_batch_nm(const NmsArgs& a, const NmsBatch& b, dim3 grid, hipStream_t s)
{
    if (a.nt_stores) hipLaunchKernelGGL((k_nms_frames<NM, true>), grid, dim3(256), 0, s, a, b);
    else hipLaunchKernelGGL((k_nms_frames<NM, false>), grid, dim3(256), 0, s, a, b);
}

static bool nonmax_ok(const NmsArgs& a)
{
    if (a.rows <= 0 || a.cols <= 0 || a.n < 1 || a.n > kNmsMax || !a.theta.p) return false;
    for (int k = 0; k < a.n; ++k)
        if (!a.in[k].p || !a.out[k].p) return false;
    return true;
}

// rows per strip and the grid of `frames` frames (cvs_grid.h: nonmax_grid)
static dim3 nonmax_grid(NmsArgs& b, long frames)
{
    const GridDims gd = nonmax_grid(b.rows, b.cols, frames, &b.strip);
    return dim3(gd.x, gd.y, gd.z);
}

hipError_t launch_nonmax(const NmsArgs& a, hipStream_t s)
{
    if (!nonmax_ok(a)) return hipErrorInvalidValue;
    NmsArgs b = a;
    const dim3 grid = nonmax_grid(b, 1);
    if (a.n == 1) launch_nonmax_nm<1>(b, grid, s);
    else if (a.n == 2) launch_nonmax_nm<2>(b, grid, s);
    else launch_nonmax_nm<3>(b, grid, s);
    return hipGetLastError();
}

hipError_t launch_nonmax_batch(const NmsArgs& a, const NmsBatch& nb, hipStream_t s)
{
    if (!nonmax_ok(a) || nb.frames < 1 || nb.frames > 65535) return hipErrorInvalidValue;
    NmsArgs b = a;
    const dim3 grid = nonmax_grid(b, nb.frames);
    if (a.n == 1) launch_nonmax_batch_nm<1>(b, nb, grid, s);
    else if (a.n == 2) launch_nonmax_batch_nm<2>(b, nb, grid, s);
    else launch_nonmax_batch_nm<3>(b, nb, grid, s);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// Hysteresis.  Labels (one byte per pixel, plane z of the launch at lab + z * lab_stride, row pitch lab_pitch bytes): 0 = never kept,
// kWeak, kStrong.  k_hyst_classify writes them; each k_hyst_propagate launch is one pass -- every workgroup loads a tile with a
// one-pixel halo into LDS, promotes weak pixels that touch a strong one until the tile is stable, writes the tile back and, if it
// promoted anything, raises *changed with one vector atomic; k_hyst_emit writes 0 / 255.  Promotion is monotone, so a stale halo
// byte (another workgroup's tile of the same pass) only delays convergence; a pass that changes nothing read only bytes of earlier
// launches, and the labels are then the unique fixed point.
// ---------------------------------------------------------------------------------------
constexpr unsigned char kWeak = 1, kStrong = 2;
constexpr int kHystTileW = 128, kHystTileH = 32;   // 8 lanes per tile row, 16 columns each
constexpr int kHystSeg = kHystTileW / 8;

__global__ __launch_bounds__(256) void k_hyst_classify(const HystArgs a)
{
    const int z = blockIdx.z;
    const PlaneRef& in = a.in[z];
    unsigned char* lab = a.lab + (size_t)z * a.lab_stride;
    for (int r = blockIdx.y; r < a.rows; r += gridDim.y)
        for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < a.cols; x += gridDim.x * blockDim.x) {
            const float v = in.p[(size_t)r * in.pitch + x];
            lab[(size_t)r * a.lab_pitch + x] = v > a.high ? kStrong : v > a.low ? kWeak : 0;   // NaN: 0
        }
}

__global__ __launch_bounds__(256) void k_hyst_propagate(const HystArgs a, unsigned* changed)
{
    __shared__ unsigned char t[kHystTileH + 2][kHystTileW + 2];
    unsigned char* lab = a.lab + (size_t)blockIdx.z * a.lab_stride;
    const int nty = tile_row_count(a.rows, kHystTileH);   // tile_grid deals the tile rows over at most kGridMaxYZ workgroup rows
    for (int by = blockIdx.y; by < nty; by += gridDim.y) {
        if (by != (int)blockIdx.y) __syncthreads();   // the previous tile is written back before t is loaded again
        const int x0 = blockIdx.x * kHystTileW, y0 = by * kHystTileH;
        for (int i = threadIdx.x; i < (kHystTileH + 2) * (kHystTileW + 2); i += blockDim.x) {
            const int ty = i / (kHystTileW + 2), tx = i % (kHystTileW + 2);
            const int y = y0 + ty - 1, x = x0 + tx - 1;
            t[ty][tx] = (y >= 0 && y < a.rows && x >= 0 && x < a.cols) ? lab[(size_t)y * a.lab_pitch + x] : 0;
        }
        __syncthreads();
        // lane -> one segment of one tile row, swept left to right and back, promoting in place: a run along the row is linked in one sweep
        const int ty = 1 + threadIdx.x / 8, tx0 = 1 + (threadIdx.x % 8) * kHystSeg;
        int any = 0;
        for (;;) {
            int ch = 0;
            for (int dir = 0; dir < 2; ++dir)
                for (int j = 0; j < kHystSeg; ++j) {
                    const int tx = dir ? tx0 + kHystSeg - 1 - j : tx0 + j;
                    if (t[ty][tx] != kWeak) continue;
                    const bool hit = t[ty - 1][tx - 1] == kStrong || t[ty - 1][tx] == kStrong || t[ty - 1][tx + 1] == kStrong ||
                                     t[ty][tx - 1] == kStrong || t[ty][tx + 1] == kStrong || t[ty + 1][tx - 1] == kStrong ||
                                     t[ty + 1][tx] == kStrong || t[ty + 1][tx + 1] == kStrong;
                    if (hit) {
                        t[ty][tx] = kStrong;
                        ch = 1;
                    }
                }
            any |= ch;
            if (!__syncthreads_or(ch)) break;
        }
        if (!__syncthreads_or(any)) continue;   // nothing promoted: nothing to write, no flag
        for (int i = threadIdx.x; i < kHystTileH * kHystTileW; i += blockDim.x) {
            const int ty2 = i / kHystTileW, tx2 = i % kHystTileW;
            const int y = y0 + ty2, x = x0 + tx2;
            if (y < a.rows && x < a.cols) lab[(size_t)y * a.lab_pitch + x] = t[ty2 + 1][tx2 + 1];
        }
        if (threadIdx.x == 0) atomicAdd(changed, 1u);
    }
}

__global__ void k_hyst_flag_reset(unsigned* changed) { *changed = 0u; }

__global__ __launch_bounds__(256) void k_hyst_emit(const HystArgs a)
{
    const int z = blockIdx.z;
    const unsigned char* lab = a.lab + (size_t)z * a.lab_stride;
    for (int r = blockIdx.y; r < a.rows; r += gridDim.y)
        for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < a.cols; x += gridDim.x * blockDim.x) {
            const bool keep = lab[(size_t)r * a.lab_pitch + x] == kStrong;
            if (a.out_u8) a.out8[z][(size_t)r * a.out_pitch[z] + x] = keep ? 255 : 0;
            else a.out32[z][(size_t)r * a.out_pitch[z] + x] = keep ? 255.0f : 0.0f;
        }
}

static dim3 hyst_point_grid(const HystArgs& a)
{
    int gx = (a.cols + 255) / 256;
    if (gx > 64) gx = 64;
    int gy = a.rows;
    if ((long)gx * gy > 4096) gy = 4096 / gx > 0 ? 4096 / gx : 1;
    return dim3(gx, gy, a.n);
}

static bool hyst_ok(const HystArgs& a)
{
    if (a.rows <= 0 || a.cols <= 0 || a.n < 1 || a.n > kHystMax || !a.lab) return false;
    for (int z = 0; z < a.n; ++z)
        if (!a.in[z].p) return false;
    return true;
}

hipError_t launch_hyst_classify(const HystArgs& a, hipStream_t s)
{
    if (!hyst_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_hyst_classify, hyst_point_grid(a), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_hyst_flag_reset(unsigned* changed, hipStream_t s)
{
    if (!changed) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_hyst_flag_reset, dim3(1), dim3(1), 0, s, changed);
    return hipGetLastError();
}

hipError_t launch_hyst_pass(const HystArgs& a, unsigned* changed, hipStream_t s)
{
    if (!hyst_ok(a) || !changed) return hipErrorInvalidValue;
    const GridDims gd = tile_grid(a.rows, a.cols, kHystTileW, kHystTileH, a.n);
    hipLaunchKernelGGL(k_hyst_propagate, dim3(gd.x, gd.y, gd.z), dim3(256), 0, s, a, changed);
    return hipGetLastError();
}

hipError_t launch_hyst_emit(const HystArgs& a, hipStream_t s)
{
    if (!hyst_ok(a)) return hipErrorInvalidValue;
    for (int z = 0; z < a.n; ++z)
        if (a.out_u8 ? !a.out8[z] : !a.out32[z]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_hyst_emit, hyst_point_grid(a), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace cvs
