// cvs_kernels_link.hip -- the one-pass link (extension beyond the reference): hysteresis and prune as ONE union-find labelling over any
// number of planes, for gfx950.  cvs_link keeps the 8-connected components of { v > low } whose largest value is > high and >= min_peak
// and whose area is >= min_area -- byte for byte what cvs_hysteresis followed by cvs_contour_prune writes, because the mask hysteresis
// keeps is exactly the set of such components that hold a strong pixel.
//
// Four launches per chain of planes, whatever the planes hold: tiles, borders, statistics at the roots, emit.  blockIdx.z (blockIdx.y in
// the border launch) is the plane.  The parent plane, the tile labelling, the border merge and the carried root of the statistics are those
// of cvs_kernels_components.hip (cvs_cc_device.h holds what the two files share); what differs: the foreground test is fused into the tile
// kernel, there is no root plane (the statistics and the emit walk the final parent plane themselves: 12 bytes of scratch per pixel), and
// nothing is read back.  Integer arithmetic and float comparisons only: every result is a function of the inputs alone.
#include <hip/hip_runtime.h>

#include "cvs_cc_device.h"
#include "cvs_link.h"

namespace cvs {

constexpr int kLW = kCcTileW, kLH = kCcTileH;
static_assert(kLW == 128 && kLH == 32, "k_link_tiles: 256 lanes, two tile rows of 128 columns per step, 16 steps");

__device__ __forceinline__ LinkDesc link_plane(const LinkArgs& a, int z)
{
    if (a.tab) return a.tab[z];
    LinkDesc d = a.first;
    d.in += (long long)z * a.in_stride;
    d.out = static_cast<char*>(d.out) + (long long)z * a.out_stride;
    return d;
}

// the descriptors of planes that lie at no constant stride: from the kernel arguments into the device table (a kernel, not a copy from
// host memory: the launch is complete when it is queued, captured or not)
__global__ __launch_bounds__(64) void k_link_table(const LinkTableArgs t, LinkDesc* tab)
{
    const int k = threadIdx.x;
    if (k < t.count) tab[t.first + k] = t.d[k];
}

// ---------------------------------------------------------------------------------------
// Step 1, k_link_tiles: k_cc_tiles with the foreground test v > low (NaN: background) read from the f32 plane itself.  One workgroup per
// 128 x 32 tile and plane; the ballot of the foreground bits gives every pixel the head of its horizontal run, run heads union with the
// row above in LDS, then every pixel stores the GLOBAL index (inside its plane) of its tile-local root.  Area and peak are cleared on the way.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_link_tiles(const LinkArgs a)
{
    __shared__ int L[kLH * kLW];
    const int z = blockIdx.z;
    const LinkDesc d = link_plane(a, z);
    const int rows = a.rows, cols = a.cols;
    if (a.kept && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) a.kept[z] = 0;
    const int nty = tile_row_count(rows, kLH);   // tile_grid deals the tile rows over at most kGridMaxYZ workgroup rows
    for (int by = blockIdx.y; by < nty; by += gridDim.y) {
        if (by != (int)blockIdx.y) __syncthreads();   // the previous tile's lookups are done before L is written again
        const int x0 = blockIdx.x * kLW, y0 = by * kLH;
        const int tx = threadIdx.x & (kLW - 1), half = threadIdx.x >> 7, lane = threadIdx.x & 63;
        const int x = x0 + tx;
        unsigned fgbits = 0;
#pragma unroll
        for (int k = 0; k < kLH / 2; ++k) {
            const int ty = 2 * k + half, y = y0 + ty;
            const bool fg = y < rows && x < cols && d.in[(size_t)y * d.in_pitch + x] > a.low;
            const unsigned long long gaps = ~__ballot(fg) & ((1ull << lane) - 1ull);   // background lanes left of this one
            const int start = gaps ? 64 - __clzll((long long)gaps) : 0;                 // first lane of this pixel's run
            const int i = ty * kLW + tx;
            L[i] = fg ? i - lane + start : -1;
            fgbits |= (fg ? 1u : 0u) << k;
        }
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < kLH / 2; ++k) {
            if (!((fgbits >> k) & 1u)) continue;
            const int ty = 2 * k + half, i = ty * kLW + tx;
            const bool up = ty > 0;
            const bool n = up && lds_get(L, i - kLW) >= 0;
            const bool nw = up && tx > 0 && lds_get(L, i - kLW - 1) >= 0;
            const bool ne = up && tx < kLW - 1 && lds_get(L, i - kLW + 1) >= 0;
            const bool in_run = lane > 0 && lds_get(L, i - 1) >= 0;   // the left neighbour is in this pixel's run (same initial parent)
            if (!in_run) {
                if (tx == 64 && lds_get(L, i - 1) >= 0) lds_union(L, i, i - 1);   // the run goes on in the other wave's half of the row
                if (n) {
                    lds_union(L, i, i - kLW);   // (nw and ne touch n in their own row)
                } else {
                    if (nw) lds_union(L, i, i - kLW - 1);
                    if (ne) lds_union(L, i, i - kLW + 1);
                }
            } else if (!n && ne) {
                lds_union(L, i, i - kLW + 1);   // every other contact of a pixel inside a run is made by its left neighbour
            }
        }
        __syncthreads();
        const size_t base = (size_t)z * a.plane_stride;
#pragma unroll 1
        for (int k = 0; k < kLH / 2; ++k) {
            const int ty = 2 * k + half, y = y0 + ty;
            if (y >= rows || x >= cols) continue;
            int v = -1;
            if ((fgbits >> k) & 1u) {
                const int r = lds_find(L, ty * kLW + tx);
                v = (y0 + r / kLW) * cols + x0 + r % kLW;
            }
            const size_t g = base + (size_t)y * cols + x;
            a.parent[g] = v;
            a.area[g] = 0;
            a.peak[g] = 0u;
        }
    }
}

// ---------------------------------------------------------------------------------------
// Step 2, k_link_borders: k_cc_borders per plane (blockIdx.y).  One lane per pixel of a tile's top row and of a tile's left column, unions
// with the neighbours across the border.  Other workgroups of the launch change the words this one reads: EVERY access to the parent
// plane is an agent-scope atomic, and the kernel touches nothing else.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_link_borders(int rows, int cols, int32_t* parent0, size_t plane_stride)
{
    int32_t* parent = parent0 + (size_t)blockIdx.y * plane_stride;
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    const int nty = tile_row_count(rows, kLH), ntx = tile_row_count(cols, kLW);
    const long long n_top = (long long)(nty - 1) * cols, n_left = (long long)(ntx - 1) * rows;
    if (id < n_top) {   // (x, y) on the top row of tile row t >= 1: the three neighbours in row y - 1
        const int x = (int)(id % cols), y = (int)(id / cols + 1) * kLH;
        const int self = y * cols + x;
        if (g_get(parent, self) < 0) return;
        const int up = self - cols;
        const bool n = g_get(parent, up) >= 0;
        const bool nw = x > 0 && g_get(parent, up - 1) >= 0;
        const bool ne = x < cols - 1 && g_get(parent, up + 1) >= 0;
        if (n) g_union(parent, self, up);
        // with n set, nw / ne are its row neighbours -- already one component with it unless they lie in another tile
        if (nw && (!n || x % kLW == 0)) g_union(parent, self, up - 1);
        if (ne && (!n || x % kLW == kLW - 1)) g_union(parent, self, up + 1);
    } else if (id < n_top + n_left) {   // (x, y) on the left column of tile column t >= 1: the three neighbours in column x - 1
        const long long j = id - n_top;
        const int y = (int)(j % rows), x = (int)(j / rows + 1) * kLW;
        const int self = y * cols + x;
        if (g_get(parent, self) < 0) return;
        const int left = self - 1;
        const bool w = g_get(parent, left) >= 0;
        const bool nw = y > 0 && g_get(parent, left - cols) >= 0;
        const bool sw = y < rows - 1 && g_get(parent, left + cols) >= 0;
        if (w) g_union(parent, self, left);
        if (nw && (!w || y % kLH == 0)) g_union(parent, self, left - cols);
        if (sw && (!w || y % kLH == kLH - 1)) g_union(parent, self, left + cols);
    }
}

// ---------------------------------------------------------------------------------------
// Step 3, k_link_stats: k_prune_stats on the roots the lanes find themselves; the weight is the input plane, and every foreground pixel has
// one (v > low: never NaN).  One lane per pixel, a wave covers 64 consecutive pixels of a row and walks down the rows of its strip; runs of
// one root are reduced in the wave, and ONE root per wave is carried in registers across the rows: the component that spans the image
// -- a low `low` percolates -- takes one atomic per wave instead of one per run on the same word.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_link_stats(const LinkArgs a)
{
    const int z = blockIdx.z;
    const LinkDesc d = link_plane(a, z);
    const int rows = a.rows, cols = a.cols;
    const size_t base = (size_t)z * a.plane_stride;
    const int32_t* parent = a.parent + base;
    int32_t* area = a.area + base;
    uint32_t* peak = a.peak + base;
    const int lane = threadIdx.x & 63;
    const int x = blockIdx.x * 256 + threadIdx.x;
    int c_root = -1, c_area = 0;
    unsigned c_key = 0u;
    for (int y = blockIdx.y; y < rows; y += gridDim.y) {
        int r = -1;
        unsigned key = 0u;
        if (x < cols) {
            const int p = parent[(size_t)y * cols + x];
            if (p >= 0) {
                r = root_of(parent, p);
                key = ordered_bits(d.in[(size_t)y * d.in_pitch + x]);
            }
        }
        bool head;
        int end;
        run_of(r, lane, head, end);
#pragma unroll
        for (int s = 1; s < 64; s *= 2) {
            const unsigned o = __shfl_down(key, s, 64);
            if (lane + s < end && o > key) key = o;
        }
        const bool h = head && r >= 0;
        const unsigned long long hm = __ballot(h);
        if (!hm) continue;   // (wave-uniform)
        // the carried root if a run of this row has it, else the root of the row's first run
        const int pick = __ballot(h && r == c_root) ? c_root : __shfl(r, __ffsll((long long)hm) - 1, 64);
        if (pick != c_root) {
            if (lane == 0 && c_root >= 0) {
                atomicAdd(&area[c_root], c_area);
                atomicMax(&peak[c_root], c_key);
            }
            c_root = pick;
            c_area = 0;
            c_key = 0u;
        }
        const bool mine = h && r == pick;
        int s = mine ? end - lane : 0;
        unsigned k = mine ? key : 0u;
#pragma unroll
        for (int t = 32; t > 0; t >>= 1) {
            s += __shfl_xor(s, t, 64);
            const unsigned o = __shfl_xor(k, t, 64);
            k = o > k ? o : k;
        }
        c_area += s;
        c_key = k > c_key ? k : c_key;
        if (h && !mine) {
            atomicAdd(&area[r], end - lane);
            atomicMax(&peak[r], key);
        }
    }
    if (lane == 0 && c_root >= 0) {
        atomicAdd(&area[c_root], c_area);
        atomicMax(&peak[c_root], c_key);
    }
}

// ---------------------------------------------------------------------------------------
// Step 4, k_link_emit: one lane per pixel looks the verdict of its root up -- the three tests of the contract, IEEE comparisons on the
// value the ordered bits stand for -- and writes 255 / 0; the root pixel of a kept component counts it.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_link_emit(const LinkArgs a)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= a.cols) return;
    const int z = blockIdx.z;
    const LinkDesc d = link_plane(a, z);
    const size_t base = (size_t)z * a.plane_stride;
    const int32_t* parent = a.parent + base;
    for (int y = blockIdx.y; y < a.rows; y += gridDim.y) {
        const int i = y * a.cols + x;
        const int p = parent[i];
        bool keep = false;
        int r = -1;
        if (p >= 0) {
            r = root_of(parent, p);
            const float top = ordered_value(a.peak[base + r]);
            keep = top > a.high && a.area[base + r] >= a.min_area && top >= a.min_peak;
        }
        if (a.out_u8) static_cast<unsigned char*>(d.out)[(size_t)y * d.out_pitch + x] = keep ? 255 : 0;
        else static_cast<float*>(d.out)[(size_t)y * d.out_pitch + x] = keep ? 255.0f : 0.0f;
        if (a.kept && keep && r == i) atomicAdd(&a.kept[z], 1);   // one per component: at its root
    }
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
static bool link_ok(const LinkArgs& a)
{
    if (a.rows <= 0 || a.cols <= 0 || (long long)a.rows * a.cols > 0x7fffffffLL - 1) return false;
    if (a.n < 1 || a.n > kLinkChainMax || !a.parent || !a.area || !a.peak) return false;
    if (a.plane_stride < (size_t)a.rows * a.cols) return false;
    return a.tab || (a.first.in && a.first.out);
}

// 256 columns per workgroup; the rows of a plane dealt over enough workgroups to fill the card once all planes are counted, and few
// enough that a wave walks many rows with its carried root
static dim3 link_row_grid(const LinkArgs& a)
{
    const int gx = (a.cols + 255) / 256;
    int per_plane = 4096 / a.n;
    per_plane = per_plane < 256 ? 256 : per_plane;
    int gy = per_plane / gx;
    gy = gy < 1 ? 1 : gy;
    return dim3(gx, a.rows < gy ? a.rows : gy, a.n);
}

hipError_t launch_link_table(const LinkTableArgs& t, LinkDesc* tab, hipStream_t s)
{
    if (!tab || t.first < 0 || t.count < 1 || t.count > kLinkTableBatch) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_link_table, dim3(1), dim3(64), 0, s, t, tab);
    return hipGetLastError();
}

hipError_t launch_link_tiles(const LinkArgs& a, hipStream_t s)
{
    if (!link_ok(a)) return hipErrorInvalidValue;
    const GridDims gd = tile_grid(a.rows, a.cols, kLW, kLH, a.n);
    hipLaunchKernelGGL(k_link_tiles, dim3(gd.x, gd.y, gd.z), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_link_borders(const LinkArgs& a, hipStream_t s)
{
    if (!link_ok(a)) return hipErrorInvalidValue;
    const long long nty = tile_row_count(a.rows, kLH), ntx = tile_row_count(a.cols, kLW);
    const long long lanes = (nty - 1) * a.cols + (ntx - 1) * a.rows;
    const long long blocks = lanes > 0 ? (lanes + 255) / 256 : 1;   // (a single tile: one workgroup that finds nothing to do)
    hipLaunchKernelGGL(k_link_borders, dim3((unsigned)blocks, a.n), dim3(256), 0, s, a.rows, a.cols, a.parent, a.plane_stride);
    return hipGetLastError();
}

hipError_t launch_link_stats(const LinkArgs& a, hipStream_t s)
{
    if (!link_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_link_stats, link_row_grid(a), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_link_emit(const LinkArgs& a, hipStream_t s)
{
    if (!link_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_link_emit, link_row_grid(a), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace cvs
