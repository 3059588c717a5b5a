// cvs_kernels_components.hip -- contour components (extension beyond the reference): 8-connected component labelling of a device-resident
// mask by union-find, and what is built on it -- dense labels in raster order (cvs_label), per-component statistics
// (cvs_component_stats), pruning of short / faint components (cvs_contour_prune) and raster-ordered point lists (cvs_contour_points),
// for gfx950.
//
// Unlike the hysteresis passes of cvs_kernels_contour.hip, nothing here depends on the shape of a contour: every entry point is a fixed
// sequence of launches for a given image size.  All arithmetic is integer (or a copy), every result is reproducible bit for bit.
//
// The PARENT plane (cvs_components.h): -1 = background, else the linear index of a pixel of the same component, never larger than the
// pixel's own; roots point at themselves.  Parents only ever decrease, so every find loop ends, and the root of a finished component
// is its smallest linear index -- its first pixel in raster order -- whatever the order in which the unions happened.
#include <hip/hip_runtime.h>

#include "cvs_cc_device.h"
#include "cvs_components.h"

namespace cvs {

constexpr int kTW = kCcTileW, kTH = kCcTileH;
static_assert(kTW == 128 && kTH == 32, "k_cc_tiles: 256 lanes, two tile rows of 128 columns per step, 16 steps");

__device__ __forceinline__ bool mask_fg(const MaskRef& m, int y, int x)
{
    if (m.u8) return static_cast<const unsigned char*>(m.p)[(size_t)y * m.pitch + x] != 0;
    return static_cast<const float*>(m.p)[(size_t)y * m.pitch + x] > 0.0f;   // NaN, zeros, negatives: background
}

// ---------------------------------------------------------------------------------------
// Step 1, k_cc_tiles: one workgroup per 128 x 32 tile, union-find in LDS on tile-local indices.  Lane -> one pixel of two tile rows per
// step (coalesced), 16 steps.  A wave covers 64 consecutive pixels of a row: the ballot of the foreground bits gives every pixel the
// start of its horizontal run at once, so only run heads (and pixels whose upper-right neighbour starts a new contact) need a union
// with the row above.  After the barrier every pixel follows its parents to the tile-local root and stores that root's GLOBAL linear
// index (plain stores; the launch boundary publishes them).
// ---------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_cc_tiles(const MaskRef mask, int rows, int cols, int32_t* parent, int32_t* zero_a, uint32_t* zero_b)
{
    __shared__ int L[kTH * kTW];
    const int nty = tile_row_count(rows, kTH);   // tile_grid deals the tile rows over at most kGridMaxYZ workgroup rows
    for (int by = blockIdx.y; by < nty; by += gridDim.y) {
        if (by != (int)blockIdx.y) __syncthreads();   // the previous tile's lookups are done before L is written again
        const int x0 = blockIdx.x * kTW, y0 = by * kTH;
        const int tx = threadIdx.x & (kTW - 1), half = threadIdx.x >> 7, lane = threadIdx.x & 63;
        const int x = x0 + tx;
        unsigned fgbits = 0;
#pragma unroll
        for (int k = 0; k < kTH / 2; ++k) {
            const int ty = 2 * k + half, y = y0 + ty;
            const bool fg = y < rows && x < cols && mask_fg(mask, y, x);
            const unsigned long long gaps = ~__ballot(fg) & ((1ull << lane) - 1ull);   // background lanes left of this one
            const int start = gaps ? 64 - __clzll((long long)gaps) : 0;                 // first lane of this pixel's run
            const int i = ty * kTW + tx;
            L[i] = fg ? i - lane + start : -1;
            fgbits |= (fg ? 1u : 0u) << k;
        }
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < kTH / 2; ++k) {
            if (!((fgbits >> k) & 1u)) continue;
            const int ty = 2 * k + half, i = ty * kTW + tx;
            const bool up = ty > 0;
            const bool n = up && lds_get(L, i - kTW) >= 0;
            const bool nw = up && tx > 0 && lds_get(L, i - kTW - 1) >= 0;
            const bool ne = up && tx < kTW - 1 && lds_get(L, i - kTW + 1) >= 0;
            const bool in_run = lane > 0 && lds_get(L, i - 1) >= 0;   // the left neighbour is in this pixel's run (same initial parent)
            if (!in_run) {
                if (tx == 64 && lds_get(L, i - 1) >= 0) lds_union(L, i, i - 1);   // the run goes on in the other wave's half of the row
                if (n) {
                    lds_union(L, i, i - kTW);   // (nw and ne touch n in their own row)
                } else {
                    if (nw) lds_union(L, i, i - kTW - 1);
                    if (ne) lds_union(L, i, i - kTW + 1);
                }
            } else if (!n && ne) {
                lds_union(L, i, i - kTW + 1);   // every other contact of a pixel inside a run is made by its left neighbour
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < kTH / 2; ++k) {
            const int ty = 2 * k + half, y = y0 + ty;
            if (y >= rows || x >= cols) continue;
            int v = -1;
            if ((fgbits >> k) & 1u) {
                const int r = lds_find(L, ty * kTW + tx);
                v = (y0 + r / kTW) * cols + x0 + r % kTW;
            }
            const size_t g = (size_t)y * cols + x;
            parent[g] = v;
            if (zero_a) zero_a[g] = 0;
            if (zero_b) zero_b[g] = 0u;
        }
    }
}

// ---------------------------------------------------------------------------------------
// Step 2, k_cc_borders: one lane per pixel of a tile's top row (all tile rows but the first) and of a tile's left column (all tile
// columns but the first), unions with the neighbours on the other side of the border -- the corner diagonals included.  Other workgroups
// of the same launch change the words this one reads, and the card has eight L2s: EVERY access to the parent plane here is an agent-scope
// atomic (loads bypass the CU's L1 and are served where the atomics are done).  The kernel reads nothing else -- background is the -1 of
// step 1.
// ---------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_cc_borders(int rows, int cols, int32_t* parent)
{
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    const int nty = tile_row_count(rows, kTH), ntx = tile_row_count(cols, kTW);
    const long long n_top = (long long)(nty - 1) * cols, n_left = (long long)(ntx - 1) * rows;
    if (id < n_top) {   // (x, y) on the top row of tile row t >= 1: the three neighbours in row y - 1
        const int x = (int)(id % cols), y = (int)(id / cols + 1) * kTH;
        const int self = y * cols + x;
        if (g_get(parent, self) < 0) return;
        const int up = self - cols;
        const bool n = g_get(parent, up) >= 0;
        const bool nw = x > 0 && g_get(parent, up - 1) >= 0;
        const bool ne = x < cols - 1 && g_get(parent, up + 1) >= 0;
        if (n) g_union(parent, self, up);
        // with n set, nw / ne are its row neighbours -- already one component with it unless they lie in another tile
        if (nw && (!n || x % kTW == 0)) g_union(parent, self, up - 1);
        if (ne && (!n || x % kTW == kTW - 1)) g_union(parent, self, up + 1);
    } else if (id < n_top + n_left) {   // (x, y) on the left column of tile column t >= 1: the three neighbours in column x - 1
        const long long j = id - n_top;
        const int y = (int)(j % rows), x = (int)(j / rows + 1) * kTW;
        const int self = y * cols + x;
        if (g_get(parent, self) < 0) return;
        const int left = self - 1;
        const bool w = g_get(parent, left) >= 0;
        const bool nw = y > 0 && g_get(parent, left - cols) >= 0;
        const bool sw = y < rows - 1 && g_get(parent, left + cols) >= 0;
        if (w) g_union(parent, self, left);
        if (nw && (!w || y % kTH == 0)) g_union(parent, self, left - cols);
        if (sw && (!w || y % kTH == kTH - 1)) g_union(parent, self, left + cols);
    }
}

// ---------------------------------------------------------------------------------------
// Step 3: the parent plane is final and read-only from here on (plain loads behind the launch boundary).
// ---------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_cc_flatten(int n, const int32_t* parent, int32_t* root)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int p = parent[i];
        root[i] = p < 0 ? -1 : root_of(parent, p);
    }
}

__global__ __launch_bounds__(256) void k_cc_relabel(int rows, int cols, const int32_t* parent, const int32_t* rank, const IntPlane labels)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= cols) return;
    for (int y = blockIdx.y; y < rows; y += gridDim.y) {
        const int p = parent[(size_t)y * cols + x];
        labels.p[(size_t)y * labels.pitch + x] = p < 0 ? 0 : rank[root_of(parent, p)] + 1;
    }
}

// ---------------------------------------------------------------------------------------
// Exclusive scan of a per-pixel flag in raster order: k_scan_count (flagged pixels per workgroup of 4096), k_scan_partials (one workgroup
// scans those counts in place), k_scan_apply (the workgroup's own scan from ballots, plus its offset).  Element j * 256 + lane of a
// workgroup's range is lane's j-th pixel, so loads are coalesced and the order inside the range is (step, wave, lane).
// ---------------------------------------------------------------------------------------
template <int KIND>
__device__ __forceinline__ bool scan_flag(const IntPlane& v, int cols, long long i, long long n, int& x, int& y, int& val)
{
    if (i >= n) return false;
    if (KIND == kScanRoots) {
        val = v.p[i];
        return val == (int)i;
    }
    y = (int)(i / cols);
    x = (int)(i - (long long)y * cols);
    val = v.p[(size_t)y * v.pitch + x];
    return val != 0;
}

template <int KIND>
__global__ __launch_bounds__(256) void k_scan_count(const IntPlane v, int rows, int cols, int32_t* partials)
{
    __shared__ int ws[4];
    const long long n = (long long)rows * cols, base = (long long)blockIdx.x * kCcScanBlock;
    int c = 0;
#pragma unroll 4
    for (int j = 0; j < kCcScanBlock / 256; ++j) {
        int x, y, val;
        c += __popcll(__ballot(scan_flag<KIND>(v, cols, base + j * 256 + threadIdx.x, n, x, y, val)));
    }
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;   // (every lane of a wave holds the wave's count)
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

__global__ __launch_bounds__(1024) void k_scan_partials(int32_t* p, int blocks)
{
    __shared__ int ws[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < blocks; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < blocks ? p[i] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d *= 2) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) ws[wave] = incl;
        __syncthreads();
        int pre = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int t = ws[w];
            pre += w < wave ? t : 0;
            tot += t;
        }
        if (i < blocks) p[i] = carry + pre + incl - v;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) p[blocks] = carry;
}

template <int KIND>
__global__ __launch_bounds__(256) void k_scan_apply(const IntPlane v, int rows, int cols, const int32_t* partials, int32_t* out)
{
    constexpr int kSteps = kCcScanBlock / 256;
    __shared__ int cnt[kSteps * 4];
    const long long n = (long long)rows * cols, base = (long long)blockIdx.x * kCcScanBlock;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned flags = 0;
    unsigned long long pre_lo = 0, pre_hi = 0;   // the lane's rank inside its wave at each step, one byte per step (8 steps per word)
#pragma unroll
    for (int j = 0; j < kSteps; ++j) {
        int x, y, val;
        const bool f = scan_flag<KIND>(v, cols, base + j * 256 + threadIdx.x, n, x, y, val);
        const unsigned long long b = __ballot(f);
        const unsigned long long pre = (unsigned long long)__popcll(b & ((1ull << lane) - 1ull));
        if (j < 8) pre_lo |= pre << (8 * j);
        else pre_hi |= pre << (8 * (j - 8));
        flags |= (f ? 1u : 0u) << j;
        if (lane == 0) cnt[j * 4 + wave] = __popcll(b);
    }
    __syncthreads();
    if (wave == 0) {   // 64 counts in (step, wave) order -> their exclusive scan, in place
        const int c = cnt[lane];
        int incl = c;
#pragma unroll
        for (int d = 1; d < 64; d *= 2) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        cnt[lane] = incl - c;
    }
    __syncthreads();
    const int off = partials[blockIdx.x];
#pragma unroll
    for (int j = 0; j < kSteps; ++j) {
        if (!((flags >> j) & 1u)) continue;
        const int pre = (int)(((j < 8 ? pre_lo >> (8 * j) : pre_hi >> (8 * (j - 8)))) & 0xffull);
        const int rank = off + cnt[j * 4 + wave] + pre;
        const long long i = base + j * 256 + threadIdx.x;
        if (KIND == kScanRoots) {
            out[i] = rank;
        } else {
            int x, y, val;
            (void)scan_flag<KIND>(v, cols, i, n, x, y, val);   // (the value again: an L2 hit, instead of 16 more registers)
            int32_t* t = out + 3 * (size_t)rank;
            t[0] = x;
            t[1] = y;
            t[2] = val;
        }
    }
}

// ---------------------------------------------------------------------------------------
// Statistics.  One lane per pixel, a wave covers 64 consecutive pixels of a row: lanes that share a label with their left neighbour form
// a run, the run's head issues the atomics for all of it (area += length, box from its two ends, the maximum of the peak keys from a
// segmented shuffle reduction).  Integer atomics only: no result depends on their order.
// ---------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_stats_init(CcAcc* acc, int count)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= count) return;
    CcAcc a;
    a.area = 0;
    a.x0 = 0x7fffffff;
    a.x1 = -1;
    a.y1 = -1;
    a.first = 0x7fffffff;
    a.pad = 0;
    a.key = 0ull;
    acc[k] = a;
}

template <bool W>
__global__ __launch_bounds__(256) void k_stats(const IntPlane labels, int rows, int cols, int count, const PlaneRef weight, CcAcc* acc)
{
    const int lane = threadIdx.x & 63;
    const int x = blockIdx.x * 256 + threadIdx.x;
    for (int y = blockIdx.y; y < rows; y += gridDim.y) {
        int l = x < cols ? labels.p[(size_t)y * labels.pitch + x] : 0;
        if (l < 1 || l > count) l = 0;   // labels outside 1 .. count are skipped: no write can leave the table
        unsigned long long key = 0ull;
        if (W && l) {
            const float f = weight.p[(size_t)y * weight.pitch + x];
            if (f == f) key = ((unsigned long long)ordered_bits(f) << 32) | (0xffffffffu - (unsigned)(y * cols + x));
        }
        bool head;
        int end;
        run_of(l, lane, head, end);
        if (W) {
#pragma unroll
            for (int d = 1; d < 64; d *= 2) {
                const unsigned long long o = __shfl_down(key, d, 64);
                if (lane + d < end && o > key) key = o;
            }
        }
        if (head && l) {
            CcAcc* a = acc + (l - 1);
            const int len = end - lane;
            atomicAdd(&a->area, len);
            atomicMin(&a->x0, x);
            atomicMax(&a->x1, x + len - 1);
            atomicMax(&a->y1, y);
            atomicMin(&a->first, y * cols + x);   // (its row is the top of the box)
            if (W && key) atomicMax(&a->key, key);
        }
    }
}

__global__ __launch_bounds__(256) void k_stats_table(const CcAcc* acc, int count, int cols, int32_t* table)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= count) return;
    const CcAcc a = acc[k];
    int32_t* t = table + 10 * (size_t)k;   // struct cvs_component: ten 4-byte fields
    const bool any = a.area > 0;
    t[0] = a.area;
    t[1] = any ? a.x0 : -1;
    t[2] = any ? a.first / cols : -1;
    t[3] = a.x1;
    t[4] = a.y1;
    t[5] = any ? a.first % cols : -1;
    t[6] = any ? a.first / cols : -1;
    const bool pk = a.key != 0ull;
    const int at = (int)(0xffffffffu - (unsigned)(a.key & 0xffffffffull));
    t[7] = pk ? at % cols : -1;
    t[8] = pk ? at / cols : -1;
    t[9] = pk ? (int32_t)__float_as_uint(ordered_value((unsigned)(a.key >> 32))) : (int32_t)0xff800000u;   // -INFINITY
}

// ---------------------------------------------------------------------------------------
// Prune: the same run aggregation, keyed by the root pixel of each component (no dense numbering, no table): area and the ordered bits of
// the peak in two planes that step 1 cleared; then one lane per pixel looks its root's verdict up.
// ---------------------------------------------------------------------------------------
template <bool W>
__global__ __launch_bounds__(256) void k_prune_stats(int rows, int cols, const int32_t* root, const PlaneRef weight, int32_t* area, uint32_t* peak)
{
    const int lane = threadIdx.x & 63;
    const int x = blockIdx.x * 256 + threadIdx.x;
    // One root per wave is carried in registers across the rows the wave visits (wave-uniform values): a component that spans much of
    // the image -- the percolating one of a dense mask -- would otherwise take one atomic per run on ONE word (measured: 45 ms at
    // 4096^2, density 0.45); carried, it takes one per wave.  Runs of every other root issue their own atomics as they come.
    int c_root = -1, c_area = 0;
    unsigned c_key = 0u;
    for (int y = blockIdx.y; y < rows; y += gridDim.y) {
        const int r = x < cols ? root[(size_t)y * cols + x] : -1;
        unsigned key = 0u;
        if (W && r >= 0) {
            const float f = weight.p[(size_t)y * weight.pitch + x];
            if (f == f) key = ordered_bits(f);
        }
        bool head;
        int end;
        run_of(r, lane, head, end);
        if (W) {
#pragma unroll
            for (int d = 1; d < 64; d *= 2) {
                const unsigned o = __shfl_down(key, d, 64);
                if (lane + d < end && o > key) key = o;
            }
        }
        const bool h = head && r >= 0;
        const unsigned long long hm = __ballot(h);
        if (!hm) continue;   // (wave-uniform)
        // the carried root if a run of this row has it, else the root of the row's first run
        const int pick = __ballot(h && r == c_root) ? c_root : __shfl(r, __ffsll((long long)hm) - 1, 64);
        if (pick != c_root) {
            if (lane == 0 && c_root >= 0) {
                atomicAdd(&area[c_root], c_area);
                if (W && c_key) atomicMax(&peak[c_root], c_key);
            }
            c_root = pick;
            c_area = 0;
            c_key = 0u;
        }
        const bool mine = h && r == pick;
        int s = mine ? end - lane : 0;
        unsigned k = mine ? key : 0u;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            s += __shfl_xor(s, d, 64);
            if (W) {
                const unsigned o = __shfl_xor(k, d, 64);
                k = o > k ? o : k;
            }
        }
        c_area += s;
        c_key = k > c_key ? k : c_key;
        if (h && !mine) {
            atomicAdd(&area[r], end - lane);
            if (W && key) atomicMax(&peak[r], key);
        }
    }
    if (lane == 0 && c_root >= 0) {
        atomicAdd(&area[c_root], c_area);
        if (W && c_key) atomicMax(&peak[c_root], c_key);
    }
}

__global__ __launch_bounds__(256) void k_prune_emit(const PruneEmit a)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= a.cols) return;
    for (int y = blockIdx.y; y < a.rows; y += gridDim.y) {
        const int i = y * a.cols + x;
        const int r = a.root[i];
        bool keep = false;
        if (r >= 0) {
            keep = a.area[r] >= a.min_area;
            if (a.peak) {
                const unsigned o = a.peak[r];
                keep = keep && (o ? ordered_value(o) : -__builtin_inff()) >= a.min_peak;
            }
        }
        if (a.out_u8) static_cast<unsigned char*>(a.out)[(size_t)y * a.out_pitch + x] = keep ? 255 : 0;
        else static_cast<float*>(a.out)[(size_t)y * a.out_pitch + x] = keep ? 255.0f : 0.0f;
        if (keep && r == i) atomicAdd(a.kept, 1);   // one per component: at its root
    }
}

__global__ __launch_bounds__(256) void k_zero_ints(int32_t* p, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0;
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
static bool size_ok(int rows, int cols) { return rows > 0 && cols > 0 && (long long)rows * cols <= 0x7fffffffLL - 1; }

static dim3 row_grid(int rows, int cols)   // 256 columns per workgroup, rows dealt over at most 4096 of them
{
    const int gx = (cols + 255) / 256;
    int gy = 4096 / gx;
    gy = gy < 1 ? 1 : gy;
    return dim3(gx, rows < gy ? rows : gy);
}

hipError_t launch_cc_tiles(const MaskRef& mask, int rows, int cols, int32_t* parent, int32_t* zero_a, uint32_t* zero_b, hipStream_t s)
{
    if (!size_ok(rows, cols) || !mask.p || !parent) return hipErrorInvalidValue;
    const GridDims gd = tile_grid(rows, cols, kTW, kTH, 1);
    hipLaunchKernelGGL(k_cc_tiles, dim3(gd.x, gd.y, gd.z), dim3(256), 0, s, mask, rows, cols, parent, zero_a, zero_b);
    return hipGetLastError();
}

hipError_t launch_cc_borders(int rows, int cols, int32_t* parent, hipStream_t s)
{
    if (!size_ok(rows, cols) || !parent) return hipErrorInvalidValue;
    const long long nty = tile_row_count(rows, kTH), ntx = tile_row_count(cols, kTW);
    const long long lanes = (nty - 1) * cols + (ntx - 1) * rows;
    const long long blocks = lanes > 0 ? (lanes + 255) / 256 : 1;   // (a single tile: one workgroup that finds nothing to do)
    hipLaunchKernelGGL(k_cc_borders, dim3((unsigned)blocks), dim3(256), 0, s, rows, cols, parent);
    return hipGetLastError();
}

hipError_t launch_cc_flatten(int rows, int cols, const int32_t* parent, int32_t* root, hipStream_t s)
{
    if (!size_ok(rows, cols) || !parent || !root) return hipErrorInvalidValue;
    const long long n = (long long)rows * cols;
    long long blocks = (n + 255) / 256;
    blocks = blocks > 65536 ? 65536 : blocks;
    hipLaunchKernelGGL(k_cc_flatten, dim3((unsigned)blocks), dim3(256), 0, s, (int)n, parent, root);
    return hipGetLastError();
}

hipError_t launch_cc_relabel(int rows, int cols, const int32_t* parent, const int32_t* rank, const IntPlane& labels, hipStream_t s)
{
    if (!size_ok(rows, cols) || !parent || !rank || !labels.p) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cc_relabel, row_grid(rows, cols), dim3(256), 0, s, rows, cols, parent, rank, labels);
    return hipGetLastError();
}

hipError_t launch_scan_count(int kind, const IntPlane& v, int rows, int cols, int32_t* partials, hipStream_t s)
{
    if (!size_ok(rows, cols) || !v.p || !partials) return hipErrorInvalidValue;
    const dim3 grid(scan_blocks(rows, cols));
    if (kind == kScanRoots) hipLaunchKernelGGL(k_scan_count<kScanRoots>, grid, dim3(256), 0, s, v, rows, cols, partials);
    else hipLaunchKernelGGL(k_scan_count<kScanNonZero>, grid, dim3(256), 0, s, v, rows, cols, partials);
    return hipGetLastError();
}

hipError_t launch_scan_partials(int32_t* partials, int blocks, hipStream_t s)
{
    if (!partials || blocks < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(1024), 0, s, partials, blocks);
    return hipGetLastError();
}

hipError_t launch_scan_apply(int kind, const IntPlane& v, int rows, int cols, const int32_t* partials, int32_t* out, hipStream_t s)
{
    if (!size_ok(rows, cols) || !v.p || !partials || !out) return hipErrorInvalidValue;
    const dim3 grid(scan_blocks(rows, cols));
    if (kind == kScanRoots) hipLaunchKernelGGL(k_scan_apply<kScanRoots>, grid, dim3(256), 0, s, v, rows, cols, partials, out);
    else hipLaunchKernelGGL(k_scan_apply<kScanNonZero>, grid, dim3(256), 0, s, v, rows, cols, partials, out);
    return hipGetLastError();
}

hipError_t launch_stats_init(CcAcc* acc, int count, hipStream_t s)
{
    if (!acc || count < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_stats_init, dim3((count + 255) / 256), dim3(256), 0, s, acc, count);
    return hipGetLastError();
}

hipError_t launch_stats(const IntPlane& labels, int rows, int cols, int count, const PlaneRef& weight, CcAcc* acc, hipStream_t s)
{
    if (!size_ok(rows, cols) || !labels.p || !acc || count < 1) return hipErrorInvalidValue;
    if (weight.p) hipLaunchKernelGGL(k_stats<true>, row_grid(rows, cols), dim3(256), 0, s, labels, rows, cols, count, weight, acc);
    else hipLaunchKernelGGL(k_stats<false>, row_grid(rows, cols), dim3(256), 0, s, labels, rows, cols, count, weight, acc);
    return hipGetLastError();
}

hipError_t launch_stats_table(const CcAcc* acc, int count, int cols, void* table, hipStream_t s)
{
    if (!acc || !table || count < 1 || cols < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_stats_table, dim3((count + 255) / 256), dim3(256), 0, s, acc, count, cols, static_cast<int32_t*>(table));
    return hipGetLastError();
}

hipError_t launch_prune_stats(int rows, int cols, const int32_t* root, const PlaneRef& weight, int32_t* area, uint32_t* peak, hipStream_t s)
{
    if (!size_ok(rows, cols) || !root || !area || (weight.p && !peak)) return hipErrorInvalidValue;
    if (weight.p) hipLaunchKernelGGL(k_prune_stats<true>, row_grid(rows, cols), dim3(256), 0, s, rows, cols, root, weight, area, peak);
    else hipLaunchKernelGGL(k_prune_stats<false>, row_grid(rows, cols), dim3(256), 0, s, rows, cols, root, weight, area, peak);
    return hipGetLastError();
}

hipError_t launch_prune_emit(const PruneEmit& a, hipStream_t s)
{
    if (!size_ok(a.rows, a.cols) || !a.root || !a.area || !a.out || !a.kept) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_prune_emit, row_grid(a.rows, a.cols), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_zero_ints(int32_t* p, int n, hipStream_t s)
{
    if (!p || n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_zero_ints, dim3((n + 255) / 256), dim3(256), 0, s, p, n);
    return hipGetLastError();
}

}  // namespace cvs
