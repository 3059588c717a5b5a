// cvs_kernels_chains_batch.hip -- contour chains and sub-pixel chain points on the batch axis (extension beyond the reference):
// cvs_contour_chains_batch and cvs_chain_refine_batch, for gfx950.
//
// The n planes of a call are stacked into one block of n * rows rows (cvs_chains_batch.h).  Only the kernels here know what a plane is:
//
//   k_chb_table     descriptors of planes that lie at no constant stride, from the kernel arguments into a device table
//   k_chb_links     k_ch_links per plane (blockIdx.z): rows outside the plane are background, so no link crosses a seam
//   k_chb_tiles, k_chb_borders   k_cc_tiles / k_cc_borders per plane: tiles counted from each plane's own row 0, STACKED indices in the
//                   stacked parent plane, no union across a seam
//   (cvs_kernels_chains.hip, as it is, on n * rows rows: nodes, roots, the arc scan, arcs, pointer jumping, heads, head count)
//   k_chb_head_apply, k_chb_emit   the twins of k_ch_head_apply / k_ch_emit: the plane of every chain, coordinates inside the plane
//   k_chb_ranges    first chain and first point of every plane, from the planes of neighbouring table entries
//   k_chain_refine_batch   k_chain_refine's body behind the lookup of the point's plane
//
// Arc ids ascend by (LIN(from), LIN(to)), so the chains come out plane after plane and inside a plane in the order of the single-image
// contract: nothing is sorted.  All chain arithmetic is integer, every output position comes from a scan, every store of a result is a
// plain vector store; the only atomics are the agent-scope ones of the border merge on the parent plane.
// Built with -ffp-contract=off: the refinement rounds every product and sum on its own, as cvs_kernels_refine.hip does.
#include <hip/hip_runtime.h>

#include "cvs_cc_device.h"
#include "cvs_chain_device.h"
#include "cvs_chains_batch.h"
#include "cvs_device_math.h"

namespace cvs {

constexpr int kBW = kCcTileW, kBH = kCcTileH;
constexpr int kChbRows = 32;   // rows one workgroup of k_chb_links walks down
static_assert(kBW == 128 && kBH == 32, "k_chb_tiles: 256 lanes, two tile rows of 128 columns per step, 16 steps");

__device__ __forceinline__ MaskRef plane_of(const PlaneSet& s, int z)
{
    if (s.tab) return s.tab[z];
    MaskRef m = s.first;
    m.p = static_cast<const char*>(m.p) + (long long)z * s.stride;
    return m;
}

// a kernel, not a copy from host memory: the launch is complete when it is queued, captured or not
__global__ __launch_bounds__(64) void k_chb_table(const ChbTableArgs t, MaskRef* tab)
{
    const int k = threadIdx.x;
    if (k < t.count) tab[t.first + k] = t.d[k];
}

__device__ __forceinline__ bool chb_fg(const MaskRef& m, int rows, int cols, int y, int x)
{
    if (y < 0 || y >= rows || x < 0 || x >= cols) return false;
    if (m.u8) return static_cast<const unsigned char*>(m.p)[(size_t)y * m.pitch + x] != 0;
    return static_cast<const float*>(m.p)[(size_t)y * m.pitch + x] > 0.0f;   // NaN, zeros, negatives: background
}

// ---------------------------------------------------------------------------------------
// Step 1.  k_ch_links with blockIdx.z = plane: one lane per column, a workgroup walks 32 rows down; y counts from the plane's own row 0, and
// a row outside [0, rows) of THAT plane is background -- the last row of plane z never sees row 0 of plane z + 1.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_chb_links(const ChbArgs a)
{
    const int z = a.z0 + blockIdx.z, rows = a.rows, cols = a.cols;
    const MaskRef mask = plane_of(a.masks, z);
    uint16_t* link = a.link + (size_t)z * rows * cols;
    const int lane = threadIdx.x & 63;
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int xe = lane == 0 ? x - 1 : (lane == 63 ? x + 1 : -1);
    const int bands = tile_row_count(rows, kChbRows);   // tile_grid deals the 32-row bands over at most kGridMaxYZ workgroup rows
    for (int by = blockIdx.y; by < bands; by += gridDim.y) {
        const int y0 = by * kChbRows, y1 = y0 + kChbRows < rows ? y0 + kChbRows : rows;
        // bit 0: row y - 1, bit 1: row y, bit 2: row y + 1 (after the shift at the top of the loop)
        unsigned own = (chb_fg(mask, rows, cols, y0 - 1, x) ? 2u : 0u) | (chb_fg(mask, rows, cols, y0, x) ? 4u : 0u);
        unsigned ext = (chb_fg(mask, rows, cols, y0 - 1, xe) ? 2u : 0u) | (chb_fg(mask, rows, cols, y0, xe) ? 4u : 0u);
        for (int y = y0; y < y1; ++y) {
            own = (own >> 1) | (chb_fg(mask, rows, cols, y + 1, x) ? 4u : 0u);
            ext = (ext >> 1) | (chb_fg(mask, rows, cols, y + 1, xe) ? 4u : 0u);
            unsigned l = __shfl_up(own, 1, 64), r = __shfl_down(own, 1, 64);
            if (lane == 0) l = ext;
            if (lane == 63) r = ext;
            if (x >= cols) continue;
            unsigned v = 0;
            if (own & 2u) {
                const unsigned n = own & 1u, s = (own >> 2) & 1u, w = (l >> 1) & 1u, e = (r >> 1) & 1u;
                const unsigned nw = l & 1u & ~(n | w), ne = r & 1u & ~(n | e), sw = (l >> 2) & 1u & ~(s | w), se = (r >> 2) & 1u & ~(s | e);
                v = nw | (n << 1) | (ne << 2) | (w << 3) | (e << 4) | (sw << 5) | (s << 6) | (se << 7);
                v |= kChFg | (__popc(v) != 2 ? kChNode : 0u);
            }
            link[(size_t)y * cols + x] = (uint16_t)v;
        }
    }
}

// ---------------------------------------------------------------------------------------
// Step 2.  k_cc_tiles per plane: one workgroup per 128 x 32 tile of ONE plane (1080 is no multiple of 32: tiles of the stacked block would
// straddle two frames), union-find in LDS on tile-local indices, then every pixel stores the STACKED index of its tile-local root.  The aux
// plane (node flags, later arc bases) is cleared on the way.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_chb_tiles(const ChbArgs a)
{
    __shared__ int L[kBH * kBW];
    const int z = a.z0 + blockIdx.z, rows = a.rows, cols = a.cols;
    const MaskRef mask = plane_of(a.masks, z);
    const int nty = tile_row_count(rows, kBH);   // tile_grid deals the tile rows over at most kGridMaxYZ workgroup rows
    for (int by = blockIdx.y; by < nty; by += gridDim.y) {
        if (by != (int)blockIdx.y) __syncthreads();   // the previous tile's lookups are done before L is written again
        const int x0 = blockIdx.x * kBW, y0 = by * kBH;
        const int tx = threadIdx.x & (kBW - 1), half = threadIdx.x >> 7, lane = threadIdx.x & 63;
        const int x = x0 + tx;
        unsigned fgbits = 0;
#pragma unroll
        for (int k = 0; k < kBH / 2; ++k) {
            const int ty = 2 * k + half, y = y0 + ty;
            const bool fg = chb_fg(mask, rows, cols, y, x);
            const unsigned long long gaps = ~__ballot(fg) & ((1ull << lane) - 1ull);   // background lanes left of this one
            const int start = gaps ? 64 - __clzll((long long)gaps) : 0;                 // first lane of this pixel's run
            const int i = ty * kBW + tx;
            L[i] = fg ? i - lane + start : -1;
            fgbits |= (fg ? 1u : 0u) << k;
        }
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < kBH / 2; ++k) {
            if (!((fgbits >> k) & 1u)) continue;
            const int ty = 2 * k + half, i = ty * kBW + tx;
            const bool up = ty > 0;
            const bool n = up && lds_get(L, i - kBW) >= 0;
            const bool nw = up && tx > 0 && lds_get(L, i - kBW - 1) >= 0;
            const bool ne = up && tx < kBW - 1 && lds_get(L, i - kBW + 1) >= 0;
            const bool in_run = lane > 0 && lds_get(L, i - 1) >= 0;   // the left neighbour is in this pixel's run (same initial parent)
            if (!in_run) {
                if (tx == 64 && lds_get(L, i - 1) >= 0) lds_union(L, i, i - 1);   // the run goes on in the other wave's half of the row
                if (n) {
                    lds_union(L, i, i - kBW);   // (nw and ne touch n in their own row)
                } else {
                    if (nw) lds_union(L, i, i - kBW - 1);
                    if (ne) lds_union(L, i, i - kBW + 1);
                }
            } else if (!n && ne) {
                lds_union(L, i, i - kBW + 1);   // every other contact of a pixel inside a run is made by its left neighbour
            }
        }
        __syncthreads();
        const int zbase = z * rows * cols;   // (n * rows * cols <= 2^28)
#pragma unroll 1
        for (int k = 0; k < kBH / 2; ++k) {
            const int ty = 2 * k + half, y = y0 + ty;
            if (y >= rows || x >= cols) continue;
            int v = -1;
            if ((fgbits >> k) & 1u) {
                const int r = lds_find(L, ty * kBW + tx);
                v = zbase + (y0 + r / kBW) * cols + x0 + r % kBW;
            }
            const size_t g = (size_t)zbase + (size_t)y * cols + x;
            a.parent[g] = v;
            a.aux[g] = 0;
        }
    }
}

// ---------------------------------------------------------------------------------------
// k_cc_borders per plane (blockIdx.z): one lane per pixel of a tile's top row and of a tile's left column INSIDE the plane, unions with the
// neighbours across the tile border.  The parent plane holds stacked indices, so finds and unions run on the stacked plane itself; no lane
// looks at a row of another plane.  Other workgroups of the launch change the words this one reads: EVERY access to the parent plane is an
// agent-scope atomic, and the kernel touches nothing else.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_chb_borders(int rows, int cols, int z0, int32_t* parent)
{
    const int zbase = (z0 + (int)blockIdx.z) * rows * cols;
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    const int nty = tile_row_count(rows, kBH), ntx = tile_row_count(cols, kBW);
    const long long n_top = (long long)(nty - 1) * cols, n_left = (long long)(ntx - 1) * rows;
    if (id < n_top) {   // (x, y) on the top row of tile row t >= 1: the three neighbours in row y - 1
        const int x = (int)(id % cols), y = (int)(id / cols + 1) * kBH;
        const int self = zbase + y * cols + x;
        if (g_get(parent, self) < 0) return;
        const int up = self - cols;
        const bool n = g_get(parent, up) >= 0;
        const bool nw = x > 0 && g_get(parent, up - 1) >= 0;
        const bool ne = x < cols - 1 && g_get(parent, up + 1) >= 0;
        if (n) g_union(parent, self, up);
        // with n set, nw / ne are its row neighbours -- already one component with it unless they lie in another tile
        if (nw && (!n || x % kBW == 0)) g_union(parent, self, up - 1);
        if (ne && (!n || x % kBW == kBW - 1)) g_union(parent, self, up + 1);
    } else if (id < n_top + n_left) {   // (x, y) on the left column of tile column t >= 1: the three neighbours in column x - 1
        const long long j = id - n_top;
        const int y = (int)(j % rows), x = (int)(j / rows + 1) * kBW;
        const int self = zbase + y * cols + x;
        if (g_get(parent, self) < 0) return;
        const int left = self - 1;
        const bool w = g_get(parent, left) >= 0;
        const bool nw = y > 0 && g_get(parent, left - cols) >= 0;
        const bool sw = y < rows - 1 && g_get(parent, left + cols) >= 0;
        if (w) g_union(parent, self, left);
        if (nw && (!w || y % kBH == 0)) g_union(parent, self, left - cols);
        if (sw && (!w || y % kBH == kBH - 1)) g_union(parent, self, left + cols);
    }
}

// ---------------------------------------------------------------------------------------
// Step 6, the twins.  block_scan and arc_ok are those of cvs_kernels_chains.hip.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ int chb_block_scan(int v, int* ws, int& total)
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

__device__ __forceinline__ int chb_arc_ok(int a, int arcs, int self) { return (unsigned)a < (unsigned)arcs ? a : self; }

// k_ch_head_apply; the fourth word of an entry is the plane of the chain's first pixel -- the source of its head arc, to[rev[a]] (the pixel
// itself for the pseudo arc of an isolated pixel: rev[a] == a)
__global__ __launch_bounds__(256) void k_chb_head_apply(int arcs, HeadRec* head, const int32_t* part_n, const int32_t* part_len, const int32_t* to,
                                                        const int32_t* rev, int plane_pixels, int32_t* chains, int n_chains)
{
    __shared__ int ws[4];
    const int a0 = blockIdx.x * kChArcBlock + threadIdx.x * 4;
    HeadRec h[4];
    int c = 0, s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        h[k] = a0 + k < arcs ? head[a0 + k] : HeadRec{0, 0};
        c += h[k].len ? 1 : 0;
        s += h[k].len;
    }
    int tc, ts;
    int idx = part_n[blockIdx.x] + chb_block_scan(c, ws, tc);
    int start = part_len[blockIdx.x] + chb_block_scan(s, ws, ts);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!h[k].len) continue;
        if (idx < n_chains) {
            int32_t* t = chains + 4 * (size_t)idx;   // struct cvs_chain: four 4-byte fields
            t[0] = start;
            t[1] = h[k].len;
            t[2] = h[k].flags;
            t[3] = to[chb_arc_ok(rev[a0 + k], arcs, a0 + k)] / plane_pixels;
        }
        head[a0 + k].len = start;   // from here on: where the chain's points begin
        ++idx;
        start += h[k].len;
    }
}

// k_ch_emit; a stacked index q is the pixel (q % cols, (q / cols) % rows) of its plane
__global__ __launch_bounds__(256) void k_chb_emit(int arcs, int rows, int cols, const int32_t* to, const int32_t* rev, const ArcRec* rec,
                                                  const HeadRec* head, int32_t* points, int n_points)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= arcs) return;
    const int ra = chb_arc_ok(rev[a], arcs, a), q = to[a];
    if (ra == a) {
        const int at = head[a].len;
        if (at < n_points) {
            points[2 * (size_t)at] = q % cols;
            points[2 * (size_t)at + 1] = (q / cols) % rows;
        }
        return;
    }
    const ArcRec r = rec[a], rr = rec[ra];
    const int first = rev[chb_arc_ok(rr.next, arcs, a)], other = rev[chb_arc_ok(r.next, arcs, a)];
    if (!(first < other) || (unsigned)first >= (unsigned)arcs) return;   // the chain is listed in the opposite direction
    const HeadRec h = head[first];
    const int pos = rr.dist, len = r.dist + rr.dist + 1;   // arcs before this one, arcs of the chain
    if (pos == 0 && h.len < n_points) {
        const int p0 = to[ra];
        points[2 * (size_t)h.len] = p0 % cols;
        points[2 * (size_t)h.len + 1] = (p0 / cols) % rows;
    }
    if ((h.flags & kChainClosed) && pos + 1 == len) return;   // the arc back into the root
    const long long at = (long long)h.len + pos + 1;
    if (at < n_points) {
        points[2 * (size_t)at] = q % cols;
        points[2 * (size_t)at + 1] = (q / cols) % rows;
    }
}

// One lane per chain.  The table is sorted by plane: chain c opens every plane after its predecessor's up to its own -- the planes in
// between are empty and repeat the pair --, the last chain closes the planes behind its own and stores the totals.  Planes are clamped
// into 0 .. n - 1, so no store leaves the 2 * (n + 1) ints.
__global__ __launch_bounds__(256) void k_chb_ranges(const int32_t* chains, int n_chains, int n_points, int n, int32_t* ranges)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_chains) return;
    auto plane = [&](int k) {
        const int z = chains[4 * (size_t)k + 3];
        return z < 0 ? 0 : (z > n - 1 ? n - 1 : z);
    };
    const int z = plane(c), before = c > 0 ? plane(c - 1) : -1, start = chains[4 * (size_t)c];
    for (int k = before + 1; k <= z; ++k) {
        ranges[2 * k] = c;
        ranges[2 * k + 1] = start;
    }
    if (c == n_chains - 1)
        for (int k = z + 1; k <= n; ++k) {
            ranges[2 * k] = n_chains;
            ranges[2 * k + 1] = n_points;
        }
}

// ---------------------------------------------------------------------------------------
// cvs_chain_refine_batch.  The plane of point i: the largest z in 0 .. n - 1 with ranges[2 * z + 1] <= i.  lo and hi never leave 0 .. n - 1,
// so the search reads inside the table and ends on a plane that exists whatever the table holds.  Behind it: k_chain_refine
// (cvs_kernels_refine.hip), operation for operation.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_chain_refine_batch(const RefineBatchArgs a)
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
    int lo = 0, hi = a.n - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;   // lo < mid <= hi
        if ((long long)a.ranges[2 * (size_t)mid + 1] <= i) lo = mid;
        else hi = mid - 1;
    }
    const MaskRef mr = plane_of(a.maps, lo), tr = plane_of(a.theta, lo / a.n_maps);
    const float* map = static_cast<const float*>(mr.p);
    const float* theta = static_cast<const float*>(tr.p);
    auto at = [&](int r, int c) -> float {
        return ((unsigned)r < (unsigned)a.rows && (unsigned)c < (unsigned)a.cols) ? map[(size_t)r * mr.pitch + c] : 0.0f;
    };
    // all ten loads before the first use: they do not depend on each other
    const float u_l = at(y - 1, x - 1), u_c = at(y - 1, x), u_r = at(y - 1, x + 1);
    const float m_l = at(y, x - 1), m = at(y, x), m_r = at(y, x + 1);
    const float d_l = at(y + 1, x - 1), d_c = at(y + 1, x), d_r = at(y + 1, x + 1);
    const float th = theta[(size_t)y * tr.pitch + x];

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
// launchers
// ---------------------------------------------------------------------------------------
static bool set_ok(const PlaneSet& s) { return s.tab || (s.first.p && s.stride >= 0); }

static bool chb_ok(const ChbArgs& a)
{
    if (a.rows <= 0 || a.cols <= 0 || a.n < 1 || (long long)a.n * a.rows * a.cols > (1LL << 28)) return false;
    return set_ok(a.masks) && a.link && a.parent && a.aux;
}

// one launch per kChbGridZ planes: f(first plane, planes) queues it
template <class F>
static hipError_t each_slab(int n, F f)
{
    for (int z0 = 0; z0 < n; z0 += kChbGridZ) {
        f(z0, n - z0 < kChbGridZ ? n - z0 : kChbGridZ);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_chb_table(const ChbTableArgs& t, MaskRef* tab, hipStream_t s)
{
    if (!tab || t.first < 0 || t.count < 1 || t.count > kChbTableBatch) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_chb_table, dim3(1), dim3(64), 0, s, t, tab);
    return hipGetLastError();
}

hipError_t launch_chb_links(const ChbArgs& a, hipStream_t s)
{
    if (!chb_ok(a)) return hipErrorInvalidValue;
    return each_slab(a.n, [&](int z0, int nz) {
        ChbArgs b = a;
        b.z0 = z0;
        const GridDims gd = tile_grid(a.rows, a.cols, 256, kChbRows, nz);
        hipLaunchKernelGGL(k_chb_links, dim3(gd.x, gd.y, gd.z), dim3(256), 0, s, b);
    });
}

hipError_t launch_chb_tiles(const ChbArgs& a, hipStream_t s)
{
    if (!chb_ok(a)) return hipErrorInvalidValue;
    return each_slab(a.n, [&](int z0, int nz) {
        ChbArgs b = a;
        b.z0 = z0;
        const GridDims gd = tile_grid(a.rows, a.cols, kBW, kBH, nz);
        hipLaunchKernelGGL(k_chb_tiles, dim3(gd.x, gd.y, gd.z), dim3(256), 0, s, b);
    });
}

hipError_t launch_chb_borders(const ChbArgs& a, hipStream_t s)
{
    if (!chb_ok(a)) return hipErrorInvalidValue;
    const long long nty = tile_row_count(a.rows, kBH), ntx = tile_row_count(a.cols, kBW);
    const long long lanes = (nty - 1) * a.cols + (ntx - 1) * a.rows;
    const long long blocks = lanes > 0 ? (lanes + 255) / 256 : 1;   // (a single tile: one workgroup that finds nothing to do)
    return each_slab(a.n, [&](int z0, int nz) {
        hipLaunchKernelGGL(k_chb_borders, dim3((unsigned)blocks, 1, nz), dim3(256), 0, s, a.rows, a.cols, z0, a.parent);
    });
}

hipError_t launch_chb_head_apply(int arcs, HeadRec* head, const int32_t* part_n, const int32_t* part_len, const int32_t* to, const int32_t* rev,
                                 int plane_pixels, int32_t* chains, int n_chains, hipStream_t s)
{
    if (arcs < 1 || !head || !part_n || !part_len || !to || !rev || plane_pixels < 1 || !chains || n_chains < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_chb_head_apply, dim3(ch_scan_blocks(arcs)), dim3(256), 0, s, arcs, head, part_n, part_len, to, rev, plane_pixels, chains,
                       n_chains);
    return hipGetLastError();
}

hipError_t launch_chb_emit(int arcs, int rows, int cols, const int32_t* to, const int32_t* rev, const ArcRec* rec, const HeadRec* head,
                           int32_t* points, int n_points, hipStream_t s)
{
    if (arcs < 1 || rows < 1 || cols < 1 || !to || !rev || !rec || !head || !points || n_points < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_chb_emit, dim3((unsigned)(((long long)arcs + 255) / 256)), dim3(256), 0, s, arcs, rows, cols, to, rev, rec, head, points,
                       n_points);
    return hipGetLastError();
}

hipError_t launch_chb_ranges(const int32_t* chains, int n_chains, int n_points, int n, int32_t* ranges, hipStream_t s)
{
    if (!chains || n_chains < 1 || n_points < 1 || n < 1 || !ranges) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_chb_ranges, dim3((unsigned)(((long long)n_chains + 255) / 256)), dim3(256), 0, s, chains, n_chains, n_points, n, ranges);
    return hipGetLastError();
}

hipError_t launch_chain_refine_batch(const RefineBatchArgs& a, hipStream_t s)
{
    if (a.rows <= 0 || a.cols <= 0 || a.n_maps < 1 || a.n < a.n_maps || a.n % a.n_maps || !set_ok(a.maps) || !set_ok(a.theta)) return hipErrorInvalidValue;
    if (!a.points || a.n_points < 1 || !a.ranges || !a.xy) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_chain_refine_batch, dim3((unsigned)(((long long)a.n_points + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace cvs
