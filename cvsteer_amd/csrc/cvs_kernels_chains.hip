// cvs_kernels_chains.hip -- contour chains (extension beyond the reference): every linked contour of a mask as ordered chains of pixels,
// cut at junctions and free ends (cvs_contour_chains), for gfx950.
//
// Like the component kernels nothing here walks a contour: the launch sequence depends on the image size and, through the number of
// pointer-jumping rounds, on ceil(log2) of the number of arcs -- never on how long or how wound a contour is.  All arithmetic is integer,
// every output position comes from a scan, and the only atomics are a flag store and four counters whose order does not matter.
//
//   1  k_ch_links      the link bits of every pixel (cvs_chains.h: the LINK plane)
//   2  k_cc_tiles, k_cc_borders (cvs_kernels_components.hip)   the parent plane
//      k_ch_nodes      a flag at the root of every component that holds a pixel of degree != 2
//      k_ch_roots      the root of every other component -- a cycle -- becomes a node; the counters the sizes follow from
//   3  k_ch_arc_count, k_scan_partials, k_ch_arc_base          arc ids: the exclusive scan of the links per pixel
//   4  k_ch_arcs       target, opposite arc and successor of every arc
//   5  k_ch_jump       x ceil(log2 arcs): every arc learns the last arc of its direction and its distance to it
//   6  k_ch_heads, k_ch_head_count, k_scan_partials x 2, k_ch_head_apply, k_ch_emit   chain table and points
#include <hip/hip_runtime.h>

#include "cvs_cc_device.h"
#include "cvs_chains.h"

namespace cvs {

constexpr int kChRows = 32;   // rows one workgroup of k_ch_links walks down

__device__ __forceinline__ bool ch_fg(const MaskRef& m, int rows, int cols, int y, int x)
{
    if (y < 0 || y >= rows || x < 0 || x >= cols) return false;
    if (m.u8) return static_cast<const unsigned char*>(m.p)[(size_t)y * m.pitch + x] != 0;
    return static_cast<const float*>(m.p)[(size_t)y * m.pitch + x] > 0.0f;   // NaN, zeros, negatives: background
}

// ---------------------------------------------------------------------------------------
// Step 1.  One lane per column, a workgroup walks 32 rows down: each lane carries the foreground bits of rows y - 1, y, y + 1 of its own
// column (one load per row) and takes the neighbouring columns from the lanes beside it; the two end lanes of a wave follow the column
// beyond their end themselves.  A diagonal is a link only when neither pixel 4-adjacent to both ends is foreground.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ch_links(const MaskRef mask, int rows, int cols, uint16_t* link)
{
    const int lane = threadIdx.x & 63;
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int xe = lane == 0 ? x - 1 : (lane == 63 ? x + 1 : -1);
    const int bands = tile_row_count(rows, kChRows);   // tile_grid deals the 32-row bands over at most kGridMaxYZ workgroup rows
    for (int by = blockIdx.y; by < bands; by += gridDim.y) {
        const int y0 = by * kChRows, y1 = y0 + kChRows < rows ? y0 + kChRows : rows;
        // bit 0: row y - 1, bit 1: row y, bit 2: row y + 1 (after the shift at the top of the loop)
        unsigned own = (ch_fg(mask, rows, cols, y0 - 1, x) ? 2u : 0u) | (ch_fg(mask, rows, cols, y0, x) ? 4u : 0u);
        unsigned ext = (ch_fg(mask, rows, cols, y0 - 1, xe) ? 2u : 0u) | (ch_fg(mask, rows, cols, y0, xe) ? 4u : 0u);
        for (int y = y0; y < y1; ++y) {
            own = (own >> 1) | (ch_fg(mask, rows, cols, y + 1, x) ? 4u : 0u);
            ext = (ext >> 1) | (ch_fg(mask, rows, cols, y + 1, xe) ? 4u : 0u);
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
// Step 2.  k_ch_nodes: one lane per pixel; pixels of degree != 2 look their root up, and the first lane of every run of equal roots in
// a wave sets the root's flag (every writer stores the same 1).  k_ch_roots: a root without a flag heads a component whose pixels all
// have degree 2 -- one cycle -- and becomes the node at which that cycle is cut; it is the component's smallest linear index.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ch_nodes(int n, const uint16_t* link, const int32_t* parent, int32_t* flag)
{
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned v = i < n ? link[i] : 0u;
    const int key = (v & kChNode) ? root_of(parent, (int)i) : -1;
    bool head;
    int end;
    run_of(key, lane, head, end);
    if (head && key >= 0) __hip_atomic_store(&flag[key], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_ch_roots(int n, uint16_t* link, const int32_t* parent, const int32_t* flag, int32_t* counters)
{
    int iso = 0, sum = 0, node = 0, closed = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const unsigned v = link[i];
        if (!(v & kChFg)) continue;
        const int deg = __popc(v & 0xffu);
        if (deg == 2 && parent[i] == (int)i && flag[i] == 0) {
            link[i] = (uint16_t)(v | kChNode);
            ++closed;
        }
        iso += deg == 0 ? 1 : 0;
        sum += deg;
        node += deg != 2 ? deg : 0;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        iso += __shfl_xor(iso, d, 64);
        sum += __shfl_xor(sum, d, 64);
        node += __shfl_xor(node, d, 64);
        closed += __shfl_xor(closed, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {   // integer sums: no result depends on the order
        if (iso) atomicAdd(&counters[kChIsolated], iso);
        if (sum) atomicAdd(&counters[kChSumDeg], sum);
        if (node) atomicAdd(&counters[kChNodeDeg], node);
        if (closed) atomicAdd(&counters[kChClosed], closed);
    }
}

// ---------------------------------------------------------------------------------------
// Scans of int values.  block_scan: the exclusive prefix of v over the workgroup's 256 lanes in thread order, and the workgroup's sum.
// A lane owns CONSECUTIVE elements (16 link words = two 16-byte loads; 4 head records = two 16-byte loads), so the order inside a
// workgroup's range is the linear one.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ int block_scan(int v, int* ws, int& total)
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

__device__ __forceinline__ int arcs_of(unsigned v)   // a pixel without links owns one pseudo arc
{
    const int deg = __popc(v & 0xffu);
    return (v & kChFg) ? (deg ? deg : 1) : 0;
}

// the lane's 16 link words, two to a register; words beyond n read as background
__device__ __forceinline__ void load_links(const uint16_t* link, long long i0, long long n, unsigned (&w)[8])
{
    if (i0 + 16 <= n) {   // (the plane is 256-byte aligned and i0 a multiple of 16)
        const uint4 a = *reinterpret_cast<const uint4*>(link + i0), b = *reinterpret_cast<const uint4*>(link + i0 + 8);
        w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
        return;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const unsigned lo = i0 + 2 * k < n ? link[i0 + 2 * k] : 0u, hi = i0 + 2 * k + 1 < n ? link[i0 + 2 * k + 1] : 0u;
        w[k] = lo | (hi << 16);
    }
}

__global__ __launch_bounds__(256) void k_ch_arc_count(long long n, const uint16_t* link, int32_t* partials)
{
    __shared__ int ws[4];
    unsigned w[8];
    load_links(link, (long long)blockIdx.x * kCcScanBlock + threadIdx.x * 16, n, w);
    int c = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) c += arcs_of(w[k] & 0xffffu) + arcs_of(w[k] >> 16);
    int total;
    (void)block_scan(c, ws, total);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_ch_arc_base(long long n, const uint16_t* link, const int32_t* partials, int32_t* base)
{
    __shared__ int ws[4];
    const long long i0 = (long long)blockIdx.x * kCcScanBlock + threadIdx.x * 16;
    unsigned w[8];
    load_links(link, i0, n, w);
    int c = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) c += arcs_of(w[k] & 0xffffu) + arcs_of(w[k] >> 16);
    int total;
    int run = partials[blockIdx.x] + block_scan(c, ws, total);
    int out[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        out[2 * k] = run;
        run += arcs_of(w[k] & 0xffffu);
        out[2 * k + 1] = run;
        run += arcs_of(w[k] >> 16);
    }
    if (i0 + 16 <= n) {
        int4* o = reinterpret_cast<int4*>(base + i0);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = make_int4(out[4 * k], out[4 * k + 1], out[4 * k + 2], out[4 * k + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (i0 + k < n) base[i0 + k] = out[k];
    }
}

// ---------------------------------------------------------------------------------------
// Step 4.  One lane per pixel writes the arcs that leave it.  Arc p -> q in direction d: its opposite arc is q's link in direction 7 - d;
// it is terminal when q is a node, and otherwise goes on along q's other link (q has exactly two).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ch_arcs(int n, int cols, const uint16_t* link, const int32_t* base, int arcs, int32_t* to, int32_t* rev,
                                                 ArcRec* rec)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned v = link[i];
    if (!(v & kChFg)) return;
    const int p = (int)i, b = base[i];
    const unsigned bits = v & 0xffu;
    if (!bits) {
        if (b < arcs) {
            to[b] = p;
            rev[b] = b;
            rec[b] = ArcRec{b, 0};
        }
        return;
    }
    int k = 0;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        if (!((bits >> d) & 1u)) continue;
        const int dy = d < 3 ? -1 : (d < 5 ? 0 : 1), dx = (d == 0 || d == 3 || d == 5) ? -1 : ((d == 1 || d == 6) ? 0 : 1);
        const int q = p + dy * cols + dx, back = 7 - d;
        const int a = b + k++;
        const unsigned vq = link[q], lq = vq & 0xffu;
        const int bq = base[q];
        if (a >= arcs) continue;
        to[a] = q;
        rev[a] = bq + __popc(lq & ((1u << back) - 1u));
        if (vq & kChNode) {
            rec[a] = ArcRec{a, 0};
        } else {
            const unsigned other = lq & ~(1u << back);
            rec[a] = ArcRec{bq + (other > (1u << back) ? 1 : 0), 1};
        }
    }
}

// ---------------------------------------------------------------------------------------
// Step 5.  Pointer jumping (Wyllie), double-buffered: a terminal arc points at itself with distance 0, so a jump that has arrived adds
// nothing.  After r rounds every arc within 2^r arcs of its direction's last arc points at it.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ch_jump(int arcs, const ArcRec* in, ArcRec* out)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= arcs) return;
    const ArcRec r = in[a];
    const ArcRec t = in[(unsigned)r.next < (unsigned)arcs ? r.next : a];
    out[a] = ArcRec{t.next, r.dist + t.dist};
}

// ---------------------------------------------------------------------------------------
// Step 6.  With last(a) = rec[a].next: the first arc of a's direction is rev[last(rev[a])], and a direction is the canonical one of its
// chain when its first arc has the smaller id of the two -- ids ascend by (lin(from), lin(to)), which is the key the contract compares;
// the same comparison sends a cycle from its root towards the smaller neighbour.  An arc is first in its direction when its opposite arc
// is terminal.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ int arc_ok(int a, int arcs, int self) { return (unsigned)a < (unsigned)arcs ? a : self; }

__global__ __launch_bounds__(256) void k_ch_heads(int arcs, const uint16_t* link, const int32_t* to, const int32_t* rev, const ArcRec* rec,
                                                  HeadRec* head)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= arcs) return;
    HeadRec h = {0, 0};
    const int ra = arc_ok(rev[a], arcs, a);
    if (ra == a) {
        h.len = 1;   // an isolated pixel
    } else if (rec[ra].dist == 0) {
        const ArcRec r = rec[a];
        const int last = arc_ok(r.next, arcs, a);
        if (a < rev[last]) {
            const int degf = __popc(link[to[ra]] & 0xffu), degt = __popc(link[to[last]] & 0xffu);
            const bool closed = degf == 2;   // a node of degree 2 is the root of a cycle: listed once, the root not repeated
            h.len = r.dist + (closed ? 1 : 2);
            h.flags = closed ? kChainClosed : ((degf >= 3 ? kChainHeadJunction : 0) | (degt >= 3 ? kChainTailJunction : 0));
        }
    }
    head[a] = h;
}

__global__ __launch_bounds__(256) void k_ch_head_count(int arcs, const HeadRec* head, int32_t* part_n, int32_t* part_len)
{
    __shared__ int ws[4];
    const int a0 = blockIdx.x * kChArcBlock + threadIdx.x * 4;
    int c = 0, s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int len = a0 + k < arcs ? head[a0 + k].len : 0;
        c += len ? 1 : 0;
        s += len;
    }
    int tc, ts;
    (void)block_scan(c, ws, tc);
    (void)block_scan(s, ws, ts);
    if (threadIdx.x == 0) {
        part_n[blockIdx.x] = tc;
        part_len[blockIdx.x] = ts;
    }
}

__global__ __launch_bounds__(256) void k_ch_head_apply(int arcs, HeadRec* head, const int32_t* part_n, const int32_t* part_len, int32_t* chains,
                                                       int n_chains)
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
    int idx = part_n[blockIdx.x] + block_scan(c, ws, tc);
    int start = part_len[blockIdx.x] + block_scan(s, ws, ts);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!h[k].len) continue;
        if (idx < n_chains) {
            int32_t* t = chains + 4 * (size_t)idx;   // struct cvs_chain: four 4-byte fields
            t[0] = start;
            t[1] = h[k].len;
            t[2] = h[k].flags;
            t[3] = 0;
        }
        head[a0 + k].len = start;   // from here on: where the chain's points begin
        ++idx;
        start += h[k].len;
    }
}

__global__ __launch_bounds__(256) void k_ch_emit(int arcs, int cols, const int32_t* to, const int32_t* rev, const ArcRec* rec, const HeadRec* head,
                                                 int32_t* points, int n_points)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= arcs) return;
    const int ra = arc_ok(rev[a], arcs, a), q = to[a];
    if (ra == a) {
        const int at = head[a].len;
        if (at < n_points) {
            points[2 * (size_t)at] = q % cols;
            points[2 * (size_t)at + 1] = q / cols;
        }
        return;
    }
    const ArcRec r = rec[a], rr = rec[ra];
    const int first = rev[arc_ok(rr.next, arcs, a)], other = rev[arc_ok(r.next, arcs, a)];
    if (!(first < other) || (unsigned)first >= (unsigned)arcs) return;   // the chain is listed in the opposite direction
    const HeadRec h = head[first];
    const int pos = rr.dist, len = r.dist + rr.dist + 1;   // arcs before this one, arcs of the chain
    if (pos == 0 && h.len < n_points) {
        const int p0 = to[ra];
        points[2 * (size_t)h.len] = p0 % cols;
        points[2 * (size_t)h.len + 1] = p0 / cols;
    }
    if ((h.flags & kChainClosed) && pos + 1 == len) return;   // the arc back into the root
    const long long at = (long long)h.len + pos + 1;
    if (at < n_points) {
        points[2 * (size_t)at] = q % cols;
        points[2 * (size_t)at + 1] = q / cols;
    }
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
static bool size_ok(int rows, int cols) { return rows > 0 && cols > 0 && (long long)rows * cols <= (1LL << 28); }
static unsigned blocks_of(long long n, int per) { return (unsigned)((n + per - 1) / per); }

hipError_t launch_ch_links(const MaskRef& mask, int rows, int cols, uint16_t* link, hipStream_t s)
{
    if (!size_ok(rows, cols) || !mask.p || !link) return hipErrorInvalidValue;
    const GridDims gd = tile_grid(rows, cols, 256, kChRows, 1);
    hipLaunchKernelGGL(k_ch_links, dim3(gd.x, gd.y, gd.z), dim3(256), 0, s, mask, rows, cols, link);
    return hipGetLastError();
}

hipError_t launch_ch_nodes(int rows, int cols, const uint16_t* link, const int32_t* parent, int32_t* flag, hipStream_t s)
{
    if (!size_ok(rows, cols) || !link || !parent || !flag) return hipErrorInvalidValue;
    const int n = rows * cols;
    hipLaunchKernelGGL(k_ch_nodes, dim3(blocks_of(n, 256)), dim3(256), 0, s, n, link, parent, flag);
    return hipGetLastError();
}

hipError_t launch_ch_roots(int rows, int cols, uint16_t* link, const int32_t* parent, const int32_t* flag, int32_t* counters, hipStream_t s)
{
    if (!size_ok(rows, cols) || !link || !parent || !flag || !counters) return hipErrorInvalidValue;
    const int n = rows * cols;
    const unsigned blocks = blocks_of(n, 256);
    hipLaunchKernelGGL(k_ch_roots, dim3(blocks < 4096u ? blocks : 4096u), dim3(256), 0, s, n, link, parent, flag, counters);
    return hipGetLastError();
}

hipError_t launch_ch_arc_count(int rows, int cols, const uint16_t* link, int32_t* partials, hipStream_t s)
{
    if (!size_ok(rows, cols) || !link || !partials) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ch_arc_count, dim3(scan_blocks(rows, cols)), dim3(256), 0, s, (long long)rows * cols, link, partials);
    return hipGetLastError();
}

hipError_t launch_ch_arc_base(int rows, int cols, const uint16_t* link, const int32_t* partials, int32_t* base, hipStream_t s)
{
    if (!size_ok(rows, cols) || !link || !partials || !base) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ch_arc_base, dim3(scan_blocks(rows, cols)), dim3(256), 0, s, (long long)rows * cols, link, partials, base);
    return hipGetLastError();
}

hipError_t launch_ch_arcs(int rows, int cols, const uint16_t* link, const int32_t* base, int arcs, int32_t* to, int32_t* rev, ArcRec* rec,
                          hipStream_t s)
{
    if (!size_ok(rows, cols) || !link || !base || arcs < 1 || !to || !rev || !rec) return hipErrorInvalidValue;
    const int n = rows * cols;
    hipLaunchKernelGGL(k_ch_arcs, dim3(blocks_of(n, 256)), dim3(256), 0, s, n, cols, link, base, arcs, to, rev, rec);
    return hipGetLastError();
}

hipError_t launch_ch_jump(int arcs, const ArcRec* in, ArcRec* out, hipStream_t s)
{
    if (arcs < 1 || !in || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ch_jump, dim3(blocks_of(arcs, 256)), dim3(256), 0, s, arcs, in, out);
    return hipGetLastError();
}

hipError_t launch_ch_heads(int arcs, const uint16_t* link, const int32_t* to, const int32_t* rev, const ArcRec* rec, HeadRec* head, hipStream_t s)
{
    if (arcs < 1 || !link || !to || !rev || !rec || !head) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ch_heads, dim3(blocks_of(arcs, 256)), dim3(256), 0, s, arcs, link, to, rev, rec, head);
    return hipGetLastError();
}

hipError_t launch_ch_head_count(int arcs, const HeadRec* head, int32_t* part_n, int32_t* part_len, hipStream_t s)
{
    if (arcs < 1 || !head || !part_n || !part_len) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ch_head_count, dim3(ch_scan_blocks(arcs)), dim3(256), 0, s, arcs, head, part_n, part_len);
    return hipGetLastError();
}

hipError_t launch_ch_head_apply(int arcs, HeadRec* head, const int32_t* part_n, const int32_t* part_len, int32_t* chains, int n_chains,
                                hipStream_t s)
{
    if (arcs < 1 || !head || !part_n || !part_len || !chains || n_chains < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ch_head_apply, dim3(ch_scan_blocks(arcs)), dim3(256), 0, s, arcs, head, part_n, part_len, chains, n_chains);
    return hipGetLastError();
}

hipError_t launch_ch_emit(int arcs, int cols, const int32_t* to, const int32_t* rev, const ArcRec* rec, const HeadRec* head, int32_t* points,
                          int n_points, hipStream_t s)
{
    if (arcs < 1 || cols < 1 || !to || !rev || !rec || !head || !points || n_points < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ch_emit, dim3(blocks_of(arcs, 256)), dim3(256), 0, s, arcs, cols, to, rev, rec, head, points, n_points);
    return hipGetLastError();
}

}  // namespace cvs
