// cvs_kernels_paths.hip -- contour paths (extension beyond the reference): the chains of a chain table stitched into paths over the mutual
// joins of a join table (cvs_chain_paths), for gfx950.  Integer arithmetic only; include/cvsteer_hip.h has the contract.
//
// One lane per END in every launch but the last.  With r = path_rounds(n_chains):
//   1      k_path_links      succ / pred of every end from the LINKED test, the chain's weight (L - 1 emitted points as a later member)
//   r      k_path_jump_min   pointer jumping along succ: the last end of the walk (or, on a cycle, some end of it) and the smallest end
//   1      k_path_cut        every cycle is cut in front of its smallest end; the ranking starts from pred
//   r      k_path_jump_rank  pointer jumping along pred: the first end of the walk, the member rank and the points before the member
//   1 + 3  k_path_count, k_scan_partials x 3 (cvs_kernels_components.hip)   paths, path points and members per 1024 ends
//   1      k_path_apply      number, start and first member of every path (block scans on top of the partials): paths, info, counts
//   1      k_path_emit       16 lanes per end: the member record and the member's points
// WHAT MAKES IT SAFE ON ANY BYTES.  A link exists only where LINKED holds, and LINKED is symmetric: succ and pred are mutually inverse
// partial maps on 0 .. 2 n_chains - 1, so following either stays inside the scratch, and every end has at most one of each.  Both
// jumping kernels read one buffer and write the other (the ranks are sums: an update in place would count a neighbour's new value
// twice); a list's last end points at itself with weight 0, so rounds past the end change nothing.  EVERY LOOP HAS A STATIC BOUND: the
// rounds are launches, counted on the host from n_chains alone; the only loop in a kernel is the copy of a member's points, L / 16 steps
// of an entry that was checked against n_points.  No lane waits for another, no atomic, nothing spins.  Chain entries are checked
// before they are addresses (chain_entry), partners before they are indices, and every store of a point is held to n_points, every
// store of a record to n_chains -- the sums of a table whose entries overlap may exceed either (they are formed modulo 2^32).
#include <hip/hip_runtime.h>

#include "cvs_chain_device.h"
#include "cvs_paths.h"

namespace cvs {

namespace {

constexpr int kPtBlock = 256;   // ends per workgroup
constexpr int kPtGroup = 16;    // lanes per end in k_path_emit
static_assert(2ll * kPathMaxChains * kPtGroup / kPtBlock <= (long long)kGridMaxX, "one workgroup per 16 ends never meets the grid bound");
static_assert(kPathScanBlock == 4 * kPtBlock, "a lane of the scan owns 4 consecutive ends");

// per end, in scratch
struct alignas(16) PtLink {   // launch 1
    int32_t succ, pred;       // the entry end that follows / precedes this one in its walk; -1: none
    int32_t w;                // L - 1 of the end's chain (0 for an invalid entry)
    int32_t kind;             // 0: invalid entry; 1: valid, no ends; 2: has ends
};
struct alignas(8) PtMin {     // the r rounds along succ
    int32_t ptr;              // 2^round ends ahead, or the walk's last end
    int32_t mn;               // the smallest end from this one up to ptr
};
struct alignas(16) PtRank {   // the r rounds along pred
    int32_t ptr;              // 2^round ends back, or the walk's first end
    uint32_t rank, before;    // members, and the sum of their w, from ptr (inclusive) up to this end (exclusive)
    int32_t pad;
};
struct alignas(16) PtRoot {   // k_path_apply, at the first end of a canonical walk; path = -1 everywhere else
    int32_t path;
    uint32_t start, first_member;
    int32_t cycle;
};
static_assert(sizeof(PtLink) + 2 * sizeof(PtMin) + 2 * sizeof(PtRank) + sizeof(PtRoot) == kPathEndBytes, "the scratch per end");

struct PtScratch {
    PtLink* link;
    PtMin* mn[2];
    PtRank* rk[2];
    PtRoot* root;
    int32_t* part[3];   // paths, path points, members
};
__host__ __device__ inline PtScratch pt_scratch(unsigned char* base, int n_chains)
{
    const size_t n = 2 * (size_t)n_chains;
    PtScratch s;
    s.link = reinterpret_cast<PtLink*>(base);
    s.mn[0] = reinterpret_cast<PtMin*>(base + n * 16);
    s.mn[1] = reinterpret_cast<PtMin*>(base + n * 24);
    s.rk[0] = reinterpret_cast<PtRank*>(base + n * 32);
    s.rk[1] = reinterpret_cast<PtRank*>(base + n * 48);
    s.root = reinterpret_cast<PtRoot*>(base + n * 64);
    for (int k = 0; k < 3; ++k) s.part[k] = reinterpret_cast<int32_t*>(base + n * kPathEndBytes + k * path_partials_bytes(n_chains));
    return s;
}

__device__ __forceinline__ long long pt_id() { return (long long)blockIdx.x * kPtBlock + threadIdx.x; }

__device__ __forceinline__ bool pt_has_ends(const PathArgs& a, int c)
{
    const ChainEntry e = chain_entry(a.chains, c, a.n_points);
    return e.ok() && e.len >= 2 && !(e.flags & kChainClosed);
}

// the partner of end e if LINKED(e), else -1.  has_ends: of e's own chain.  Of a join record only partner (word 3) and flags (word 4)
// are read, and a partner is an index only once it lies in 0 .. 2 n_chains - 1.
__device__ __forceinline__ int pt_linked(const PathArgs& a, int e, bool has_ends)
{
    if (!has_ends) return -1;
    const int32_t* j = a.joins + (size_t)kJoinWords * e;
    const int p = j[3];
    if (!(j[4] & kJoinMutual) || p < 0 || p >= 2ll * a.n_chains || p == e) return -1;
    if (!pt_has_ends(a, p >> 1)) return -1;
    const int32_t* q = a.joins + (size_t)kJoinWords * p;
    return (q[4] & kJoinMutual) && q[3] == e ? p : -1;
}

// does the walk of end e close on itself: after the r rounds along succ, the end e points at has a successor (the last end of an open
// walk has none)
__device__ __forceinline__ bool pt_on_cycle(const PtLink* link, const PtMin* mn, int e) { return link[mn[e].ptr].succ >= 0; }

// what end e starts: a canonical path or nothing
struct PtStart {
    bool path;            // e is the first entry end of a canonical walk
    bool cycle;
    int last;             // the entry end of the last member
    uint32_t len, members;
};
__device__ __forceinline__ PtStart pt_start(const PtLink* link, const PtMin* mn, const PtRank* rk, int e)
{
    PtStart s{false, false, e, 0u, 0u};
    const PtLink l = link[e];
    if (l.kind == 1) {   // a chain without ends: one member, entered through its head
        s.path = (e & 1) == 0;
        s.len = (uint32_t)l.w + 1u;
        s.members = 1u;
    } else if (l.kind == 2 && rk[e].ptr == e) {   // the first end of a walk; on a cycle: its smallest end
        s.cycle = pt_on_cycle(link, mn, e);
        s.last = s.cycle ? l.pred : mn[e].ptr;
        // the twin starts at last ^ 1; a cycle's smallest end of both twins is a head
        s.path = s.cycle ? (e & 1) == 0 : e < (s.last ^ 1);
        const PtRank r = rk[s.last];
        s.len = r.before + (uint32_t)link[s.last].w + (s.cycle ? 0u : 1u);
        s.members = r.rank + 1u;
    }
    return s;
}

// the exclusive prefix of v over the workgroup's 256 lanes in thread order, and the workgroup's sum: the block scan of the chain and
// polyline kernels (block_scan, pl_block_scan), on unsigned words
__device__ __forceinline__ uint32_t pt_block_scan(uint32_t v, uint32_t* ws, uint32_t& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
        const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) ws[wave] = incl;
    __syncthreads();
    uint32_t pre = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t t = ws[w];
        pre += w < wave ? t : 0u;
        total += t;
    }
    __syncthreads();   // ws may be used again
    return pre + incl - v;
}

}  // namespace

__global__ __launch_bounds__(kPtBlock) void k_path_links(const PathArgs a)
{
    const long long id = pt_id();
    if (id >= 2ll * a.n_chains) return;
    const int e = (int)id;
    const PtScratch s = pt_scratch(a.scratch, a.n_chains);
    const ChainEntry c = chain_entry(a.chains, e >> 1, a.n_points);
    const bool ok = c.ok(), ends = ok && c.len >= 2 && !(c.flags & kChainClosed);
    const int mine = pt_linked(a, e, ends), other = pt_linked(a, e ^ 1, ends);
    PtLink l;
    l.succ = other;                          // out through the other end, into its partner
    l.pred = mine >= 0 ? (mine ^ 1) : -1;    // whoever leaves through this end's partner came in through that chain's other end
    l.w = ok ? c.len - 1 : 0;
    l.kind = !ok ? 0 : ends ? 2 : 1;
    s.link[e] = l;
    s.mn[0][e] = PtMin{other >= 0 ? other : e, e};
}

__global__ __launch_bounds__(kPtBlock) void k_path_jump_min(const PtMin* __restrict__ src, PtMin* __restrict__ dst, long long n_ends)
{
    const long long id = pt_id();
    if (id >= n_ends) return;
    const PtMin v = src[id], q = src[v.ptr];
    dst[id] = PtMin{q.ptr, min(v.mn, q.mn)};
}

__global__ __launch_bounds__(kPtBlock) void k_path_cut(const PtLink* __restrict__ link, const PtMin* __restrict__ mn, PtRank* __restrict__ rk,
                                                       long long n_ends)
{
    const long long id = pt_id();
    if (id >= n_ends) return;
    const int e = (int)id;
    const PtLink l = link[e];
    int pred = l.pred;
    if (pred >= 0 && mn[e].mn == e && pt_on_cycle(link, mn, e)) pred = -1;   // the smallest end of a cycle is where its walk starts
    rk[e] = pred >= 0 ? PtRank{pred, 1u, (uint32_t)link[pred].w, 0} : PtRank{e, 0u, 0u, 0};
}

__global__ __launch_bounds__(kPtBlock) void k_path_jump_rank(const PtRank* __restrict__ src, PtRank* __restrict__ dst, long long n_ends)
{
    const long long id = pt_id();
    if (id >= n_ends) return;
    const PtRank v = src[id], q = src[v.ptr];
    dst[id] = PtRank{q.ptr, v.rank + q.rank, v.before + q.before, 0};
}

__global__ __launch_bounds__(kPtBlock) void k_path_count(const PtLink* __restrict__ link, const PtMin* __restrict__ mn,
                                                         const PtRank* __restrict__ rk, long long n_ends, int32_t* part_n, int32_t* part_len,
                                                         int32_t* part_mem)
{
    __shared__ uint32_t ws[4];
    const long long e0 = (long long)blockIdx.x * kPathScanBlock + threadIdx.x * 4;
    uint32_t n = 0, len = 0, mem = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (e0 + k >= n_ends) continue;
        const PtStart s = pt_start(link, mn, rk, (int)(e0 + k));
        n += s.path ? 1u : 0u;
        len += s.path ? s.len : 0u;
        mem += s.path ? s.members : 0u;
    }
    uint32_t tn, tl, tm;
    (void)pt_block_scan(n, ws, tn);
    (void)pt_block_scan(len, ws, tl);
    (void)pt_block_scan(mem, ws, tm);
    if (threadIdx.x == 0) {
        part_n[blockIdx.x] = (int32_t)tn;
        part_len[blockIdx.x] = (int32_t)tl;
        part_mem[blockIdx.x] = (int32_t)tm;
    }
}

__global__ __launch_bounds__(kPtBlock) void k_path_apply(const PathArgs a, const PtMin* __restrict__ mn, const PtRank* __restrict__ rk)
{
    __shared__ uint32_t ws[4];
    const PtScratch sc = pt_scratch(a.scratch, a.n_chains);
    const long long n_ends = 2ll * a.n_chains, e0 = (long long)blockIdx.x * kPathScanBlock + threadIdx.x * 4;
    PtStart st[4];
    uint32_t n = 0, len = 0, mem = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        st[k] = e0 + k < n_ends ? pt_start(sc.link, mn, rk, (int)(e0 + k)) : PtStart{false, false, 0, 0u, 0u};
        n += st[k].path ? 1u : 0u;
        len += st[k].path ? st[k].len : 0u;
        mem += st[k].path ? st[k].members : 0u;
    }
    uint32_t total;
    uint32_t path = (uint32_t)sc.part[0][blockIdx.x] + pt_block_scan(n, ws, total);
    uint32_t start = (uint32_t)sc.part[1][blockIdx.x] + pt_block_scan(len, ws, total);
    uint32_t member = (uint32_t)sc.part[2][blockIdx.x] + pt_block_scan(mem, ws, total);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.counts[0] = sc.part[0][gridDim.x];
        a.counts[1] = sc.part[1][gridDim.x];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (e0 + k >= n_ends) continue;
        const int e = (int)(e0 + k);
        const PtStart s = st[k];
        sc.root[e] = s.path ? PtRoot{(int32_t)path, start, member, s.cycle ? 1 : 0} : PtRoot{-1, 0u, 0u, 0};
        if (!s.path) continue;
        if (path < (uint32_t)a.n_chains) {   // (always: at most one of a chain's two ends starts a path)
            const int exit_end = s.last ^ 1;
            const int f0 = a.chains[4 * (size_t)(e >> 1) + 2], plane = a.chains[4 * (size_t)(e >> 1) + 3];
            const int f1 = a.chains[4 * (size_t)(exit_end >> 1) + 2];
            int flags;
            if (s.cycle || (f0 & kChainClosed)) {
                flags = kChainClosed;
            } else {
                const bool head = (f0 & ((e & 1) ? kChainTailJunction : kChainHeadJunction)) != 0;
                const bool tail = (f1 & ((exit_end & 1) ? kChainTailJunction : kChainHeadJunction)) != 0;
                flags = (head ? kChainHeadJunction : 0) | (tail ? kChainTailJunction : 0);
            }
            int32_t* p = a.paths + 4 * (size_t)path;
            p[0] = (int32_t)start, p[1] = (int32_t)s.len, p[2] = flags, p[3] = plane;
            int32_t* i = a.info + 4 * (size_t)path;
            i[0] = (int32_t)member, i[1] = (int32_t)s.members, i[2] = e, i[3] = exit_end;
        }
        path += 1u;
        start += s.len;
        member += s.members;
    }
}

__global__ __launch_bounds__(kPtBlock) void k_path_emit(const PathArgs a, const PtRank* __restrict__ rk)
{
    const long long t = pt_id();
    const long long id = t / kPtGroup;
    const int sub = (int)(t % kPtGroup);
    if (id >= 2ll * a.n_chains) return;
    const int e = (int)id;
    const PtScratch sc = pt_scratch(a.scratch, a.n_chains);
    const PtLink l = sc.link[e];
    PtRoot root;
    uint32_t rank = 0, before = 0;
    bool last = false;
    if (l.kind == 1) {
        if (e & 1) return;
        root = sc.root[e];
    } else if (l.kind == 2) {
        const PtRank r = rk[e];
        root = sc.root[r.ptr];
        rank = r.rank;
        before = r.before;
        last = root.cycle && sc.link[r.ptr].pred == e;   // the last member of a cycle also drops its last position
    } else {
        return;
    }
    if (root.path < 0) return;   // the twin of a canonical walk
    const ChainEntry c = chain_entry(a.chains, e >> 1, a.n_points);
    if (!c.ok()) return;         // (never: kind says it is)
    const int drop = rank > 0 ? 1 : 0;
    const uint32_t first = root.start + before + (uint32_t)drop;
    const uint32_t m = root.first_member + rank;
    if (sub == 0 && m < (uint32_t)a.n_chains) {
        int32_t* r = a.members + 4 * (size_t)m;
        r[0] = e >> 1, r[1] = (e & 1) ? kMemberReversed : 0, r[2] = root.path, r[3] = (int32_t)first;
    }
    const int count = c.len - drop - (last ? 1 : 0);
    const WordPair* src = reinterpret_cast<const WordPair*>(a.points);
    WordPair* dst = reinterpret_cast<WordPair*>(a.path_points);
    const WordPair* sxy = reinterpret_cast<const WordPair*>(a.xy);
    WordPair* dxy = reinterpret_cast<WordPair*>(a.path_xy);
#pragma unroll 1
    for (int j = sub; j < count; j += kPtGroup) {
        const int i = j + drop;
        const int pos = (e & 1) ? c.start + c.len - 1 - i : c.start + i;   // inside S .. S + L - 1, which lies inside `points`
        const uint32_t at = first + (uint32_t)j;
        if (at >= (uint32_t)a.n_points) continue;
        dst[at] = src[pos];
        if (a.index) a.index[at] = pos;
        if (sxy) dxy[at] = sxy[pos];
    }
}

// ---------------------------------------------------------------------------------------
// the launch sequence: a function of n_chains alone
// ---------------------------------------------------------------------------------------
static bool paths_ok(const PathArgs& a)
{
    return a.n_chains >= 1 && a.n_chains <= kPathMaxChains && a.n_points >= 0 && a.n_points <= (1 << 30) && a.chains && a.joins &&
           (a.n_points == 0 || (a.points && a.path_points)) && a.paths && a.info && a.members && a.counts && a.scratch &&
           (a.xy != nullptr) == (a.path_xy != nullptr) && reinterpret_cast<uintptr_t>(a.scratch) % 16 == 0;
}

hipError_t launch_paths(const PathArgs& a, hipStream_t s)
{
    if (!paths_ok(a)) return hipErrorInvalidValue;
    const long long n_ends = 2ll * a.n_chains;
    const PtScratch sc = pt_scratch(a.scratch, a.n_chains);
    const GridDims g = list_grid(n_ends, kPtBlock);
    const dim3 grid(g.x, g.y, g.z), block(kPtBlock);
    const int rounds = path_rounds(a.n_chains), blocks = path_scan_blocks(a.n_chains);
    hipError_t e;

    hipLaunchKernelGGL(k_path_links, grid, block, 0, s, a);
    int cur = 0;
    for (int r = 0; r < rounds; ++r, cur ^= 1) hipLaunchKernelGGL(k_path_jump_min, grid, block, 0, s, sc.mn[cur], sc.mn[cur ^ 1], n_ends);
    const PtMin* mn = sc.mn[cur];
    hipLaunchKernelGGL(k_path_cut, grid, block, 0, s, sc.link, mn, sc.rk[0], n_ends);
    cur = 0;
    for (int r = 0; r < rounds; ++r, cur ^= 1) hipLaunchKernelGGL(k_path_jump_rank, grid, block, 0, s, sc.rk[cur], sc.rk[cur ^ 1], n_ends);
    const PtRank* rk = sc.rk[cur];
    if ((e = hipGetLastError()) != hipSuccess) return e;

    hipLaunchKernelGGL(k_path_count, dim3(blocks), block, 0, s, sc.link, mn, rk, n_ends, sc.part[0], sc.part[1], sc.part[2]);
    for (int k = 0; k < 3; ++k)
        if ((e = launch_scan_partials(sc.part[k], blocks, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_path_apply, dim3(blocks), block, 0, s, a, mn, rk);
    const GridDims ge = list_grid(n_ends * kPtGroup, kPtBlock);
    hipLaunchKernelGGL(k_path_emit, dim3(ge.x, ge.y, ge.z), block, 0, s, a, rk);
    return hipGetLastError();
}

}  // namespace cvs
