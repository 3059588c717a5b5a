// cvs_kernels_bridges.hip -- contour bridges (extension beyond the reference): which free chain ends face each other across a gap, and the
// digital lines that close the gaps, appended to the chain table as ordinary chains (cvs_chain_bridges), for gfx950.
//
// One lane per END in every launch but the scans and the last; include/cvsteer_hip.h has the contract.
//   1  k_bridge_arms      the arm of cvs_chain_joins, the key (plane, y, x), the cell (plane, floor(y / max_gap), floor(x / max_gap)) and the
//                         flags of every end into its BrEnd; every slot of the cell table cleared; the written totals set
//   2  k_bridge_insert    every end that may be a candidate finds or claims the slot of its cell (the open addressing of k_join_insert: an
//                         empty slot is claimed by compare-and-swap with the end's own number, and a claimed slot belongs to the cell of the
//                         end that claimed it, so all key bits count), counts itself in and pushes itself onto the cell's list
//   3  k_bridge_crowd     every end looks its nine cells up, keeps their slots, and is CROWDED if one of them holds more than 32 ends
//   4  k_bridge_best      every candidate walks the lists of its nine cells, at most 32 members each, and keeps the admissible end with the
//                         smallest (d2, end number) -- an order that does not see in which order the race left the lists
//   5  k_bridge_resolve   MUTUAL iff the partner's partner is the end; bridges and bridge points per 1024 ends
//   6  k_scan_partials x 2 (cvs_kernels_components.hip)
//   7  k_bridge_records   number and first point of every bridge (block scans on top of the partials): the records, the counts, the copy of
//                         the chain table with the junction bits of the MUTUAL ends set, the entry of every bridge that fits
//   8  k_bridge_emit      one lane per output point: the copy of the points, then every bridge point on its own from (bridge, j)
// WHAT MAKES IT SAFE ON ANY BYTES.  Chain entries are checked before they are addresses (chain_entry); everything after launch 1 reads
// positions, coordinates and arms from the scratch, which only launches of this call write.  Coordinates are never addresses: a cell is
// reached through the hash of its number.  EVERY LOOP HAS A STATIC BOUND: the arm kJoinMaxRadius terms, the probing `slots` steps (the
// table is at most half full, so an empty slot or the cell's own ends the search long before), a list walk kBridgeMaxCell steps, the
// search for a point's bridge 27 halvings, the strided copy its share of the lanes.  No lane waits for another; the atomics are integer
// (compare-and-swap, add, exchange, max) and every value they leave is the same in any order.
// Built with -ffp-contract=off: every product, sum and difference below rounds on its own; the double divisions and square roots are the
// correctly rounded ones.  No floating-point atomic.
#include <hip/hip_runtime.h>

#include "cvs_bridges.h"
#include "cvs_chain_device.h"

namespace cvs {

namespace {

constexpr int kBrBlock = 256;   // lanes per workgroup
static_assert(2ll * kBridgeMaxChains / kBrBlock <= (long long)kGridMaxX, "one workgroup per 256 ends never meets the grid bound");
static_assert(kBridgeScanBlock == 4 * kBrBlock, "a lane of the scan owns 4 consecutive ends");

struct BrEnd {
    double ax, ay, len;       // the arm: the centroid of its points relative to the end, and its length
    int32_t x, y, r;          // the key: the integer point and the plane
    int32_t cx, cy;           // the cell
    int32_t link;             // the next member of the cell's list; -1: the last
    int32_t n, flags;         // points of the arm; everything but MUTUAL after launch 3, MUTUAL after launch 5
    int32_t partner, steps;   // launch 4
    float cos, cosp;
    int32_t slot[9];          // launch 3: the slots of the nine cells around the end; -1: a cell nobody is in
    int32_t bridge;           // launch 7, at the smaller end of a MUTUAL pair
    uint32_t start;
    int32_t pos;              // the position of the end in `points`
};
static_assert(sizeof(BrEnd) == kBridgeEndBytes, "BrEnd");

struct alignas(16) BrSlot {
    int32_t rep;    // 0: empty; else 1 + the end that claimed the slot -- the slot is the cell of that end
    int32_t head;   // 0: no member yet; else 1 + the member pushed last
    int32_t cnt;    // members
    int32_t pad;
};
static_assert(sizeof(BrSlot) == kBridgeSlotBytes, "BrSlot");

struct BrScratch {
    BrEnd* ends;
    int32_t* los;       // the smaller end of bridge k
    BrSlot* slots;
    int32_t* part[2];   // bridges, bridge points
    int32_t* written;   // chain entries and points written
};
__host__ __device__ inline BrScratch br_scratch(unsigned char* base, int n_chains)
{
    BrScratch s;
    s.ends = reinterpret_cast<BrEnd*>(base);
    base += bridge_ends_bytes(n_chains);
    s.los = reinterpret_cast<int32_t*>(base);
    base += bridge_los_bytes(n_chains);
    s.slots = reinterpret_cast<BrSlot*>(base);
    base += join_slots(n_chains) * kBridgeSlotBytes;
    s.part[0] = reinterpret_cast<int32_t*>(base);
    s.part[1] = reinterpret_cast<int32_t*>(base + bridge_partials_bytes(n_chains));
    s.written = reinterpret_cast<int32_t*>(base + 2 * bridge_partials_bytes(n_chains));
    return s;
}

__device__ __forceinline__ long long br_id() { return (long long)blockIdx.x * kBrBlock + threadIdx.x; }

__device__ __forceinline__ unsigned long long br_hash(int cx, int cy, int r)
{
    unsigned long long k = ((unsigned long long)(uint32_t)cy << 32) | (uint32_t)cx;
    k ^= (unsigned long long)(uint32_t)r * 0x9E3779B97F4A7C15ull;
    k ^= k >> 33;
    k *= 0xFF51AFD7ED558CCDull;
    k ^= k >> 33;
    k *= 0xC4CEB9FE1A85EC53ull;
    k ^= k >> 33;
    return k;
}

// floor(a / b), b > 0
__device__ __forceinline__ long long br_floordiv(long long a, long long b)
{
    const long long q = a / b;
    return (a % b) < 0 ? q - 1 : q;
}

// the slot of cell (r, cy, cx) once launch 2 is through; -1: nobody is in that cell
__device__ __forceinline__ int br_find(const BrEnd* ends, long long n_ends, const BrSlot* slots, unsigned long long n_slots, int cx, int cy, int r)
{
    const unsigned long long mask = n_slots - 1;
    unsigned long long h = br_hash(cx, cy, r) & mask;
#pragma unroll 1
    for (unsigned long long step = 0; step < n_slots; ++step) {
        const int o = slots[h].rep - 1;
        if (o < 0) return -1;
        if (o < n_ends && ends[o].cx == cx && ends[o].cy == cy && ends[o].r == r) return (int)h;
        h = (h + 1) & mask;
    }
    return -1;
}

// is bridge k, whose first point is `start`, written: its chain entry and its last point inside the capacities
__device__ __forceinline__ bool br_fits(const BridgeArgs& a, uint32_t k, uint32_t start, int steps)
{
    return a.out_points && (long long)a.n_chains + (long long)k < (long long)a.cap_chains &&
           (unsigned long long)start + (unsigned long long)steps < (unsigned long long)a.cap_points;
}

// the exclusive prefix of v over the workgroup's 256 lanes in thread order, and the workgroup's sum: the block scan of the path kernels
__device__ __forceinline__ uint32_t br_block_scan(uint32_t v, uint32_t* ws, uint32_t& total)
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

// does end e start a bridge (the smaller end of a MUTUAL pair), and with how many points
__device__ __forceinline__ bool br_is_lo(const BrEnd* ends, int e, uint32_t& len)
{
    const bool lo = (ends[e].flags & kBridgeMutual) && e < ends[e].partner;
    len = lo ? (uint32_t)ends[e].steps + 1u : 0u;
    return lo;
}

}  // namespace

__global__ __launch_bounds__(kBrBlock) void k_bridge_arms(const BridgeArgs a)
{
    const long long n_ends = 2ll * a.n_chains, lanes = (long long)gridDim.x * kBrBlock;
    const long long id = br_id();
    const BrScratch sc = br_scratch(a.scratch, a.n_chains);
    // the slots: fewer than 4 per end, so at most four per lane (lanes >= n_ends)
    const long long n_slots = (long long)join_slots(a.n_chains);
    for (long long s = id; s < n_slots; s += lanes) *reinterpret_cast<int4*>(sc.slots + s) = make_int4(0, 0, 0, 0);
    if (id == 0) {
        sc.written[0] = a.n_chains;
        sc.written[1] = a.n_points;
    }
    if (id >= n_ends) return;

    BrEnd me{};
    me.link = me.partner = me.bridge = me.pos = -1;
    me.cos = me.cosp = __uint_as_float(0x7fc00000u);
    for (int k = 0; k < 9; ++k) me.slot[k] = -1;
    const int c = (int)(id >> 1);
    const bool tail = (id & 1) != 0;
    const ChainEntry e = chain_entry(a.chains, c, a.n_points);
    const int S = e.start, L = e.len, F = e.flags, R = e.plane;
    if (!e.ok()) {
        me.flags = kBridgeNone | kBridgeNoChain;
    } else if ((F & kChainClosed) || L < 2) {
        me.flags = kBridgeNone;
    } else {
        // positions j + sign k, k <= n <= L - 1, stay inside S .. S + L - 1, which lies inside `points`
        const long long j = tail ? (long long)S + L - 1 : (long long)S;
        const int sign = tail ? -1 : 1;
        const int n = min(a.radius, L - 1);
        const bool sub = a.xy != nullptr;
        const WordPair* src = reinterpret_cast<const WordPair*>(sub ? static_cast<const void*>(a.xy) : static_cast<const void*>(a.points));
        auto coords = [&](long long p, double& x, double& y) {
            const WordPair v = src[p];
            x = sub ? (double)__uint_as_float(v.x) : (double)(int)v.x;
            y = sub ? (double)__uint_as_float(v.y) : (double)(int)v.y;
        };
        double x0, y0;
        coords(j, x0, y0);
        double sx = -0.0, sy = -0.0;   // -0.0 + t == t for every t, the sign of a zero included: the sums START FROM term 1
#pragma unroll 1
        for (int k = 1; k <= n && k <= kJoinMaxRadius; ++k) {
            double x, y;
            coords(j + sign * k, x, y);
            sx = sx + (x - x0);
            sy = sy + (y - y0);
        }
        me.ax = __ddiv_rn(sx, (double)n);
        me.ay = __ddiv_rn(sy, (double)n);
        me.len = __dsqrt_rn(me.ax * me.ax + me.ay * me.ay);
        me.n = n;
        me.pos = (int32_t)j;
        me.x = a.points[2 * j];
        me.y = a.points[2 * j + 1];
        me.r = R;
        me.cx = (int32_t)br_floordiv(me.x, a.max_gap);
        me.cy = (int32_t)br_floordiv(me.y, a.max_gap);
        if (F & (tail ? kChainTailJunction : kChainHeadJunction)) me.flags |= kBridgeJunction;
        if (n < a.min_arm) me.flags |= kBridgeShort;
        if (!(me.len > 0.0) || me.len == INFINITY) me.flags |= kBridgeDegenerate;
    }
    sc.ends[id] = me;
}

__global__ __launch_bounds__(kBrBlock) void k_bridge_insert(const BridgeArgs a)
{
    const long long n_ends = 2ll * a.n_chains;
    const long long id = br_id();
    if (id >= n_ends) return;
    const BrScratch sc = br_scratch(a.scratch, a.n_chains);
    BrEnd* ends = sc.ends;
    if (ends[id].flags & kBridgeNotInCell) return;
    const int e = (int)id;
    const int cx = ends[e].cx, cy = ends[e].cy, r = ends[e].r;
    BrSlot* slots = sc.slots;
    const unsigned long long n_slots = join_slots(a.n_chains), mask = n_slots - 1;
    unsigned long long h = br_hash(cx, cy, r) & mask;
    int found = -1;
#pragma unroll 1
    for (unsigned long long step = 0; step < n_slots; ++step) {
        int* rep = &slots[h].rep;
        int cur = __hip_atomic_load(rep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(rep, 0, e + 1);   // the value before: 0 = this end has claimed the slot, else whoever did
            if (cur == 0) cur = e + 1;
        }
        const int o = cur - 1;                // an end number: only launches of this call write `rep`
        if (o >= 0 && o < n_ends && ends[o].cx == cx && ends[o].cy == cy && ends[o].r == r) {
            found = (int)h;
            break;
        }
        h = (h + 1) & mask;
    }
    if (found < 0) return;   // (never: the table is at most half full)
    BrSlot* sl = slots + found;
    atomicAdd(&sl->cnt, 1);
    ends[e].link = atomicExch(&sl->head, e + 1) - 1;
}

__global__ __launch_bounds__(kBrBlock) void k_bridge_crowd(const BridgeArgs a)
{
    const long long n_ends = 2ll * a.n_chains;
    const long long id = br_id();
    if (id >= n_ends) return;
    const BrScratch sc = br_scratch(a.scratch, a.n_chains);
    BrEnd* ends = sc.ends;
    const int flags = ends[id].flags;
    if (flags & kBridgeNone) return;
    const int cx = ends[id].cx, cy = ends[id].cy, r = ends[id].r;   // |cx|, |cy| <= 2^30: max_gap >= 2
    const unsigned long long n_slots = join_slots(a.n_chains);
    bool crowded = false;
#pragma unroll 1
    for (int k = 0; k < 9; ++k) {
        const int s = br_find(ends, n_ends, sc.slots, n_slots, cx + k % 3 - 1, cy + k / 3 - 1, r);
        ends[id].slot[k] = s;
        if (s >= 0 && sc.slots[s].cnt > kBridgeMaxCell) crowded = true;
    }
    if (crowded) ends[id].flags = flags | kBridgeCrowded;
}

__global__ __launch_bounds__(kBrBlock) void k_bridge_best(const BridgeArgs a)
{
    const long long n_ends = 2ll * a.n_chains;
    const long long id = br_id();
    if (id >= n_ends) return;
    const BrScratch sc = br_scratch(a.scratch, a.n_chains);
    BrEnd* ends = sc.ends;
    if (ends[id].flags & kBridgeNotCandidate) return;
    const int e = (int)id;
    const bool sub = a.xy != nullptr;
    const WordPair* src = reinterpret_cast<const WordPair*>(sub ? static_cast<const void*>(a.xy) : static_cast<const void*>(a.points));
    auto coords = [&](int p, double& x, double& y) {   // p: the position of an end, checked in launch 1
        const WordPair v = src[p];
        x = sub ? (double)__uint_as_float(v.x) : (double)(int)v.x;
        y = sub ? (double)__uint_as_float(v.y) : (double)(int)v.y;
    };
    const int ex = ends[e].x, ey = ends[e].y;
    const double eax = ends[e].ax, eay = ends[e].ay, el = ends[e].len;
    double ecx, ecy;
    coords(ends[e].pos, ecx, ecy);
    int best = -1, best_steps = 0;
    long long best_d2 = 0;
    float best_cos = 0.0f, best_cosp = 0.0f;
#pragma unroll 1
    for (int k = 0; k < 9; ++k) {
        const int s = ends[e].slot[k];
        if (s < 0) continue;
        int p = sc.slots[s].head - 1;
#pragma unroll 1
        for (int t = 0; t < kBridgeMaxCell && p >= 0 && p < n_ends; ++t) {   // (a cell of more members has made this end CROWDED)
            const int f = p;
            p = ends[f].link;
            if (f == e || (ends[f].flags & kBridgeNotCandidate)) continue;
            // the pair is evaluated from its smaller end number (lo) to its larger (hi): both ends see the same products
            const bool up = e < f;
            const long long dx = up ? (long long)ends[f].x - ex : (long long)ex - ends[f].x;
            const long long dy = up ? (long long)ends[f].y - ey : (long long)ey - ends[f].y;
            const long long adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
            const long long steps = adx > ady ? adx : ady;
            if (steps < 2 || steps > a.max_gap) continue;
            const long long d2 = dx * dx + dy * dy;
            double fcx, fcy;
            coords(ends[f].pos, fcx, fcy);
            const double Dx = up ? fcx - ecx : ecx - fcx, Dy = up ? fcy - ecy : ecy - fcy;
            const double dlen = __dsqrt_rn(Dx * Dx + Dy * Dy);
            if (!(dlen > 0.0) || dlen == INFINITY) continue;
            const double fax = ends[f].ax, fay = ends[f].ay, fl = ends[f].len;
            const double lax = up ? eax : fax, lay = up ? eay : fay, ll = up ? el : fl;
            const double hax = up ? fax : eax, hay = up ? fay : eay, hl = up ? fl : el;
            const float cos_lo = (float)__ddiv_rn(-(lax * Dx + lay * Dy), ll * dlen);
            const float cos_hi = (float)__ddiv_rn(hax * Dx + hay * Dy, hl * dlen);
            if (!(cos_lo >= a.min_cos && cos_hi >= a.min_cos)) continue;
            if (best < 0 || d2 < best_d2 || (d2 == best_d2 && f < best)) {
                best = f;
                best_d2 = d2;
                best_steps = (int)steps;
                best_cos = up ? cos_lo : cos_hi;
                best_cosp = up ? cos_hi : cos_lo;
            }
        }
    }
    if (best < 0) return;
    ends[e].partner = best;
    ends[e].steps = best_steps;
    ends[e].cos = best_cos;
    ends[e].cosp = best_cosp;
}

__global__ __launch_bounds__(kBrBlock) void k_bridge_resolve(const BridgeArgs a)
{
    __shared__ uint32_t ws[4];
    const BrScratch sc = br_scratch(a.scratch, a.n_chains);
    BrEnd* ends = sc.ends;
    const long long n_ends = 2ll * a.n_chains, e0 = (long long)blockIdx.x * kBridgeScanBlock + threadIdx.x * 4;
    uint32_t n = 0, len = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (e0 + k >= n_ends) continue;
        const int e = (int)(e0 + k);
        const int p = ends[e].partner;   // an end number or -1: launch 4 wrote it
        if (p < 0 || p >= n_ends || ends[p].partner != e) continue;
        ends[e].flags |= kBridgeMutual;   // (nobody reads the flags in this launch)
        if (e < p) {
            n += 1u;
            len += (uint32_t)ends[e].steps + 1u;
        }
    }
    uint32_t tn, tl;
    (void)br_block_scan(n, ws, tn);
    (void)br_block_scan(len, ws, tl);
    if (threadIdx.x == 0) {
        sc.part[0][blockIdx.x] = (int32_t)tn;
        sc.part[1][blockIdx.x] = (int32_t)tl;
    }
}

__global__ __launch_bounds__(kBrBlock) void k_bridge_records(const BridgeArgs a)
{
    __shared__ uint32_t ws[4];
    const BrScratch sc = br_scratch(a.scratch, a.n_chains);
    BrEnd* ends = sc.ends;
    const long long n_ends = 2ll * a.n_chains, e0 = (long long)blockIdx.x * kBridgeScanBlock + threadIdx.x * 4;
    bool lo[4];
    uint32_t ln[4], n = 0, len = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lo[k] = e0 + k < n_ends && br_is_lo(ends, (int)(e0 + k), ln[k]);
        if (!lo[k]) ln[k] = 0u;
        n += lo[k] ? 1u : 0u;
        len += ln[k];
    }
    uint32_t total;
    uint32_t bridge = (uint32_t)sc.part[0][blockIdx.x] + br_block_scan(n, ws, total);
    uint32_t start = (uint32_t)a.n_points + (uint32_t)sc.part[1][blockIdx.x] + br_block_scan(len, ws, total);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint32_t nb = (uint32_t)sc.part[0][gridDim.x];
        a.counts[0] = (int32_t)nb;
        a.counts[1] = (int32_t)((uint32_t)a.n_chains + nb);
        a.counts[2] = (int32_t)((uint32_t)a.n_points + (uint32_t)sc.part[1][gridDim.x]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (e0 + k >= n_ends) continue;
        const int e = (int)(e0 + k);
        const int flags = ends[e].flags, partner = ends[e].partner;
        // words 0 .. 3 and 6, 7 are the end's own; words 4, 5 (bridge, start) of BOTH ends of a MUTUAL pair are written by its smaller end
        uint32_t* r = a.table + (size_t)kBridgeWords * e;
        r[0] = (uint32_t)partner, r[1] = (uint32_t)flags, r[2] = (uint32_t)ends[e].n, r[3] = (uint32_t)ends[e].steps;
        r[6] = __float_as_uint(ends[e].cos), r[7] = __float_as_uint(ends[e].cosp);
        if (!(flags & kBridgeMutual)) r[4] = r[5] = 0xffffffffu;
        if ((e & 1) == 0 && a.out_chains) {   // the chain's entry as it is, the junction bits of its MUTUAL ends set
            const int32_t* src = a.chains + 4 * (size_t)(e >> 1);
            int32_t* dst = a.out_chains + 4 * (size_t)(e >> 1);
            const int add = ((flags & kBridgeMutual) ? kChainHeadJunction : 0) | ((ends[e + 1].flags & kBridgeMutual) ? kChainTailJunction : 0);
            dst[0] = src[0], dst[1] = src[1], dst[2] = src[2] | add, dst[3] = src[3];
        }
        if (!lo[k]) continue;
        const int steps = (int)ln[k] - 1;
        uint32_t* q = a.table + (size_t)kBridgeWords * partner;
        r[4] = q[4] = bridge, r[5] = q[5] = start;
        ends[e].bridge = (int32_t)bridge;
        ends[e].start = start;
        if (bridge < (uint32_t)a.n_chains) sc.los[bridge] = e;   // (always: a bridge takes two of the 2 n_chains ends)
        if (br_fits(a, bridge, start, steps)) {
            int32_t* dst = a.out_chains + 4 * ((size_t)a.n_chains + bridge);
            dst[0] = (int32_t)start, dst[1] = steps + 1, dst[2] = kChainHeadJunction | kChainTailJunction, dst[3] = ends[e].r;
            atomicMax(&sc.written[0], a.n_chains + (int)bridge + 1);
            atomicMax(&sc.written[1], (int)(start + (uint32_t)steps + 1u));
        }
        bridge += 1u;
        start += ln[k];
    }
}

__global__ __launch_bounds__(kBrBlock) void k_bridge_emit(const BridgeArgs a, long long lanes)
{
    const BrScratch sc = br_scratch(a.scratch, a.n_chains);
    const BrEnd* ends = sc.ends;
    const WordPair* src = reinterpret_cast<const WordPair*>(a.points);
    WordPair* dst = reinterpret_cast<WordPair*>(a.out_points);
    const WordPair* sxy = reinterpret_cast<const WordPair*>(a.xy);
    WordPair* dxy = reinterpret_cast<WordPair*>(a.out_xy);
    const int nb = min(sc.part[0][bridge_scan_blocks(a.n_chains)], a.n_chains);
    const long long n_ends = 2ll * a.n_chains;
    // lanes <= cap_points: no index below is outside out_points
    for (long long i = br_id(); i < lanes; i += (long long)gridDim.x * kBrBlock) {
        if (i < a.n_points) {
            dst[i] = src[i];
            if (sxy) dxy[i] = sxy[i];
            continue;
        }
        if (nb < 1) continue;
        // the bridge of point i: the largest k with start[k] <= i (the starts ascend from n_points)
        int lo_k = 0, hi_k = nb - 1;
#pragma unroll 1
        for (int t = 0; t < 27 && lo_k < hi_k; ++t) {   // nb <= 2^26
            const int mid = lo_k + (hi_k - lo_k + 1) / 2;
            const int m = sc.los[mid];
            if (m >= 0 && m < n_ends && (long long)ends[m].start <= i) lo_k = mid;
            else hi_k = mid - 1;
        }
        const int e = sc.los[lo_k];
        if (e < 0 || e >= n_ends) continue;   // (never: launch 7 named the smaller end of every bridge)
        const int f = ends[e].partner;
        const uint32_t start = ends[e].start;
        const int steps = ends[e].steps;
        const long long j = i - (long long)start;
        if (f < 0 || f >= n_ends || j < 0 || j > steps || steps < 1 || !br_fits(a, (uint32_t)lo_k, start, steps)) continue;
        const long long x0 = ends[e].x, y0 = ends[e].y, dx = (long long)ends[f].x - x0, dy = (long long)ends[f].y - y0;
        WordPair p;
        p.x = (uint32_t)(int32_t)(x0 + br_floordiv(2 * j * dx + steps, 2ll * steps));
        p.y = (uint32_t)(int32_t)(y0 + br_floordiv(2 * j * dy + steps, 2ll * steps));
        dst[i] = p;
        if (!sxy) continue;
        if (ends[e].pos < 0 || ends[e].pos >= a.n_points || ends[f].pos < 0 || ends[f].pos >= a.n_points) continue;   // (never)
        const WordPair c0 = sxy[ends[e].pos], c1 = sxy[ends[f].pos];
        WordPair v = j == 0 ? c0 : c1;
        if (j > 0 && j < steps) {
            const double t = __ddiv_rn((double)j, (double)steps);
            const double ax = (double)__uint_as_float(c0.x), ay = (double)__uint_as_float(c0.y);
            const double bx = (double)__uint_as_float(c1.x), by = (double)__uint_as_float(c1.y);
            v.x = __float_as_uint((float)(ax + t * (bx - ax)));
            v.y = __float_as_uint((float)(ay + t * (by - ay)));
        }
        dxy[i] = v;
    }
}

// ---------------------------------------------------------------------------------------
// the launch sequence: 8 launches, 9 with outputs
// ---------------------------------------------------------------------------------------
static bool bridges_ok(const BridgeArgs& a)
{
    const bool emit = a.out_points != nullptr;
    return a.n_chains >= 1 && a.n_chains <= kBridgeMaxChains && a.chains && a.table && a.counts && a.scratch && a.n_points >= 0 &&
           a.n_points <= (1 << 30) && (a.points || a.n_points == 0) && a.radius >= 1 && a.radius <= kJoinMaxRadius && a.min_arm >= 1 &&
           a.min_arm <= a.radius && a.max_gap >= 2 && a.max_gap <= kBridgeMaxGap && emit == (a.out_chains != nullptr) &&
           (!emit || (a.cap_points >= a.n_points && a.cap_chains >= a.n_chains)) && (a.out_xy != nullptr) == (emit && a.xy != nullptr) &&
           reinterpret_cast<uintptr_t>(a.scratch) % 16 == 0;
}

hipError_t launch_bridges(const BridgeArgs& a, hipStream_t s)
{
    if (!bridges_ok(a)) return hipErrorInvalidValue;
    const BrScratch sc = br_scratch(a.scratch, a.n_chains);
    const GridDims g = list_grid(2ll * a.n_chains, kBrBlock);
    const dim3 grid(g.x, g.y, g.z), block(kBrBlock);
    const int blocks = bridge_scan_blocks(a.n_chains);
    hipError_t e;
    hipLaunchKernelGGL(k_bridge_arms, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_bridge_insert, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_bridge_crowd, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_bridge_best, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_bridge_resolve, dim3(blocks), block, 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    for (int k = 0; k < 2; ++k)
        if ((e = launch_scan_partials(sc.part[k], blocks, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_bridge_records, dim3(blocks), block, 0, s, a);
    if (a.out_points) {
        // a lane per point that can be written: the copies, and at most kBridgeMaxGap + 1 points for each of at most n_chains bridges
        const long long most = (long long)a.n_points + (long long)(kBridgeMaxGap + 1) * a.n_chains;
        const long long lanes = most < a.cap_points ? most : a.cap_points;
        const GridDims ge = list_grid(lanes, kBrBlock);
        hipLaunchKernelGGL(k_bridge_emit, dim3(ge.x, ge.y, ge.z), block, 0, s, a, lanes);
    }
    return hipGetLastError();
}

}  // namespace cvs
