// cvs_kernels_joins.hip -- contour joins (extension beyond the reference): which chain ends meet at a node and which of them continues
// which (cvs_chain_joins), one record per chain end, for gfx950.
//
// One lane per END in all three launches; ends are few beside points (two per chain), so nothing here is tuned for bandwidth.
// k_join_arms: the lane reads its chain's entry, checks it before it is used as an address (chain_entry), adds the terms of its arm in
// ascending k -- sequential in the lane, so the arm is a function of the inputs, bit for bit -- and leaves arm, key (plane, y, x of the
// integer point) and flags in its JnEnd.  The launch also clears the hash table of the nodes, at most four slots per lane.
// k_join_insert: every end that exists looks for the slot of its node by open addressing from the hash of its key.  An empty slot is
// claimed by compare-and-swap with the end's own number, and a claimed slot belongs to the key of the end that claimed it: keys are
// compared through that end's JnEnd, so all 96 bits count and no key is ever stored twice.  The end then counts itself into the slot,
// lowers the slot's smallest end number and pushes itself onto the slot's list (atomic add, min and exchange: integers, any order gives
// the same count, the same minimum and the same SET of list members).  Which slot a node gets and in which order its list runs depend on
// the race; nothing below reads either but through order-free questions (the count, the minimum, "the smallest member above f").
// k_join_resolve: the lane visits the members of its node in ascending end number -- at most kJoinMaxDegree walks of a list of at most
// kJoinMaxDegree members, no array, no sort -- derives next and partner, finds its partner's partner the same way and stores the record.
// EVERY LOOP HAS A STATIC BOUND: the arm kJoinMaxRadius terms, the probing `slots` steps (the table is at most half full, so an empty
// slot or the node's own ends the search long before), the list walks kJoinMaxDegree steps.  No lane ever waits for another lane: a
// failed compare-and-swap returns the winner, whose key is final since launch 1, and the probe goes on.
// Built with -ffp-contract=off: every product, sum and difference below rounds on its own, as the contract in include/cvsteer_hip.h says;
// the double divisions and square roots are the correctly rounded ones.  No floating-point atomic.
#include <hip/hip_runtime.h>

#include <climits>

#include "cvs_chain_device.h"
#include "cvs_joins.h"

namespace cvs {

namespace {

constexpr int kJnBlock = 256;   // ends per workgroup
static_assert(2ll * kJoinMaxChains / kJnBlock <= (long long)kGridMaxX, "one workgroup per 256 ends never meets the grid bound");

struct JnEnd {    // what launch 1 (arm, key, n, flags) and launch 2 (slot, link) leave of one end
    double ax, ay, len;   // the arm: the centroid of its points relative to the end, and its length
    int32_t x, y, r;      // the key: the integer point and the plane
    int32_t slot;         // the slot of the node; -1: none (never on a table that is at most half full)
    int32_t link;         // the next member of the node's list; -1: the last
    int32_t n, flags;     // points of the arm; NONE, NO_CHAIN, SHORT, DEGENERATE
    int32_t pad;
};
static_assert(sizeof(JnEnd) == kJoinEndBytes, "JnEnd");

struct alignas(16) JnSlot {
    int32_t rep;    // 0: empty; else 1 + the end that claimed the slot -- the slot is the node of that end's key
    int32_t head;   // 0: no member yet; else 1 + the member pushed last
    int32_t cnt;    // members
    int32_t mn;     // the smallest member
};
static_assert(sizeof(JnSlot) == kJoinSlotBytes, "JnSlot");

__device__ __forceinline__ JnEnd* jn_ends(const JoinArgs& a) { return reinterpret_cast<JnEnd*>(a.scratch); }
__device__ __forceinline__ JnSlot* jn_slots(const JoinArgs& a) { return reinterpret_cast<JnSlot*>(a.scratch + 2 * (size_t)a.n_chains * kJoinEndBytes); }

__device__ __forceinline__ unsigned long long jn_hash(int x, int y, int r)
{
    unsigned long long k = ((unsigned long long)(uint32_t)y << 32) | (uint32_t)x;
    k ^= (unsigned long long)(uint32_t)r * 0x9E3779B97F4A7C15ull;
    k ^= k >> 33;
    k *= 0xFF51AFD7ED558CCDull;
    k ^= k >> 33;
    k *= 0xC4CEB9FE1A85EC53ull;
    k ^= k >> 33;
    return k;
}

__device__ __forceinline__ void jn_store(const JoinArgs& a, long long e, int node, int degree, int next, int partner, int flags, int n, float cs, float sn)
{
    uint32_t* r = a.table + (size_t)kJoinWords * e;
    const uint4 head = make_uint4((uint32_t)node, (uint32_t)degree, (uint32_t)next, (uint32_t)partner);
    const uint4 tail = make_uint4((uint32_t)flags, (uint32_t)n, __float_as_uint(cs), __float_as_uint(sn));
    if ((reinterpret_cast<uintptr_t>(a.table) & 15) == 0) {   // (uniform) the record as two 16-byte stores
        reinterpret_cast<uint4*>(r)[0] = head;
        reinterpret_cast<uint4*>(r)[1] = tail;
    } else {                                                  // a table aligned to 4 bytes only: words
        r[0] = head.x, r[1] = head.y, r[2] = head.z, r[3] = head.w;
        r[4] = tail.x, r[5] = tail.y, r[6] = tail.z, r[7] = tail.w;
    }
}

// the smallest member above `cur` of the list that starts at `head` (1 + end, 0: empty); -1: none.  At most kJoinMaxDegree steps, and a
// link is followed only while it is an end number.
__device__ __forceinline__ int jn_above(const JnEnd* ends, long long n_ends, int head, int cur)
{
    int best = -1;
    int p = head - 1;
#pragma unroll 1
    for (int k = 0; k < kJoinMaxDegree && p >= 0 && p < n_ends; ++k) {
        if (p > cur && (best < 0 || p < best)) best = p;
        p = ends[p].link;
    }
    return best;
}

struct JnBest {
    int partner;
    float cos, sin;
};

// the partner of the eligible end e among the members of its node (list at `head`, d <= kJoinMaxDegree members): candidates in ascending
// end number, replaced on strictly greater only
__device__ __forceinline__ JnBest jn_partner(const JnEnd* ends, long long n_ends, int head, int d, int e)
{
    const float qnan = __uint_as_float(0x7fc00000u);
    JnBest b{-1, qnan, qnan};
    const double ex = ends[e].ax, ey = ends[e].ay, el = ends[e].len;
    int cur = -1;
#pragma unroll 1
    for (int t = 0; t < kJoinMaxDegree && t < d; ++t) {
        const int f = jn_above(ends, n_ends, head, cur);
        if (f < 0) break;
        cur = f;
        if (f == e || (ends[f].flags & kJoinIneligible)) continue;
        const double fx = ends[f].ax, fy = ends[f].ay, fl = ends[f].len;
        // the pair is evaluated from its smaller end number (lo) to its larger (hi): both directions see the same products
        const bool up = e < f;
        const double lx = up ? ex : fx, ly = up ? ey : fy, ll = up ? el : fl;
        const double hx = up ? fx : ex, hy = up ? fy : ey, hl = up ? fl : el;
        const double den = ll * hl;
        const double dt = -(lx * hx + ly * hy);
        const double cr = ly * hx - lx * hy;
        const float cs = (float)__ddiv_rn(dt, den);
        float sn = (float)__ddiv_rn(cr, den);
        if (!up) sn = __uint_as_float(__float_as_uint(sn) ^ 0x80000000u);   // the other direction: the sign bit flipped, zeros included
        if (b.partner < 0 || cs > b.cos) {
            b.partner = f;
            b.cos = cs;
            b.sin = sn;
        }
    }
    return b;
}

}  // namespace

__global__ __launch_bounds__(kJnBlock) void k_join_arms(const JoinArgs a)
{
    const long long n_ends = 2ll * a.n_chains, lanes = (long long)gridDim.x * kJnBlock;
    const long long id = (long long)blockIdx.x * kJnBlock + threadIdx.x;
    // the slots: fewer than 4 per end, so at most four per lane (lanes >= n_ends)
    JnSlot* slots = jn_slots(a);
    const long long n_slots = (long long)join_slots(a.n_chains);
    for (long long s = id; s < n_slots; s += lanes) *reinterpret_cast<int4*>(slots + s) = make_int4(0, 0, 0, INT_MAX);
    if (id >= n_ends) return;

    JnEnd me{};
    me.slot = me.link = -1;
    const int c = (int)(id >> 1);
    const bool tail = (id & 1) != 0;
    const ChainEntry e = chain_entry(a.chains, c, a.n_points);
    const int S = e.start, L = e.len, F = e.flags, R = e.plane;
    if (!e.ok()) {
        me.flags = kJoinNone | kJoinNoChain;
    } else if ((F & kChainClosed) || L < 2) {
        me.flags = kJoinNone;
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
        me.x = a.points[2 * j];
        me.y = a.points[2 * j + 1];
        me.r = R;
        if (n < a.min_arm) me.flags |= kJoinShort;
        if (!(me.len > 0.0) || me.len == INFINITY) me.flags |= kJoinDegenerate;
    }
    jn_ends(a)[id] = me;
}

__global__ __launch_bounds__(kJnBlock) void k_join_insert(const JoinArgs a)
{
    const long long n_ends = 2ll * a.n_chains;
    const long long id = (long long)blockIdx.x * kJnBlock + threadIdx.x;
    if (id >= n_ends) return;
    JnEnd* ends = jn_ends(a);
    if (ends[id].flags & kJoinNone) return;
    const int e = (int)id;
    const int x = ends[e].x, y = ends[e].y, r = ends[e].r;
    JnSlot* slots = jn_slots(a);
    const unsigned long long n_slots = join_slots(a.n_chains), mask = n_slots - 1;
    unsigned long long h = jn_hash(x, y, r) & mask;
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
        if (o >= 0 && o < n_ends && ends[o].x == x && ends[o].y == y && ends[o].r == r) {
            found = (int)h;
            break;
        }
        h = (h + 1) & mask;
    }
    ends[e].slot = found;
    if (found < 0) return;
    JnSlot* sl = slots + found;
    atomicAdd(&sl->cnt, 1);
    atomicMin(&sl->mn, e);
    ends[e].link = atomicExch(&sl->head, e + 1) - 1;
}

__global__ __launch_bounds__(kJnBlock) void k_join_resolve(const JoinArgs a)
{
    const long long n_ends = 2ll * a.n_chains;
    const long long id = (long long)blockIdx.x * kJnBlock + threadIdx.x;
    if (id >= n_ends) return;
    const float qnan = __uint_as_float(0x7fc00000u);
    const JnEnd* ends = jn_ends(a);
    const int e = (int)id;
    const int flags = ends[e].flags, n = ends[e].n, slot = ends[e].slot;
    if (flags & kJoinNone) {
        jn_store(a, id, -1, 0, -1, -1, flags, 0, qnan, qnan);
        return;
    }
    if (slot < 0) {   // (no slot: not on a table at most half full) a node of its own
        jn_store(a, id, e, 1, e, -1, flags, n, qnan, qnan);
        return;
    }
    const JnSlot sl = jn_slots(a)[slot];
    const int d = sl.cnt, node = sl.mn;
    if (d > kJoinMaxDegree) {
        jn_store(a, id, node, d, -1, -1, flags | kJoinCrowded, n, qnan, qnan);
        return;
    }
    const int above = jn_above(ends, n_ends, sl.head, e);
    const int next = above >= 0 ? above : node;
    JnBest b{-1, qnan, qnan};
    int out = flags;
    if (!(flags & kJoinIneligible)) {
        b = jn_partner(ends, n_ends, sl.head, d, e);
        if (b.partner >= 0 && b.cos >= a.min_cos && jn_partner(ends, n_ends, sl.head, d, b.partner).partner == e) out |= kJoinMutual;
    }
    jn_store(a, id, node, d, next, b.partner, out, n, b.cos, b.sin);
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
static bool joins_ok(const JoinArgs& a)
{
    return a.n_chains >= 1 && a.n_chains <= kJoinMaxChains && a.chains && a.table && a.scratch && a.n_points >= 0 && a.n_points <= (1 << 30) &&
           (a.points || a.n_points == 0) && a.radius >= 1 && a.radius <= kJoinMaxRadius && a.min_arm >= 1 && a.min_arm <= a.radius &&
           reinterpret_cast<uintptr_t>(a.scratch) % 16 == 0;
}

// all three: one lane per end, the same grid
static hipError_t join_launch(void (*kernel)(const JoinArgs), const JoinArgs& a, hipStream_t s)
{
    if (!joins_ok(a)) return hipErrorInvalidValue;
    const GridDims g = list_grid(2ll * a.n_chains, kJnBlock);
    hipLaunchKernelGGL(kernel, dim3(g.x, g.y, g.z), dim3(kJnBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_join_arms(const JoinArgs& a, hipStream_t s) { return join_launch(k_join_arms, a, s); }
hipError_t launch_join_insert(const JoinArgs& a, hipStream_t s) { return join_launch(k_join_insert, a, s); }
hipError_t launch_join_resolve(const JoinArgs& a, hipStream_t s) { return join_launch(k_join_resolve, a, s); }

}  // namespace cvs
