// cvs_kernels_turns.hip -- contour turns (extension beyond the reference): the turn of the contour at every chain point and the corners of
// every chain (cvs_chain_turns), one record per point, for gfx950.
//
// k_turns: one lane per point.  The lane finds its chain by binary search, adds the terms of its two arms in ascending k -- all of a
// point's arithmetic is sequential in its lane, so the record is a function of the inputs, bit for bit -- and stores the record without
// its CORNER bit.  Adjacent lanes read windows that overlap in all but one point, so a workgroup first stages its 256 points and `radius`
// more on either side in LDS (8 bytes per point as they lie in memory, integer pairs or float pairs; at most 3 KiB); an arm point is read
// from global memory only where it lies outside that window, which happens where a closed chain wraps.  The arithmetic is double (the
// contract's): per point 4 nb + 4 nf additions, four divisions, two square roots and two more divisions -- the fp64 vector rate of
// gfx950 is half the fp32 rate, and the kernel stays bound by its 32 bytes of record per 8 bytes of point.
// k_turn_nms: one lane per point; only a point that is eligible and turns sharply enough (cos <= max_cos) walks its window.
// k_turn_summary: one wave per chain of at most kPlWaveMax points, one 256-lane workgroup per longer chain (ms_long_entries, shared with
// the measures and the segments), integers and (cos, position) pairs combined by butterfly.
// What the table says is checked before it is used as an address (chain_entry); coordinates are never addresses.  No atomic, no scratch,
// nothing read back.
// Built with -ffp-contract=off: every product, sum and difference below rounds on its own, as the contract in include/cvsteer_hip.h says;
// the double divisions and square roots are the correctly rounded ones.
#include <hip/hip_runtime.h>

#include "cvs_chain_device.h"
#include "cvs_turns.h"

namespace cvs {

namespace {

constexpr int kTnBlock = 256;                              // points per workgroup of k_turns and k_turn_nms
constexpr int kTnTile = kTnBlock + 2 * kTurnMaxRadius;     // staged points: the workgroup's own and the halo of the largest radius
constexpr int kTnNone = 0x7fffffff;                        // "no eligible point yet" in a (cos, position) pair
static_assert((1ll << 30) / kTnBlock <= (long long)kGridMaxX, "k_turns and k_turn_nms: one workgroup per 256 points never meets the grid bound");

struct alignas(8) TnStaged {   // a point (a WordPair: the bits of an (x, y) pair of `points` or of an (xs, ys) pair of `xy`) in LDS
    uint32_t x, y;
};

__device__ __forceinline__ void tn_store(const TurnArgs& a, long long i, int chain, int flags, int nb, int nf, float sn, float cs, float lb, float lf)
{
    uint32_t* r = a.table + (size_t)kTurnWords * i;
    const uint4 head = make_uint4((uint32_t)chain, (uint32_t)flags, (uint32_t)nb, (uint32_t)nf);
    const uint4 tail = make_uint4(__float_as_uint(sn), __float_as_uint(cs), __float_as_uint(lb), __float_as_uint(lf));
    if ((reinterpret_cast<uintptr_t>(a.table) & 15) == 0) {   // (uniform) the record as two 16-byte stores
        reinterpret_cast<uint4*>(r)[0] = head;
        reinterpret_cast<uint4*>(r)[1] = tail;
    } else {                                                  // a table aligned to 4 bytes only: words
        r[0] = head.x, r[1] = head.y, r[2] = head.z, r[3] = head.w;
        r[4] = tail.x, r[5] = tail.y, r[6] = tail.z, r[7] = tail.w;
    }
}

struct TnSum {   // what k_turn_summary reduces
    int corners, eligible, idx;
    float cos;
};

// record p into the sums of chain c; a lane visits its positions in ascending order, so the strict comparison keeps the first on ties
__device__ __forceinline__ void tn_take(TnSum& s, const TurnArgs& a, long long p, int c)
{
    const uint32_t* r = a.table + (size_t)kTurnWords * p;
    if ((int)r[0] != c) return;
    const int fl = (int)r[1];
    s.corners += fl & kTurnCorner;
    if (fl & kTurnIneligible) return;
    ++s.eligible;
    const float v = __uint_as_float(r[5]);
    if (s.idx == kTnNone || v < s.cos) {
        s.cos = v;
        s.idx = (int)p;
    }
}

__device__ __forceinline__ void tn_merge(TnSum& s, const TnSum& o)
{
    s.corners += o.corners;
    s.eligible += o.eligible;
    if (o.idx != kTnNone && (s.idx == kTnNone || o.cos < s.cos || (o.cos == s.cos && o.idx < s.idx))) {
        s.cos = o.cos;
        s.idx = o.idx;
    }
}

// butterfly over the wave: every lane ends with the same sums (integer sums and a minimum under a total order: any order gives them)
__device__ __forceinline__ void tn_wave(TnSum& s)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        TnSum o;
        o.corners = __shfl_xor(s.corners, d, 64);
        o.eligible = __shfl_xor(s.eligible, d, 64);
        o.idx = __shfl_xor(s.idx, d, 64);
        o.cos = __shfl_xor(s.cos, d, 64);
        tn_merge(s, o);
    }
}

__device__ __forceinline__ void tn_store_summary(const TurnArgs& a, long long c, const TnSum& s)
{
    uint32_t* r = a.summary + (size_t)kTurnSummaryWords * c;
    r[0] = (uint32_t)s.corners;
    r[1] = (uint32_t)s.eligible;
    r[2] = (uint32_t)(s.idx == kTnNone ? -1 : s.idx);
    r[3] = __float_as_uint(s.idx == kTnNone ? INFINITY : s.cos);
}

}  // namespace

__global__ __launch_bounds__(kTnBlock) void k_turns(const TurnArgs a)
{
    __shared__ TnStaged tile[kTnTile];
    const int tid = threadIdx.x;
    const long long n = a.n_points, base = (long long)blockIdx.x * kTnBlock;
    const WordPair* src = reinterpret_cast<const WordPair*>(a.xy ? static_cast<const void*>(a.xy) : static_cast<const void*>(a.points));
    const bool sub = a.xy != nullptr;
    // the window [lo, hi) of `points` this workgroup stages: hi - lo <= kTnBlock + 2 radius <= kTnTile
    const long long lo = base - a.radius < 0 ? 0 : base - a.radius;
    const long long hi = base + kTnBlock + a.radius > n ? n : base + kTnBlock + a.radius;
    for (long long p = lo + tid; p < hi; p += kTnBlock) {
        const WordPair v = src[p];
        tile[p - lo].x = v.x;
        tile[p - lo].y = v.y;
    }
    __syncthreads();
    const long long i = base + tid;
    if (i >= n) return;

    const float qnan = __uint_as_float(0x7fc00000u);
    const int c = entry_of(a.chains, a.n_chains, i);
    const ChainEntry e = chain_entry(a.chains, c, a.n_points);
    const int S = e.start, L = e.len, F = e.flags;
    if (!e.ok() || i < S || i >= (long long)S + L) {   // a point of a broken entry, or of none
        tn_store(a, i, -1, kTurnNoChain, 0, 0, qnan, qnan, 0.0f, 0.0f);
        return;
    }
    auto coords = [&](long long p, double& x, double& y) {   // S <= p < S + L <= n_points
        WordPair v;
        if (p >= lo && p < hi) {
            const TnStaged t = tile[p - lo];
            v.x = t.x;
            v.y = t.y;
        } else {
            v = src[p];
        }
        x = sub ? (double)__uint_as_float(v.x) : (double)(int)v.x;
        y = sub ? (double)__uint_as_float(v.y) : (double)(int)v.y;
    };
    const int j = (int)(i - S);
    const bool closed = (F & kChainClosed) != 0;
    int nb, nf;
    if (closed) {
        nb = nf = min(a.radius, (L - 1) / 2);
    } else {
        nb = min(a.radius, j);
        nf = min(a.radius, L - 1 - j);
    }
    double x0, y0;
    coords(i, x0, y0);
    // -0.0 + t == t for every t, the sign of a zero included: the sums START FROM term 1, as the contract says
    double sbx = -0.0, sby = -0.0, sfx = -0.0, sfy = -0.0;
    for (int k = 1; k <= nb; ++k) {
        int jb = j - k;
        if (jb < 0) jb += L;   // closed chains only (k <= nb <= j on an open one); k <= (L - 1) / 2: one turn at most
        double x, y;
        coords((long long)S + jb, x, y);
        sbx = sbx + (x - x0);
        sby = sby + (y - y0);
    }
    for (int k = 1; k <= nf; ++k) {
        int jf = j + k;
        if (jf >= L) jf -= L;
        double x, y;
        coords((long long)S + jf, x, y);
        sfx = sfx + (x - x0);
        sfy = sfy + (y - y0);
    }
    int flags = 0;
    if (nb == 0 || nf == 0) flags |= kTurnEnd;
    if (nb < a.min_arm || nf < a.min_arm) flags |= kTurnShort;
    double abx = 0.0, aby = 0.0, afx = 0.0, afy = 0.0, la = 0.0, lf = 0.0;
    if (nb > 0) {
        abx = __ddiv_rn(sbx, (double)nb);
        aby = __ddiv_rn(sby, (double)nb);
        la = __dsqrt_rn(abx * abx + aby * aby);
    }
    if (nf > 0) {
        afx = __ddiv_rn(sfx, (double)nf);
        afy = __ddiv_rn(sfy, (double)nf);
        lf = __dsqrt_rn(afx * afx + afy * afy);
    }
    float sn = qnan, cs = qnan;
    if (!(flags & kTurnEnd)) {
        const double dinx = -abx, diny = -aby;
        const double cr = dinx * afy - diny * afx, dt = dinx * afx + diny * afy, den = la * lf;
        if (!(den > 0.0) || den == INFINITY) {
            flags |= kTurnDegenerate;
        } else {
            sn = (float)__ddiv_rn(cr, den);
            cs = (float)__ddiv_rn(dt, den);
        }
    }
    float lb32 = (float)la, lf32 = (float)lf;
    if (lb32 != lb32) lb32 = qnan;   // a NaN from xy: every NaN the call stores is this one
    if (lf32 != lf32) lf32 = qnan;
    tn_store(a, i, c, flags, nb, nf, sn, cs, lb32, lf32);
}

// The CORNER bits.  No race: a lane writes nothing but bit 0 of the flags word of its OWN record, as one aligned 32-bit store, and reads of
// other records only their cos and the END / DEGENERATE / SHORT / NO_CHAIN bits of their flags -- all of them final since launch 1, which
// this launch follows on the stream; whether a neighbour's word is seen before or after its owner set bit 0 changes none of the bits read.
__global__ __launch_bounds__(kTnBlock) void k_turn_nms(const TurnArgs a)
{
    const long long i = (long long)blockIdx.x * kTnBlock + threadIdx.x;
    if (i >= a.n_points) return;
    uint32_t* r = a.table + (size_t)kTurnWords * i;
    const int c = (int)r[0], flags = (int)r[1];
    if (flags & kTurnIneligible) return;
    const float ci = __uint_as_float(r[5]);
    if (!(ci <= a.max_cos)) return;
    if (c < 0 || c >= a.n_chains) return;   // (launch 1 has checked this, and what follows)
    const ChainEntry e = chain_entry(a.chains, c, a.n_points);
    const int S = e.start, L = e.len;
    if (!e.ok() || i < S || i >= (long long)S + L) return;
    const int j = (int)(i - S);
    const bool closed = (e.flags & kChainClosed) != 0;
    const int reach = closed ? min(a.nms, (L - 1) / 2) : a.nms;
    for (int k = 1; k <= reach; ++k) {
        int jb = j - k, jf = j + k;
        bool has_b = true, has_f = true;
        if (jb < 0) {
            if (closed) jb += L;
            else has_b = false;
        }
        if (jf >= L) {
            if (closed) jf -= L;
            else has_f = false;
        }
        if (has_b) {
            const uint32_t* q = a.table + (size_t)kTurnWords * ((long long)S + jb);
            if (!((int)q[1] & kTurnIneligible) && !(ci < __uint_as_float(q[5]))) return;    // strict backwards
        }
        if (has_f) {
            const uint32_t* q = a.table + (size_t)kTurnWords * ((long long)S + jf);
            if (!((int)q[1] & kTurnIneligible) && !(ci <= __uint_as_float(q[5]))) return;
        }
        if (!has_b && !has_f) break;
    }
    r[1] = (uint32_t)(flags | kTurnCorner);
}

__global__ __launch_bounds__(256) void k_turn_summary(const TurnArgs a)
{
    __shared__ unsigned long long lm[4];
    __shared__ TnSum part[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // one wave per chain of at most kPlWaveMax points, and the summary of every entry that does not lie inside `points`
    for (long long c = (long long)blockIdx.x * 4 + wave; c < a.n_chains; c += (long long)gridDim.x * 4) {
        const ChainEntry e = chain_entry(a.chains, (int)c, a.n_points);
        const bool ok = e.ok();
        if (ok && e.len > kPlWaveMax) continue;   // a workgroup's, below
        TnSum s{0, 0, kTnNone, 0.0f};
        if (ok)
            for (int j = lane; j < e.len; j += 64) tn_take(s, a, (long long)e.start + j, (int)c);
        tn_wave(s);
        if (lane == 0) tn_store_summary(a, c, s);
    }
    ms_long_entries(
        a.n_chains, lm,
        [&](long long c) {
            const ChainEntry e = chain_entry(a.chains, (int)c, a.n_points);
            return e.ok() && e.len > kPlWaveMax;
        },
        [&](long long c) {
            const ChainEntry e = chain_entry(a.chains, (int)c, a.n_points);
            TnSum s{0, 0, kTnNone, 0.0f};
            for (int j = tid; j < e.len; j += 256) tn_take(s, a, (long long)e.start + j, (int)c);
            tn_wave(s);
            __syncthreads();   // `part` is free again: the chain before has been read to its end
            if (lane == 0) part[wave] = s;
            __syncthreads();
            if (tid == 0) {
                tn_merge(s, part[1]);
                tn_merge(s, part[2]);
                tn_merge(s, part[3]);
                tn_store_summary(a, c, s);
            }
        });
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
static bool turns_ok(const TurnArgs& a)
{
    return a.n_points >= 1 && a.n_points <= (1 << 30) && a.points && a.n_chains >= 1 && a.chains && a.table && a.radius >= 1 &&
           a.radius <= kTurnMaxRadius && a.min_arm >= 1 && a.min_arm <= a.radius && a.nms >= 0 && a.nms <= kTurnMaxNms;
}

hipError_t launch_turns(const TurnArgs& a, hipStream_t s)
{
    if (!turns_ok(a)) return hipErrorInvalidValue;
    const GridDims g = list_grid(a.n_points, kTnBlock);
    hipLaunchKernelGGL(k_turns, dim3(g.x, g.y, g.z), dim3(kTnBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_turn_nms(const TurnArgs& a, hipStream_t s)
{
    if (!turns_ok(a)) return hipErrorInvalidValue;
    const GridDims g = list_grid(a.n_points, kTnBlock);
    hipLaunchKernelGGL(k_turn_nms, dim3(g.x, g.y, g.z), dim3(kTnBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_turn_summary(const TurnArgs& a, hipStream_t s)
{
    if (!turns_ok(a) || !a.summary) return hipErrorInvalidValue;
    const GridDims g = list_grid(a.n_chains, 4);   // four waves, four chains per workgroup; the kernel strides where the bound holds the grid
    hipLaunchKernelGGL(k_turn_summary, dim3(g.x, g.y, g.z), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace cvs
