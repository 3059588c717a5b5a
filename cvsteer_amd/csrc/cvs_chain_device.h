// cvs_chain_device.h -- how the kernels of the contour tail read the arrays of a chain call (cvs_kernels_polyline.hip, _refine, _segments,
// _turns, _joins, _bridges, and the point pairs of cvs_kernels_chains_batch.hip): the 8-byte point pair, the entry of a chain table with the test that
// it lies inside `points`, the search for the entry a position belongs to, and the loop of the workgroup kernels over the long entries.
// Only the reading and the test are shared: what a kernel stores for a broken entry -- an empty record, NO_CHAIN, a chain of no points --
// is its own.  Everything is __forceinline__ and returns by value, so a field a kernel does not use (the plane word, mostly) is never loaded.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
namespace cvs {

// two 4-byte words that travel as one 8-byte access (the arrays are aligned to 4 bytes, which a global dwordx2 access allows)
template <class T>
struct Pair {
    T x, y;
};
typedef Pair<int> IntPair;         // an (x, y) pair of `points`
typedef Pair<float> FloatPair;     // an (xs, ys) pair of `xy`
typedef Pair<uint32_t> WordPair;   // the bits of either

// entry c of a chain table (start, length, flags, plane), and whether it lies inside the n_points points: nothing but an entry that is
// `ok` may become an address
// (the test is a macro, not one more inline function: a level of inlining more or less changes the order in which the optimiser meets it,
// and with that the instruction stream of kernels this header is meant to leave as they were)
#define CVS_INSIDE_POINTS(start, len, n_points) ((start) >= 0 && (len) >= 1 && (long long)(start) + (len) <= (long long)(n_points))
struct ChainEntry {
    int start, len, flags, plane, n_points;
    __device__ __forceinline__ bool ok() const { return CVS_INSIDE_POINTS(start, len, n_points); }
};
__device__ __forceinline__ ChainEntry chain_entry(const int32_t* chains, long long c, int n_points)
{
    const int32_t* e = chains + 4 * c;
    return ChainEntry{e[0], e[1], e[2], e[3], n_points};
}
// the same for the kernels to which a broken entry is a chain of no points: start = len = 0
__device__ __forceinline__ ChainEntry chain_or_empty(const int32_t* chains, long long c, int n_points)
{
    const int32_t* e = chains + 4 * c;
    const int s = e[0], l = e[1];
    const bool ok = CVS_INSIDE_POINTS(s, l, n_points);
    return ChainEntry{ok ? s : 0, ok ? l : 0, e[2], e[3], n_points};
}

// the largest c with table[c].start <= i where the starts ascend; never outside 0 .. n - 1, whatever the table holds
__device__ __forceinline__ int entry_of(const int32_t* table, int n, long long i)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;   // lo < mid <= hi
        if ((long long)table[4 * (size_t)mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the long entries of a table of n entries, for the _block kernels: a 256-lane workgroup takes slices of 256 entries (slice = blockIdx.x,
// + gridDim.x, ...), ballots is_long(entry) and calls f(entry) for each entry that is, all 256 lanes together.  lm: four words of LDS.
template <class P, class F>
__device__ __forceinline__ void ms_long_entries(long long n, unsigned long long* lm, P is_long, F f)
{
    for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
        const long long c = base + threadIdx.x;
        const unsigned long long b = __ballot(c < n && is_long(c));
        if ((threadIdx.x & 63) == 0) lm[threadIdx.x >> 6] = b;
        __syncthreads();
#pragma unroll 1
        for (int w = 0; w < 4; ++w) {
            unsigned long long bits = lm[w];
            while (bits) {
                const int k = __ffsll((long long)bits) - 1;
                bits &= bits - 1;
                f(base + w * 64 + k);
            }
        }
        __syncthreads();   // lm is written again
    }
}
// the long chains of a chain table: f(chain index, chain) for each chain of more than `wave_max` points
template <class F>
__device__ __forceinline__ void long_chains(const int32_t* chains, int n_chains, int n_points, int wave_max, unsigned long long* lm, F f)
{
    ms_long_entries(
        n_chains, lm, [&](long long c) { return chain_or_empty(chains, c, n_points).len > wave_max; },
        [&](long long c) { f(c, chain_or_empty(chains, c, n_points)); });
}

}  // namespace cvs
#endif
