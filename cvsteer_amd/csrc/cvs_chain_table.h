// cvs_chain_table.h -- what a HOST chain table is refused for, for every call of the contour tail that takes one (cvs_polyline.cpp,
// cvs_refine.cpp, cvs_segments.cpp, cvs_turns.cpp, cvs_joins.cpp, cvs_paths.cpp, cvs_bridges.cpp), and the size of the join scratch, which cvs_joins.cpp and the join
// kernels both compute.  A table is n_chains entries of four int32 words (start, length, flags, plane: struct cvs_chain).
// No HIP header and no other header of the engine: tests/cpp/chain_table_san.cpp compiles this file alone under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace cvs {

// the inside-points rule (polylines, measures, segments): every entry has a start >= 0, a length >= 1 and ends inside the n_points points
// (what entry c, and what the table, is refused for: nullptr if nothing)
inline const char* chain_entry_outside(int n_points, const int32_t* chains, size_t c)
{
    const int32_t start = chains[4 * c], length = chains[4 * c + 1];
    return start < 0 || length < 1 || (long long)start + length > n_points ? "a chain does not lie inside points" : nullptr;
}
inline const char* chain_table_outside(int n_points, const int32_t* chains, int n_chains)
{
    const char* what = nullptr;
    for (int c = 0; c < n_chains && !what; ++c) what = chain_entry_outside(n_points, chains, (size_t)c);
    return what;
}

// the running-sum rule (turns, joins, paths, bridges): the starts are the running sum of the lengths from 0 to n_points and every length is >= 1
inline const char* chain_table_not_running_sum(int n_points, const int32_t* chains, int n_chains)
{
    long long at = 0;
    for (int c = 0; c < n_chains; ++c) {
        const int32_t start = chains[4 * (size_t)c], length = chains[4 * (size_t)c + 1];
        if (length < 1) return "a chain has no point";
        if (start != at) return "the chain starts are not the running sum of the lengths";
        at += length;
        if (at > n_points) return "the chains hold more points than n_points";
    }
    return at == n_points ? nullptr : "the chain lengths do not add up to n_points";
}

// Scratch of one cvs_chain_joins call: per end one JnEnd (kJoinEndBytes: the arm, the key and the list link), then the hash table of the
// nodes -- a power of two of slots, at least 4 per chain = 2 per end, so that at most half of them are ever claimed -- of kJoinSlotBytes each.
constexpr size_t kJoinEndBytes = 56, kJoinSlotBytes = 16;
constexpr size_t join_slots(int n_chains)   // (constexpr: the kernels call it too)
{
    size_t s = 8;
    while (s < 4 * (size_t)n_chains) s <<= 1;
    return s;
}
constexpr size_t join_scratch_bytes(int n_chains) { return 2 * (size_t)n_chains * kJoinEndBytes + join_slots(n_chains) * kJoinSlotBytes; }

}  // namespace cvs
