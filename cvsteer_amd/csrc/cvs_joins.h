// cvs_joins.h -- launch descriptor of the contour-join kernels (cvs_kernels_joins.hip), shared with their C-ABI layer (cvs_joins.cpp).
// The chain table and kChainClosed are those of cvs_chains.h.
// The first part -- the record's flags, the size of the scratch and the check of a HOST chain table -- needs no HIP header:
// tests/cpp/joins_host_san.cpp compiles it alone (CVS_JOINS_HOST_ONLY) under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace cvs {
// ---- contour joins (cvs_chain_joins, extension) ----
// One record per chain END: kJoinWords 4-byte words (struct cvs_chain_join; cvs_joins.cpp asserts the layout): node, degree, next, partner,
// flags, n, then the floats cos, sin.  Record 2c is the head of chain c, 2c + 1 its tail.
constexpr int kJoinWords = 8;
constexpr int kJoinMutual = 1, kJoinNone = 2, kJoinCrowded = 4, kJoinShort = 8, kJoinDegenerate = 16, kJoinNoChain = 32;   // CVS_JOIN_*
constexpr int kJoinIneligible = kJoinNone | kJoinCrowded | kJoinShort | kJoinDegenerate | kJoinNoChain;
constexpr int kJoinMaxRadius = 64, kJoinMaxDegree = 8;
constexpr int kJoinMaxChains = 1 << 26;

// Scratch of one call: per end one JnEnd (kJoinEndBytes: the arm, the key and the list link), then the hash table of the nodes -- a power
// of two of slots, at least 4 per chain = 2 per end, so that at most half of them are ever claimed -- of kJoinSlotBytes each.
constexpr size_t kJoinEndBytes = 56, kJoinSlotBytes = 16;
constexpr size_t join_slots(int n_chains)   // (constexpr: the kernels call it too)
{
    size_t s = 8;
    while (s < 4 * (size_t)n_chains) s <<= 1;
    return s;
}
constexpr size_t join_scratch_bytes(int n_chains) { return 2 * (size_t)n_chains * kJoinEndBytes + join_slots(n_chains) * kJoinSlotBytes; }

// what a HOST call is refused for: nullptr if the starts of the n_chains entries (start, length, flags, reserved) are the running sum of
// the lengths from 0 to n_points and every length is >= 1
inline const char* joins_host_table_wrong(int n_points, const int32_t* chains, int n_chains)
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

}  // namespace cvs

#ifndef CVS_JOINS_HOST_ONLY
#include "cvs_chains.h"

namespace cvs {
struct JoinArgs {
    const int32_t* points;   // n_points (x, y) pairs
    int n_points;
    const int32_t* chains;   // n_chains entries (start, length, flags, plane)
    int n_chains;
    const float* xy;         // nullptr: the integer points
    int radius, min_arm;
    float min_cos;
    uint32_t* table;         // 2 * n_chains records
    unsigned char* scratch;  // join_scratch_bytes(n_chains), aligned to 16 bytes: the JnEnd of every end, then the slots
};
// launch 1: the arm, the key and the flags of every end into scratch, and every slot cleared; launch 2: every end that exists finds or
// claims the slot of its node and links itself into the node's list; launch 3: the records
hipError_t launch_join_arms(const JoinArgs& a, hipStream_t s);
hipError_t launch_join_insert(const JoinArgs& a, hipStream_t s);
hipError_t launch_join_resolve(const JoinArgs& a, hipStream_t s);

}  // namespace cvs
#endif
