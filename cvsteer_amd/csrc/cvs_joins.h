// cvs_joins.h -- launch descriptor of the contour-join kernels (cvs_kernels_joins.hip), shared with their C-ABI layer (cvs_joins.cpp).
// The chain table and kChainClosed are those of cvs_chains.h; the size of the scratch (join_slots, join_scratch_bytes) and the check of a
// HOST chain table (chain_table_not_running_sum) are those of cvs_chain_table.h.
#pragma once
#include "cvs_chain_table.h"
#include "cvs_chains.h"

namespace cvs {
// ---- contour joins (cvs_chain_joins, extension) ----
// One record per chain END: kJoinWords 4-byte words (struct cvs_chain_join; cvs_joins.cpp asserts the layout): node, degree, next, partner,
// flags, n, then the floats cos, sin.  Record 2c is the head of chain c, 2c + 1 its tail.
constexpr int kJoinWords = 8;
constexpr int kJoinMutual = 1, kJoinNone = 2, kJoinCrowded = 4, kJoinShort = 8, kJoinDegenerate = 16, kJoinNoChain = 32;   // CVS_JOIN_*
constexpr int kJoinIneligible = kJoinNone | kJoinCrowded | kJoinShort | kJoinDegenerate | kJoinNoChain;
constexpr int kJoinMaxRadius = 64, kJoinMaxDegree = 8;
constexpr int kJoinMaxChains = 1 << 26;

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
