// cvs_turns.h -- launch descriptor of the contour-turn kernels (cvs_kernels_turns.hip), shared with their C-ABI layer (cvs_turns.cpp).
// The chain table and kChainClosed are those of cvs_chains.h, the wave / workgroup split of the summary (kPlWaveMax, kPlMaxGrid) and the
// search for long entries (ms_long_entries) those of cvs_refine.h.
// The first part -- the record's flags and the check of a HOST chain table -- needs no HIP header: tests/cpp/turns_host_san.cpp compiles it
// alone (CVS_TURNS_HOST_ONLY) under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace cvs {
// ---- contour turns (cvs_chain_turns, extension) ----
// One record per point: kTurnWords 4-byte words (struct cvs_chain_turn; cvs_turns.cpp asserts the layout): chain, flags, nb, nf, then the
// floats sin, cos, lb, lf.  One summary per chain: kTurnSummaryWords words (corners, eligible, sharpest, min_cos).
constexpr int kTurnWords = 8, kTurnSummaryWords = 4;
constexpr int kTurnCorner = 1, kTurnEnd = 2, kTurnDegenerate = 4, kTurnShort = 8, kTurnNoChain = 16;   // CVS_TURN_*
constexpr int kTurnIneligible = kTurnEnd | kTurnDegenerate | kTurnShort | kTurnNoChain;
constexpr int kTurnMaxRadius = 64, kTurnMaxNms = 64;

// what a HOST call is refused for: nullptr if the starts of the n_chains entries (start, length, flags, reserved) are the running sum of
// the lengths from 0 to n_points and every length is >= 1
inline const char* turns_host_table_wrong(int n_points, const int32_t* chains, int n_chains)
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

#ifndef CVS_TURNS_HOST_ONLY
#include "cvs_refine.h"

namespace cvs {
struct TurnArgs {
    const int32_t* points;   // n_points (x, y) pairs
    int n_points;
    const int32_t* chains;   // n_chains entries (start, length, flags, reserved)
    int n_chains;
    const float* xy;         // nullptr: the integer points
    int radius, min_arm, nms;
    float max_cos;
    uint32_t* table;         // n_points records
    uint32_t* summary;       // nullptr, or n_chains records
};
// launch 1: the record of every point but its CORNER bit; launch 2: the CORNER bits, from the cos and flags launch 1 left; launch 3
// (summary != nullptr): one wave per chain of at most kPlWaveMax points, one 256-lane workgroup per longer chain, in one grid
hipError_t launch_turns(const TurnArgs& a, hipStream_t s);
hipError_t launch_turn_nms(const TurnArgs& a, hipStream_t s);
hipError_t launch_turn_summary(const TurnArgs& a, hipStream_t s);

}  // namespace cvs
#endif
