// cvs_turns.h -- launch descriptor of the contour-turn kernels (cvs_kernels_turns.hip), shared with their C-ABI layer (cvs_turns.cpp).
// The chain table and kChainClosed are those of cvs_chains.h, the wave / workgroup split of the summary (kPlWaveMax, kPlMaxGrid) that of
// cvs_polyline.h; the check of a HOST chain table is chain_table_not_running_sum (cvs_chain_table.h).
#pragma once
#include "cvs_refine.h"

namespace cvs {
// ---- contour turns (cvs_chain_turns, extension) ----
// One record per point: kTurnWords 4-byte words (struct cvs_chain_turn; cvs_turns.cpp asserts the layout): chain, flags, nb, nf, then the
// floats sin, cos, lb, lf.  One summary per chain: kTurnSummaryWords words (corners, eligible, sharpest, min_cos).
constexpr int kTurnWords = 8, kTurnSummaryWords = 4;
constexpr int kTurnCorner = 1, kTurnEnd = 2, kTurnDegenerate = 4, kTurnShort = 8, kTurnNoChain = 16;   // CVS_TURN_*
constexpr int kTurnIneligible = kTurnEnd | kTurnDegenerate | kTurnShort | kTurnNoChain;
constexpr int kTurnMaxRadius = 64, kTurnMaxNms = 64;

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
