// cvs_refine.h -- launch descriptors of the contour-edgel kernels (cvs_kernels_refine.hip), shared with their C-ABI layer (cvs_refine.cpp).
// kChainClosed is that of cvs_chains.h, the wave / workgroup split of the chain table that of cvs_polyline.h (kPlWaveMax, kPlMaxGrid).
#pragma once
#include "cvs_polyline.h"

namespace cvs {
// ---- sub-pixel chain points (cvs_chain_refine, extension) ----
// One lane per point.  A point whose coordinates do not lie inside rows x cols stores NaN and reads no plane; `strength` may be null.
struct RefineArgs {
    int rows, cols;
    PlaneRef map, theta;     // f32 planes of rows x cols, pitch in elements
    const int32_t* points;   // n_points (x, y) pairs
    int n_points;
    float* xy;               // n_points (xs, ys) pairs
    float* strength;         // nullptr, or n_points floats
};
hipError_t launch_chain_refine(const RefineArgs& a, hipStream_t s);

// ---- per-chain measures (cvs_chain_measures, extension) ----
// A chain table as in cvs_polyline.h: four int32 per chain, an entry that does not lie inside `points` is an EMPTY chain (an all-zero record
// with peak_index -1).  A record is kMeasureWords 4-byte words (struct cvs_chain_measure; cvs_refine.cpp asserts the layout): axial,
// diagonal, other, peak_index, peak, weakest, then the two doubles sum and length as low / high words.
constexpr int kMeasureWords = 10;
struct MeasureArgs {
    const int32_t* points;   // n_points (x, y) pairs
    int n_points;
    const int32_t* chains;
    int n_chains;
    const float* xy;         // nullptr: lengths from the integer points
    const float* strength;   // nullptr: no peak, no sum
    uint32_t* table;         // n_chains records
};
// _wave: one wave per chain of at most kPlWaveMax points (and the record of every empty chain); _block: a bounded grid of 256-lane
// workgroups strides over the table and takes the longer chains.  Both are launched for every table.
hipError_t launch_measure_wave(const MeasureArgs& a, hipStream_t s);
hipError_t launch_measure_block(const MeasureArgs& a, hipStream_t s);

}  // namespace cvs
