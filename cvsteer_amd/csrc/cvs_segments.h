// cvs_segments.h -- launch descriptor of the contour-segment kernels (cvs_kernels_segments.hip), shared with their C-ABI layer
// (cvs_segments.cpp).  The chain table and kChainClosed are those of cvs_chains.h, the polyline table and the index those of cvs_polyline.h,
// the wave / workgroup split (kPlWaveMax, kPlMaxGrid) that of cvs_polyline.h.
#pragma once
#include "cvs_refine.h"

namespace cvs {
// ---- line fits of polyline spans (cvs_polyline_segments, extension) ----
// One record per vertex: kSegmentWords 4-byte words (struct cvs_segment; cvs_segments.cpp asserts the layout): first, count, chain, flags,
// then fourteen doubles as low / high words.  A vertex without a span -- the last vertex of an open polyline, and every vertex whose table
// entries do not pass the checks of sg_span -- has count 0 and zeros behind `chain`.
constexpr int kSegmentWords = 32;
constexpr int kSegWraps = 1, kSegDegenerate = 2;
struct SegmentArgs {
    const int32_t* points;      // n_points (x, y) pairs
    int n_points;
    const int32_t* chains;      // n_chains entries (start, length, flags, reserved)
    const int32_t* polylines;   // n_chains entries (first vertex, vertices, flags, reserved)
    int n_chains;
    const int32_t* index;       // n_vertices positions in `points`
    int n_vertices;
    const float* xy;            // nullptr: the integer points are fitted
    const float* strength;      // nullptr: unit weights
    uint32_t* table;            // n_vertices records
};
// _wave: one group of 16 lanes -- four to a wave -- per vertex whose span has at most kPlWaveMax points (and the record of every vertex
// without a span); _block: a bounded grid of 256-lane workgroups strides over the vertices and takes the longer spans.  Both are launched
// for every table.
hipError_t launch_segments_wave(const SegmentArgs& a, hipStream_t s);
hipError_t launch_segments_block(const SegmentArgs& a, hipStream_t s);

}  // namespace cvs
