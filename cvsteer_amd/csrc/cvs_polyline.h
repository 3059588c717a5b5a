// cvs_polyline.h -- launch descriptors of the contour-polyline kernels (cvs_kernels_polyline.hip), shared with their C-ABI layer
// (cvs_polyline.cpp).  kChainClosed is that of cvs_chains.h; the scan over the per-chain counts goes through launch_scan_partials of
// cvs_components.h as it is.
#pragma once
#include "cvs_chains.h"

namespace cvs {
// ---- contour polylines (cvs_chain_polylines, extension) ----
// A chain table is what cvs_contour_chains writes: four int32 per chain (start, length, flags, 0), chain c = points[start .. start + length).
// An entry with start < 0, length < 1 or start + length > n_points is an EMPTY chain to every kernel here: nothing of it is read or written.
// KEEP: one byte per point, 1 = the point is a vertex of its chain's polyline.  COUNT: one int per chain, first the number of kept points,
// after k_pl_apply the chain's first vertex.
constexpr int kPlWaveMax = 256;      // chains of at most this many points are simplified by one wave, longer ones by one workgroup
constexpr int kPlWaveWords = kPlWaveMax / 64;   // ... whose keep flags are this many 64-bit words held by the wave
constexpr int kPlScanBlock = 1024;   // chains per workgroup of the scan over the counts (256 lanes x 4)
constexpr int kPlMaxGrid = 1024;     // most workgroups of a launch that strides over the table for long chains
static_assert(kPlWaveMax > 64 && kPlWaveMax <= 1024 && kPlWaveMax % 64 == 0, "whole words of flags, more than one wave's lanes");

inline int pl_scan_blocks(int n_chains) { return (n_chains + kPlScanBlock - 1) / kPlScanBlock; }

// step 1: keep flags and kept count of every chain; e2 = eps * eps in double.  _wave: one wave per chain of length <= kPlWaveMax (and the
// count 0 of every empty chain); _block: a bounded grid of 256-lane workgroups strides over the table and takes the longer chains
hipError_t launch_pl_keep_wave(const int32_t* points, int n_points, const int32_t* chains, int n_chains, double e2, uint8_t* keep,
                               int32_t* count, hipStream_t s);
hipError_t launch_pl_keep_block(const int32_t* points, int n_points, const int32_t* chains, int n_chains, double e2, uint8_t* keep,
                                int32_t* count, hipStream_t s);
// step 2: exclusive scan of the counts, three launches (launch_scan_partials between the two); partials: pl_scan_blocks + 1 ints, the total
// in partials[blocks].  k_pl_apply turns count[c] into the chain's first vertex and -- only when the total fits `capacity` and `polylines` is
// not null -- writes the table (start, count, flags of chains[c], 0)
hipError_t launch_pl_count(const int32_t* count, int n_chains, int32_t* partials, hipStream_t s);
hipError_t launch_pl_apply(int32_t* count, int n_chains, const int32_t* partials, const int32_t* chains, int capacity, int32_t* polylines,
                           hipStream_t s);
// step 3: the kept points and (index != nullptr) their positions in `points`, at first vertex + rank; nothing when the total exceeds
// `capacity`, and no store at or beyond `capacity` in any case
hipError_t launch_pl_emit_wave(const int32_t* points, int n_points, const int32_t* chains, int n_chains, const uint8_t* keep,
                               const int32_t* first, const int32_t* partials, int capacity, int32_t* vertices, int32_t* index, hipStream_t s);
hipError_t launch_pl_emit_block(const int32_t* points, int n_points, const int32_t* chains, int n_chains, const uint8_t* keep,
                                const int32_t* first, const int32_t* partials, int capacity, int32_t* vertices, int32_t* index, hipStream_t s);

}  // namespace cvs
