// cvs_chains.h -- launch descriptors of the contour-chain kernels (cvs_kernels_chains.hip), shared with their C-ABI layer
// (cvs_chains.cpp).  The labelling itself is that of cvs_components.h: k_cc_tiles and k_cc_borders are launched as they are.
#pragma once
#include "cvs_components.h"

namespace cvs {
// ---- contour chains (cvs_contour_chains, extension) ----
// The LINK plane holds one uint16 per pixel, dense (row pitch = cols).  Bits 0..7: a link to the neighbour in direction d, directions
// numbered by ascending linear index of the neighbour -- NW N NE W E SW S SE, so direction d and 7 - d are opposite.  Bit 8: foreground.
// Bit 9: the pixel is a node (degree != 2, or the root of a component that has no such pixel).  Background is 0.
constexpr unsigned kChFg = 0x100u, kChNode = 0x200u;

// An ARC is a directed link.  The arcs that leave pixel p have the ids base[p] + k, k counting p's links in direction order, so arc ids
// ascend by (lin(from), lin(to)); a pixel without links owns one pseudo arc (rev[a] == a).  Per arc: to[a] = lin of its target, rev[a] = the
// id of the opposite arc, and an ArcRec for the pointer jumping.
struct alignas(8) ArcRec {
    int32_t next;   // an arc further along the same direction; a terminal arc (its target is a node) points at itself
    int32_t dist;   // arcs between this one and `next`
};
struct alignas(8) HeadRec {
    int32_t len;     // points of the chain this arc is the canonical first arc of, 0 for every other arc; after the scan: the chain's start
    int32_t flags;   // CVS_CHAIN_* of that chain
};
constexpr int kChainClosed = 1, kChainHeadJunction = 2, kChainTailJunction = 4;   // CVS_CHAIN_* (cvs_chains.cpp asserts they are)
constexpr int kChArcBlock = 1024;   // arcs per workgroup of the scan over the arcs (256 lanes x 4)
// the counters k_ch_roots fills (ints, zeroed before)
enum { kChIsolated = 0, kChSumDeg = 1, kChNodeDeg = 2, kChClosed = 3, kChCounters = 4 };

// step 1: link bits, foreground and degree != 2 of every pixel -> link
hipError_t launch_ch_links(const MaskRef& mask, int rows, int cols, uint16_t* link, hipStream_t s);
// step 2: flag[root of p] = 1 for every pixel p of degree != 2 (flag: dense ints, zero before; parent final)
hipError_t launch_ch_nodes(int rows, int cols, const uint16_t* link, const int32_t* parent, int32_t* flag, hipStream_t s);
// ... the root of a component without a flag becomes a node; the four counters over all pixels
hipError_t launch_ch_roots(int rows, int cols, uint16_t* link, const int32_t* parent, const int32_t* flag, int32_t* counters, hipStream_t s);
// step 3: exclusive scan of the arcs per pixel in raster order, three launches (launch_scan_partials between the two); partials as in
// cvs_components.h
hipError_t launch_ch_arc_count(int rows, int cols, const uint16_t* link, int32_t* partials, hipStream_t s);
hipError_t launch_ch_arc_base(int rows, int cols, const uint16_t* link, const int32_t* partials, int32_t* base, hipStream_t s);
// step 4: to, rev and the first ArcRec of every arc
hipError_t launch_ch_arcs(int rows, int cols, const uint16_t* link, const int32_t* base, int arcs, int32_t* to, int32_t* rev, ArcRec* rec,
                          hipStream_t s);
// step 5: one round of pointer jumping, in -> out
hipError_t launch_ch_jump(int arcs, const ArcRec* in, ArcRec* out, hipStream_t s);
// step 6: the canonical first arcs and their chains' lengths and flags; their scan (count and length: two partials arrays, scanned by
// launch_scan_partials each); the chain table and every chain's start; the points
hipError_t launch_ch_heads(int arcs, const uint16_t* link, const int32_t* to, const int32_t* rev, const ArcRec* rec, HeadRec* head, hipStream_t s);
inline int ch_scan_blocks(int arcs) { return (arcs + kChArcBlock - 1) / kChArcBlock; }
hipError_t launch_ch_head_count(int arcs, const HeadRec* head, int32_t* part_n, int32_t* part_len, hipStream_t s);
// (n_chains, n_points: what the caller's arrays hold -- no store goes beyond them)
hipError_t launch_ch_head_apply(int arcs, HeadRec* head, const int32_t* part_n, const int32_t* part_len, int32_t* chains, int n_chains,
                                hipStream_t s);
hipError_t launch_ch_emit(int arcs, int cols, const int32_t* to, const int32_t* rev, const ArcRec* rec, const HeadRec* head, int32_t* points,
                          int n_points, hipStream_t s);

}  // namespace cvs
