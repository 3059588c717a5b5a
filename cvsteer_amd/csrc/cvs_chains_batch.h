// cvs_chains_batch.h -- launch descriptors of the contour-chain kernels on the batch axis (cvs_kernels_chains_batch.hip), shared with their
// C-ABI layer (cvs_chains_batch.cpp).  The n planes of a call are STACKED: the link plane, the parent plane and the aux plane of
// cvs_chains.h hold n * rows rows of cols columns, plane z at rows z * rows .. (z + 1) * rows - 1, and a pixel's linear index is
// LIN(z, p) = z * rows * cols + lin(p).  No link and no union crosses a seam between two planes, so every launch of cvs_chains.h from
// launch_ch_nodes to launch_ch_head_count serves the block as it is, called with n * rows rows; only the links, the labelling, the table and
// the emit know what a plane is, and those are declared here.
#pragma once
#include "cvs_chains.h"
#include "cvs_refine.h"

namespace cvs {

constexpr int kChbTableBatch = 16;   // plane descriptors one k_chb_table launch carries in its arguments
constexpr int kChbGridZ = 65535;     // planes one launch addresses by blockIdx.z; more planes take more launches (PlaneSet::z0)

struct ChbTableArgs {
    MaskRef d[kChbTableBatch];
    int first, count;   // d[0 .. count) -> tab[first ..]
};

// n planes of rows x cols: tab[z] when tab != nullptr, else plane 0 (`first`) moved by z strides >= 0 of `stride` BYTES
struct PlaneSet {
    MaskRef first;
    long long stride;
    const MaskRef* tab;
};

struct ChbArgs {
    int rows, cols, n;   // n planes; n * rows * cols <= 2^28
    int z0;              // the launch covers planes z0 + blockIdx.z (set by the launchers)
    PlaneSet masks;
    uint16_t* link;      // stacked planes, dense
    int32_t* parent;
    int32_t* aux;        // cleared by the tile launch
};

hipError_t launch_chb_table(const ChbTableArgs& t, MaskRef* tab, hipStream_t s);
// step 1: the link bits of every pixel of every plane; rows outside a plane are background
hipError_t launch_chb_links(const ChbArgs& a, hipStream_t s);
// step 2: tile-local components per plane -> parent (stacked indices), aux cleared; unions across the tile borders of each plane
hipError_t launch_chb_tiles(const ChbArgs& a, hipStream_t s);
hipError_t launch_chb_borders(const ChbArgs& a, hipStream_t s);
// step 6: launch_ch_head_apply that also writes the plane of every chain into the table's fourth word (plane_pixels = rows * cols);
// launch_ch_emit that stores coordinates inside the point's own plane; the range table -- 2 * (n + 1) ints, entry z = (first chain, first
// point) of plane z, entry n the totals, an empty plane its successor's pair.  n_chains >= 1
hipError_t launch_chb_head_apply(int arcs, HeadRec* head, const int32_t* part_n, const int32_t* part_len, const int32_t* to, const int32_t* rev,
                                 int plane_pixels, int32_t* chains, int n_chains, hipStream_t s);
hipError_t launch_chb_emit(int arcs, int rows, int cols, const int32_t* to, const int32_t* rev, const ArcRec* rec, const HeadRec* head,
                           int32_t* points, int n_points, hipStream_t s);
hipError_t launch_chb_ranges(const int32_t* chains, int n_chains, int n_points, int n, int32_t* ranges, hipStream_t s);

// ---- sub-pixel chain points on the batch axis (cvs_chain_refine_batch) ----
// One lane per point: its plane z is the largest z in 0 .. n - 1 with ranges[2 * z + 1] <= i (a binary search that cannot leave 0 .. n - 1,
// whatever `ranges` holds), the samples come from maps[z], theta from theta[z / n_maps]; the rest is k_chain_refine's body.
struct RefineBatchArgs {
    int rows, cols, n, n_maps;   // n = frames * n_maps planes
    PlaneSet maps, theta;        // f32 planes (u8 = 0): n maps, n / n_maps theta planes
    const int32_t* points;
    int n_points;
    const int32_t* ranges;       // 2 * (n + 1) ints
    float* xy;
    float* strength;             // nullptr, or n_points floats
};
hipError_t launch_chain_refine_batch(const RefineBatchArgs& a, hipStream_t s);

}  // namespace cvs
