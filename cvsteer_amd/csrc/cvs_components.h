// cvs_components.h -- launch descriptors of the contour-component kernels (cvs_kernels_components.hip), shared with their C-ABI layer
// (cvs_components.cpp).  Kept apart from cvs_contour.h: the thinning kernels do not depend on it.
#pragma once
#include "cvs_internal.h"

namespace cvs {
// ---- contour components (cvs_label / cvs_component_stats / cvs_contour_prune / cvs_contour_points, extension) ----
// A PARENT plane holds one int32 per pixel, dense (row pitch = cols): -1 for background, else the linear index (row * cols + col) of
// another pixel of the same component that is not larger than the pixel's own; a root holds its own index.
constexpr int kCcTileW = 128;   // tile of the in-LDS labelling, columns
constexpr int kCcTileH = 32;    // ... rows
constexpr int kCcScanBlock = 4096;   // elements per workgroup of the scan launches (256 lanes x 16)

struct MaskRef {
    const void* p;   // f32 (foreground: v > 0.0f) or bytes (foreground: non-zero)
    size_t pitch;    // elements of the plane's own type
    int u8;
};
struct IntPlane {
    int32_t* p;
    size_t pitch;    // elements
};

// step 1: tile-local components in LDS -> parent (plain stores); zero_a / zero_b (dense planes, may be nullptr) are cleared on the way
hipError_t launch_cc_tiles(const MaskRef& mask, int rows, int cols, int32_t* parent, int32_t* zero_a, uint32_t* zero_b, hipStream_t s);
// step 2: unions across the tile borders (agent-scope atomics on parent only)
hipError_t launch_cc_borders(int rows, int cols, int32_t* parent, hipStream_t s);
// step 3 (prune): root of every pixel -> root (dense), parent read-only
hipError_t launch_cc_flatten(int rows, int cols, const int32_t* parent, int32_t* root, hipStream_t s);

// exclusive scan of a per-pixel flag in raster order, three launches.  Flag kinds: kScanRoots = parent[i] == i (plane dense),
// kScanNonZero = value != 0 (any pitch).  partials: number of workgroups + 1 ints; after launch_scan_partials partials[b] is the number of
// flagged pixels before workgroup b and partials[blocks] the total.
enum { kScanRoots = 0, kScanNonZero = 1 };
inline int scan_blocks(int rows, int cols) { return (int)(((long long)rows * cols + kCcScanBlock - 1) / kCcScanBlock); }
hipError_t launch_scan_count(int kind, const IntPlane& v, int rows, int cols, int32_t* partials, hipStream_t s);
hipError_t launch_scan_partials(int32_t* partials, int blocks, hipStream_t s);
// kScanRoots: rank[i] = rank of root i (written at roots only); kScanNonZero: points[3 * rank ..] = (x, y, value)
hipError_t launch_scan_apply(int kind, const IntPlane& v, int rows, int cols, const int32_t* partials, int32_t* out, hipStream_t s);
// step 4 (label): labels = rank[root of the pixel] + 1, 0 for background
hipError_t launch_cc_relabel(int rows, int cols, const int32_t* parent, const int32_t* rank, const IntPlane& labels, hipStream_t s);

// statistics of a label plane: acc = count accumulators (device), then the table (count entries of 40 bytes, device)
struct CcAcc {
    int32_t area, x0, x1, y1, first, pad;
    unsigned long long key;   // (ordered weight bits << 32) | ~linear index; 0 = no weight seen
};
hipError_t launch_stats_init(CcAcc* acc, int count, hipStream_t s);
hipError_t launch_stats(const IntPlane& labels, int rows, int cols, int count, const PlaneRef& weight, CcAcc* acc, hipStream_t s);
hipError_t launch_stats_table(const CcAcc* acc, int count, int cols, void* table, hipStream_t s);

// prune: area / peak keyed by the root pixel, then the 0 / 255 output and the number of components kept
hipError_t launch_prune_stats(int rows, int cols, const int32_t* root, const PlaneRef& weight, int32_t* area, uint32_t* peak, hipStream_t s);
struct PruneEmit {
    int rows, cols;
    const int32_t* root;
    const int32_t* area;
    const uint32_t* peak;   // nullptr: no weight
    int min_area;
    float min_peak;
    int out_u8;
    void* out;              // bytes or f32
    size_t out_pitch;       // elements of the output type
    int32_t* kept;          // one counter, zeroed before
};
hipError_t launch_prune_emit(const PruneEmit& a, hipStream_t s);
hipError_t launch_zero_ints(int32_t* p, int n, hipStream_t s);

}  // namespace cvs
