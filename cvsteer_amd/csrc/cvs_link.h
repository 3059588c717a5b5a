// cvs_link.h -- launch descriptors of the one-pass link kernels (cvs_kernels_link.hip), shared with their C-ABI layer (cvs_link.cpp).
// cvs_link is hysteresis and prune in ONE labelling: the foreground of a plane is { v > low }, a component is kept iff its largest value
// is > high and >= min_peak and it has >= min_area pixels.  Any number of planes per launch (blockIdx.z), four launches per chain.
#pragma once
#include "cvs_components.h"

namespace cvs {

// the most scratch the parent, area and peak planes of one chain may take (12 bytes per pixel; the descriptor table and the byte staging
// of host outputs come on top); more planes than fit run as several chains, one plane that does not fit runs alone.  A chain is also bounded by what one grid dimension can count.
constexpr size_t kLinkScratchMax = (size_t)1 << 30;
constexpr int kLinkChainMax = 65535;
constexpr int kLinkTableBatch = 16;   // plane descriptors one k_link_table launch carries in its arguments

// one plane of a chain: input (f32) and output (bytes or f32), pitches in elements of each plane's own type
struct LinkDesc {
    const float* in;
    size_t in_pitch;
    void* out;
    size_t out_pitch;
};
struct LinkTableArgs {
    LinkDesc d[kLinkTableBatch];
    int first, count;   // d[0 .. count) -> tab[first ..]
};

struct LinkArgs {
    int rows, cols, n;   // n planes in this chain
    float low, high;
    int min_area;
    float min_peak;
    int out_u8;
    // plane z: tab[z] when tab != nullptr, else plane 0 (`first`) moved by z strides >= 0 (in: elements, out: BYTES)
    LinkDesc first;
    long long in_stride, out_stride;
    const LinkDesc* tab;
    // scratch, dense planes of plane_stride elements each, plane z at z * plane_stride
    int32_t* parent;
    int32_t* area;
    uint32_t* peak;
    size_t plane_stride;
    int32_t* kept;   // n counters (cleared by the tile launch), or nullptr
};

hipError_t launch_link_table(const LinkTableArgs& t, LinkDesc* tab, hipStream_t s);
// step 1: v > low -> tile-local components in LDS -> parent; area and peak cleared, kept[z] = 0
hipError_t launch_link_tiles(const LinkArgs& a, hipStream_t s);
// step 2: unions across the tile borders (agent-scope atomics on parent only)
hipError_t launch_link_borders(const LinkArgs& a, hipStream_t s);
// step 3: area and the ordered bits of the largest value, accumulated at each component's root
hipError_t launch_link_stats(const LinkArgs& a, hipStream_t s);
// step 4: the verdict of each pixel's root -> 0 / 255, and the number of components kept
hipError_t launch_link_emit(const LinkArgs& a, hipStream_t s);

}  // namespace cvs
