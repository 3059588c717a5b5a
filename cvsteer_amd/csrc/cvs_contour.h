// cvs_contour.h -- launch descriptors of the contour-thinning kernels (cvs_kernels_contour.hip), shared with the C-ABI layer
// (cvs_api.cpp).  Kept apart from cvs_internal.h so that the strip and per-pixel kernel objects do not depend on it.
#pragma once
#include "cvs_internal.h"

namespace cvs {
// ---- contour thinning (cvs_nonmax / cvs_hysteresis, extension; cvs_kernels_contour.hip) ----
// Non-maximum suppression of n maps across theta in ONE launch (theta read once): map k from in[k] to out[k]; pitches in elements.
constexpr int kNmsMax = 3;
struct NmsArgs {
    int rows, cols, n;
    int strip;                 // rows per wave strip (filled by the launcher)
    PlaneRef theta;
    PlaneRef in[kNmsMax], out[kNmsMax];
    int nt_stores;             // 1 = nontemporal output stores
};
hipError_t launch_nonmax(const NmsArgs& a, hipStream_t s);
// ... of `frames` frames in ONE launch (blockIdx.z = frame): `a` describes frame 0, frame z is every plane of it moved by z strides
// (elements, >= 0; the pitches are those of frame 0).  The same body as launch_nonmax: the same values, bit for bit.
struct NmsBatch {
    int frames;
    long long theta_stride;
    long long in_stride[kNmsMax], out_stride[kNmsMax];
};
hipError_t launch_nonmax_batch(const NmsArgs& a, const NmsBatch& b, hipStream_t s);
// Hysteresis over n planes (blockIdx.z): byte labels at lab + z * lab_stride (row pitch lab_pitch bytes) in device scratch; outputs
// out8[z] (bytes, out_u8 = 1) or out32[z] (f32), out_pitch in elements of the output type.
constexpr int kHystMax = 3;
struct HystArgs {
    int rows, cols, n;
    float low, high;
    PlaneRef in[kHystMax];
    unsigned char* lab;
    size_t lab_pitch, lab_stride;
    int out_u8;
    unsigned char* out8[kHystMax];
    float* out32[kHystMax];
    size_t out_pitch[kHystMax];
};
hipError_t launch_hyst_classify(const HystArgs& a, hipStream_t s);
hipError_t launch_hyst_flag_reset(unsigned* changed, hipStream_t s);   // *changed = 0, as a kernel (not a memset node)
hipError_t launch_hyst_pass(const HystArgs& a, unsigned* changed, hipStream_t s);   // one propagation pass; ++*changed if it promoted
hipError_t launch_hyst_emit(const HystArgs& a, hipStream_t s);


}  // namespace cvs
