// cvs_peaks.h -- launch descriptor of the orientation peaks (extension: cvs_orientation_peaks), shared between cvs_peaks.cpp and
// cvs_kernels_peaks.hip.  Internal; the contract of every value is stated in include/cvsteer_hip.h.
#pragma once
#include "cvs_internal.h"

namespace cvs {

constexpr int kPeaksMax = 4;        // CVS_PEAKS_MAX
constexpr int kPeaksMinAngles = 4;  // K runs from here to kBankMax: the weights of all K angles lie in the kernel-argument segment

// M planes of one output kind: slot s at p + s * stride, row pitch `pitch` (elements); p == nullptr = not written
struct PeakPlanes {
    float* p;
    size_t pitch;
    size_t stride;
};

struct PeaksArgs {
    int rows, cols;
    int n;                          // K sample angles, kPeaksMinAngles .. kBankMax
    int m;                          // M slots written, 1 .. kPeaksMax
    float min_energy, min_ratio, min_contrast;
    float step;                     // (float)(pi / K)
    // the basis planes read, as groups of planes at a constant stride, as BankArgs::in: G2 = 7 basis, G4 = g4a..e | h4a..f
    BankPlane in[2];
    PeakPlanes angle, energy;
    unsigned char* count;           // bytes; nullptr = not written
    size_t count_pitch;             // bytes
    float w[kBankMax][kMaxBasis];   // host_steer_weights of theta_k = (float)((double)k * pi / K)
};

hipError_t launch_orientation_peaks(int nb, const PeaksArgs& a, hipStream_t s);

}  // namespace cvs
