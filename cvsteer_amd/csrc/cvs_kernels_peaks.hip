// cvs_kernels_peaks.hip -- orientation peaks (extension: cvs_orientation_peaks) for gfx950: every local orientation of a pixel from
// ONE read of its basis values.
//
// The composition this replaces steers the bank at K angles (cvs_steer_bank: 8 K bytes per pixel written), reads those planes back
// and searches them.  Here a lane loads its pixels' 7 / 11 basis values once, walks the K angles with the weights of all of them in the
// kernel-argument segment (scalar registers: PeaksArgs::w, as BankArgs::w), and keeps in registers only what the contract of
// include/cvsteer_hip.h needs: the two samples before the current one, the first two for the wrap-around, the running largest and
// smallest sample, and the M strongest candidates so far as a sorted list of (e_k, k, e_(k-1), e_(k+1)) kept by a fixed
// compare-and-shift chain.  No array is indexed by a run-time value, so nothing lives in scratch.  It writes 8 M + 1 bytes per pixel.
//
// (g_k, h_k) are g2_steer_weights / g4_steer_weights on the host weights of theta_k -- the expression of OP_G2_STEER_SCALAR /
// OP_G4_STEER_SCALAR and of k_steer_bank, bit for bit.  Built with -ffp-contract=off: every product and sum below rounds on its own.
#include <hip/hip_runtime.h>

#include "cvs_device_math.h"
#include "cvs_peaks.h"

namespace cvs {

namespace {

// the candidate (c, k, p, n) takes its place in the list, which is sorted by e descending: behind the entries it ties with (candidates
// arrive by ascending k), or -- FRONT_OF_TIES, for k = 0, which arrives last -- in front of them.  Empty entries hold e = -1, k = -1:
// a candidate's e is above a sample and samples are sums of squares.  gt[i] implies gt[i + 1].
template <int MM, bool FRONT_OF_TIES>
__device__ __forceinline__ void peak_insert(float (&le)[MM], int (&lk)[MM], float (&lp)[MM], float (&ln)[MM], float c, int k, float p, float n)
{
    bool gt[MM];
#pragma unroll
    for (int i = 0; i < MM; ++i) gt[i] = FRONT_OF_TIES ? c >= le[i] : c > le[i];
#pragma unroll
    for (int i = MM - 1; i >= 1; --i) {
        const bool shift = gt[i - 1];   // the entry above moves down into slot i
        le[i] = shift ? le[i - 1] : gt[i] ? c : le[i];
        lk[i] = shift ? lk[i - 1] : gt[i] ? k : lk[i];
        lp[i] = shift ? lp[i - 1] : gt[i] ? p : lp[i];
        ln[i] = shift ? ln[i - 1] : gt[i] ? n : ln[i];
    }
    le[0] = gt[0] ? c : le[0];
    lk[0] = gt[0] ? k : lk[0];
    lp[0] = gt[0] ? p : lp[0];
    ln[0] = gt[0] ? n : ln[0];
}

}  // namespace

// NB = 7 (G2) or 11 (G4).  VEC = 4: rows are walked in float4 units (the host guarantees 16-B aligned pointers, pitches and strides
// that are multiples of four, cols % 4 == 0 and a count plane of 4-byte alignment); VEC = 1: plain dwords and bytes.  MM: length of the
// list, 2 (M <= 2) or 4.
template <int NB, int VEC, int MM>
__global__ __launch_bounds__(256) void k_orientation_peaks(const PeaksArgs a)
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    constexpr int kH = NB == 7 ? 7 : 5;   // first plane of the second group
    const int ncv = a.cols / VEC;
    for (int row = blockIdx.y; row < a.rows; row += gridDim.y) {
        for (int cv = blockIdx.x * blockDim.x + threadIdx.x; cv < ncv; cv += gridDim.x * blockDim.x) {
            float b[VEC][NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const BankPlane& gp = a.in[i < kH ? 0 : 1];
                const float* src = gp.p + (size_t)(i < kH ? i : i - kH) * gp.stride + (size_t)row * gp.pitch + (size_t)cv * VEC;
                if constexpr (VEC == 4) {
                    const f4 v = *reinterpret_cast<const f4*>(src);
                    b[0][i] = v.x; b[1][i] = v.y; b[2][i] = v.z; b[3][i] = v.w;
                } else {
                    b[0][i] = *src;
                }
            }
            // e_t of this lane's pixel v: the weights are wave-uniform, read from the kernel arguments
            auto sample = [&](int t, int v) {
                float w[NB];
#pragma unroll
                for (int i = 0; i < NB; ++i) w[i] = a.w[t][i];
                float g, h;
                if constexpr (NB == 7) g2_steer_weights(b[v], w, g, h);
                else g4_steer_weights(b[v], w, g, h);
                return __fadd_rn(__fmul_rn(g, g), __fmul_rn(h, h));
            };
            float e0[VEC], e1[VEC], ep[VEC], ec[VEC], emax[VEC], emin[VEC];
            bool finite[VEC];
            float le[VEC][MM], lp[VEC][MM], ln[VEC][MM];
            int lk[VEC][MM];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                e0[v] = sample(0, v);
                e1[v] = sample(1, v);
                ep[v] = e0[v];
                ec[v] = e1[v];
                emax[v] = fmaxf(e0[v], e1[v]);
                emin[v] = fminf(e0[v], e1[v]);
                finite[v] = e0[v] < INFINITY && e1[v] < INFINITY;   // samples are sums of squares: +inf and NaN are what is not finite
#pragma unroll
                for (int s = 0; s < MM; ++s) {
                    le[v][s] = -1.f;
                    lk[v][s] = -1;
                    lp[v][s] = 0.f;
                    ln[v][s] = 0.f;
                }
            }
            for (int t = 2; t < a.n; ++t) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const float e = sample(t, v);
                    emax[v] = fmaxf(emax[v], e);
                    emin[v] = fminf(emin[v], e);
                    finite[v] = finite[v] && e < INFINITY;
                    // k = t - 1 between its neighbours
                    if (ec[v] > ep[v] && ec[v] >= e && ec[v] > a.min_energy) peak_insert<MM, false>(le[v], lk[v], lp[v], ln[v], ec[v], t - 1, ep[v], e);
                    ep[v] = ec[v];
                    ec[v] = e;
                }
            }
            float oa[MM][VEC], oe[MM][VEC];
            unsigned cnt[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                // the wrap-around: k = K - 1 against e_0, then k = 0 against e_(K-1) and e_1
                if (ec[v] > ep[v] && ec[v] >= e0[v] && ec[v] > a.min_energy) peak_insert<MM, false>(le[v], lk[v], lp[v], ln[v], ec[v], a.n - 1, ep[v], e0[v]);
                if (e0[v] > ec[v] && e0[v] >= e1[v] && e0[v] > a.min_energy) peak_insert<MM, true>(le[v], lk[v], lp[v], ln[v], e0[v], 0, ec[v], e1[v]);
                const bool pixel = finite[v] && __fsub_rn(emax[v], emin[v]) > __fmul_rn(a.min_contrast, emax[v]);
                const float floor_e = __fmul_rn(a.min_ratio, emax[v]);
                cnt[v] = 0;
#pragma unroll
                for (int s = 0; s < MM; ++s) {
                    // the entries that pass are a prefix of the list: it is sorted by e
                    const bool valid = pixel && s < a.m && lk[v][s] >= 0 && le[v][s] >= floor_e;
                    const float p = lp[v][s], c = le[v][s], n = ln[v][s];
                    const float num = __fsub_rn(p, n);
                    const float den = __fadd_rn(__fsub_rn(p, __fmul_rn(2.0f, c)), n);
                    float d = den < 0.f ? __fdiv_rn(__fmul_rn(0.5f, num), den) : 0.f;
                    d = fminf(fmaxf(d, -0.5f), 0.5f);
                    float ang = __fmul_rn(__fadd_rn((float)lk[v][s], d), a.step);
                    if (ang < 0.f) ang = __fadd_rn(ang, kPiF);
                    if (!(ang < kPiF)) ang = __fsub_rn(ang, kPiF);
                    const float en = __fsub_rn(c, __fmul_rn(__fmul_rn(0.25f, num), d));
                    oa[s][v] = valid ? ang : -1.0f;
                    oe[s][v] = valid ? en : 0.0f;
                    cnt[v] += valid ? 1u : 0u;
                }
            }
            const size_t col = (size_t)cv * VEC;
#pragma unroll
            for (int s = 0; s < MM; ++s) {
                if (s >= a.m) break;
                if (a.angle.p) {
                    float* dst = a.angle.p + (size_t)s * a.angle.stride + (size_t)row * a.angle.pitch + col;
                    if constexpr (VEC == 4) *reinterpret_cast<f4*>(dst) = f4{oa[s][0], oa[s][1], oa[s][2], oa[s][3]};
                    else *dst = oa[s][0];
                }
                if (a.energy.p) {
                    float* dst = a.energy.p + (size_t)s * a.energy.stride + (size_t)row * a.energy.pitch + col;
                    if constexpr (VEC == 4) *reinterpret_cast<f4*>(dst) = f4{oe[s][0], oe[s][1], oe[s][2], oe[s][3]};
                    else *dst = oe[s][0];
                }
            }
            if (a.count) {
                unsigned char* dst = a.count + (size_t)row * a.count_pitch + col;
                if constexpr (VEC == 4) *reinterpret_cast<unsigned*>(dst) = cnt[0] | cnt[1] << 8 | cnt[2] << 16 | cnt[3] << 24;   // four bytes, one store
                else *dst = (unsigned char)cnt[0];
            }
        }
    }
}

template <int NB>
static void launch_peaks_nb(const PeaksArgs& a, bool v4, dim3 grid, hipStream_t s)
{
    const dim3 block(256);
    const bool two = a.m <= 2;
    if (v4 && two) hipLaunchKernelGGL((k_orientation_peaks<NB, 4, 2>), grid, block, 0, s, a);
    else if (v4) hipLaunchKernelGGL((k_orientation_peaks<NB, 4, 4>), grid, block, 0, s, a);
    else if (two) hipLaunchKernelGGL((k_orientation_peaks<NB, 1, 2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_orientation_peaks<NB, 1, 4>), grid, block, 0, s, a);
}

hipError_t launch_orientation_peaks(int nb, const PeaksArgs& a, hipStream_t s)
{
    if (a.rows <= 0 || a.cols <= 0 || a.n < kPeaksMinAngles || a.n > kBankMax || a.m < 1 || a.m > kPeaksMax || (nb != 7 && nb != 11))
        return hipErrorInvalidValue;
    if (!a.angle.p && !a.energy.p && !a.count) return hipErrorInvalidValue;
    // float4 per lane when every plane it touches allows it (as launch_steer_bank), the count plane as one dword per lane
    bool v4 = a.cols % 4 == 0;
    for (int g = 0; g < (nb == 7 ? 1 : 2); ++g) {
        if (!a.in[g].p) return hipErrorInvalidValue;
        v4 = v4 && ((uintptr_t)a.in[g].p & 15) == 0 && a.in[g].pitch % 4 == 0 && a.in[g].stride % 4 == 0;
    }
    for (const PeakPlanes* p : {&a.angle, &a.energy})
        if (p->p) v4 = v4 && ((uintptr_t)p->p & 15) == 0 && p->pitch % 4 == 0 && p->stride % 4 == 0;
    if (a.count) v4 = v4 && ((uintptr_t)a.count & 3) == 0 && a.count_pitch % 4 == 0;
    const int ncv = v4 ? a.cols / 4 : a.cols;
    int gx = (ncv + 255) / 256;
    if (gx > 64) gx = 64;
    int gy = a.rows;
    // the angle loop is long (K weighted sums and a list per pixel): 64 workgroups per CU before rows are strided, as the bank's
    // magnitude / phase launches
    const int cap = 256 * 64;
    if ((long)gx * gy > cap) gy = cap / gx > 0 ? cap / gx : 1;
    const dim3 grid(gx, gy);
    if (nb == 7) launch_peaks_nb<7>(a, v4, grid, s);
    else launch_peaks_nb<11>(a, v4, grid, s);
    return hipGetLastError();
}

}  // namespace cvs
