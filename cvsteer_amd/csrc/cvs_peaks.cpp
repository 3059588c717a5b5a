// cvs_peaks.cpp -- the C ABI of the orientation peaks (extension): cvs_orientation_peaks in front of cvs_kernels_peaks.hip.  Argument
// checks, the sample angles and their host weights, staging of host planes (and of device planes the launch cannot address as a run)
// in the handle's arena, and the launch.  Nothing is read back; no arithmetic on image data happens here.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <vector>

#include "cvs_contour_host.h"
#include "cvs_layout.h"
#include "cvs_peaks.h"

using namespace cvs;

static_assert(CVS_PEAKS_MAX == kPeaksMax, "CVS_PEAKS_MAX: the list length of the kernel instances");

namespace {

bool in_unit(float v) { return v >= 0.f && v <= 1.f; }   // (false for NaN)

}  // namespace

extern "C" int cvs_orientation_peaks(cvs_handle h, const cvs_peaks_cfg* cfg, const cvs_plane* angles, const cvs_plane* energies,
                                     const cvs_plane* count)
{
    if (!h) return CVS_E_BADARG;
    if (!cfg) return fail(h, CVS_E_BADARG, "cfg");
    if (cfg->struct_size != sizeof(cvs_peaks_cfg)) return fail(h, CVS_E_BADARG, "cvs_peaks_cfg.struct_size is not sizeof(cvs_peaks_cfg)");
    if (cfg->n_angles < kPeaksMinAngles || cfg->n_angles > kBankMax) return fail(h, CVS_E_BADARG, "n_angles is 4 .. 32");
    if (cfg->max_peaks < 1 || cfg->max_peaks > kPeaksMax) return fail(h, CVS_E_BADARG, "max_peaks is 1 .. CVS_PEAKS_MAX");
    if (std::isnan(cfg->min_energy) || !in_unit(cfg->min_ratio) || !in_unit(cfg->min_contrast))
        return fail(h, CVS_E_BADARG, "thresholds: min_energy not NaN, min_ratio and min_contrast in [0, 1]");
    if (!angles && !energies && !count) return fail(h, CVS_E_BADARG, "no output requested");
    int rc = need_state(h, false);
    if (rc) return rc;
    const int K = cfg->n_angles, M = cfg->max_peaks, rows = h->rows, cols = h->cols;
    for (int s = 0; s < M; ++s)
        if ((angles && (rc = check_sized(h, &angles[s], "angles", rows, cols))) || (energies && (rc = check_sized(h, &energies[s], "energies", rows, cols))))
            return rc;
    if (count) {
        if ((rc = check_sized(h, count, "count", rows, cols, true))) return rc;
        if (!is_u8(count)) return fail(h, CVS_E_BADARG, "count is a CVS_DEPTH_U8 plane");
    }
    // an output shares no byte with another output, nor with a state plane of the selected frame (the basis planes the launch reads, and
    // the orientation planes where the handle holds them)
    std::vector<cvs_plane> ins, outs;
    for (int i = 0; i < h->nb + (h->have_orient ? 5 : 0); ++i) {
        const PlaneRef r = state_ref(h, i);
        ins.push_back(device_plane(r.p, rows, cols, r.pitch));
    }
    for (int s = 0; s < M; ++s) {
        if (angles) outs.push_back(angles[s]);
        if (energies) outs.push_back(energies[s]);
    }
    if (count) outs.push_back(*count);
    if ((rc = check_disjoint(h, ins.data(), ins.size(), outs.data(), outs.size()))) return rc;

    PeaksArgs a{};
    a.rows = rows;
    a.cols = cols;
    a.n = K;
    a.m = M;
    a.min_energy = cfg->min_energy;
    a.min_ratio = cfg->min_ratio;
    a.min_contrast = cfg->min_contrast;
    const double pi = 3.14159265358979323846;
    a.step = (float)(pi / (double)K);
    for (int k = 0; k < K; ++k) host_steer_weights(h->kind, (float)((double)k * pi / (double)K), a.w[k]);
    BankPlane in[3];
    if (!bank_inputs(h, false, in)) return fail(h, CVS_E_STATE, "state planes not at a constant stride within their group");
    a.in[0] = in[0];
    a.in[1] = in[1];

    // direct: every plane on the device and the M slots of each kind one run (a step they share, a constant distance).  Anything else
    // is written into a dense block of the arena by the same launch and copied out plane by plane.
    bool direct = true;
    for (const cvs_plane& p : outs) direct = direct && mem_of(&p) == CVS_MEM_DEVICE;
    PlaneRun run[2] = {{true, 0}, {true, 0}};
    const cvs_plane* kind[2] = {angles, energies};
    for (int o = 0; o < 2 && direct; ++o) {
        if (!kind[o]) continue;
        run[o] = plane_run(M, 1, [&](int s, int) { return plane_at(kind[o][s]); }, false, sizeof(float));
        direct = run[o].ok;
    }
    bool host = false;
    for (const cvs_plane& p : outs) host = host || mem_of(&p) == CVS_MEM_HOST;
    if (!direct && (rc = refuse_capture(h, "cvs_orientation_peaks stages these planes in the handle's arena: not capturable"))) return rc;

    const size_t pitch = round_up((size_t)cols, 64), plane = pitch * rows;   // of the staging block; count: rows of `pitch` bytes
    const size_t need = direct ? 0 : (angles ? plane * M : 0) + (energies ? plane * M : 0) + (count ? round_up(plane / 4 + 64, 64) : 0);
    Call c;
    if ((rc = begin(h, c, {}, need))) return rc;
    PeakPlanes* dst[2] = {&a.angle, &a.energy};
    if (direct) {
        for (int o = 0; o < 2; ++o)
            if (kind[o]) *dst[o] = {kind[o][0].data, kind[o][0].step / sizeof(float), (size_t)run[o].stride / sizeof(float)};
        if (count) {
            a.count = reinterpret_cast<unsigned char*>(count->data);
            a.count_pitch = count->step;
        }
    } else {
        for (int o = 0; o < 2; ++o)
            if (kind[o]) *dst[o] = {arena_take(h, plane * M), pitch, plane};
        if (count) {
            a.count = reinterpret_cast<unsigned char*>(arena_take(h, plane / 4 + 64));
            a.count_pitch = pitch;
        }
    }
    HIP_TRY(h, launch_orientation_peaks(h->nb, a, h->stream));
    if (!direct) {
        auto kind_of = [](const cvs_plane* p) { return mem_of(p) == CVS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice; };
        for (int o = 0; o < 2; ++o)
            for (int s = 0; kind[o] && s < M; ++s) {
                const cvs_plane* p = &kind[o][s];
                HIP_TRY(h, copy_rows(p->data, p->step, dst[o]->p + (size_t)s * plane, pitch * sizeof(float), (size_t)cols * sizeof(float), rows,
                                     kind_of(p), h->stream));
            }
        if (count) HIP_TRY(h, copy_rows(count->data, count->step, a.count, pitch, (size_t)cols, rows, kind_of(count), h->stream));
        if (host) HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return CVS_OK;
}
