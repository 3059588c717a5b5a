// cvs_api.cpp -- the C ABI of libcvsteer_hip.so (declared in include/cvsteer_hip.h) but for the caller pipeline (cvs_pipeline.cpp)
// and the multi-GPU batch layer (cvs_batch.cpp): handles and options, the setup calls and do_setup behind them, state access, steering,
// and the per-pixel stages.
//
// Argument checks, device-state ownership, host<->device staging when a caller hands over host planes, and kernel dispatch.  All
// arithmetic on the hot path is in the HIP kernels; the only host arithmetic is what the reference also does on the host before it
// touches an image: tap generation and the scalar steering weights of a given theta (cvs_taps.cpp).  No CPU fallback exists.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "cvs_context.h"
#include "cvs_layout.h"

using namespace cvs;

int cvs::do_setup(cvs_handle h, const SetupReq& rq)
{
    if (!h) return CVS_E_BADARG;
    const cvs_plane *image = rq.image, *g = rq.g, *hq = rq.hq, *pyr = rq.pyr;
    unsigned flags = rq.flags;
    int rc = check_plane(h, image, "image", true);
    if (rc) return rc;
    if (pyr) {  // the next pyramid level, written by the same pass (cvs_setup_pyr)
        if ((rc = check_plane(h, pyr, "next_level")) || (rc = check_same(h, pyr, (image->rows + 1) / 2, (image->cols + 1) / 2))) return rc;
    }
    if (flags & ~(unsigned)CVS_SETUP_FULL) return fail(h, CVS_E_BADARG, "unknown setup flags");
    if (!(flags & CVS_SETUP_BASIS)) flags |= CVS_SETUP_BASIS;
    if ((flags & CVS_SETUP_ORIENT) && h->kind != CVS_KIND_G2 && !h->g4_ext)
        return fail(h, CVS_E_UNSUPPORTED, "the reference computes no orientation for G4 (G4.cpp:67-81); see CVS_OPT_G4_EXTENSIONS");
    if (rq.steer) {
        if ((rc = check_plane(h, g, "g")) || (rc = check_plane(h, hq, "hq"))) return rc;
        if ((rc = check_same(h, g, image->rows, image->cols)) || (rc = check_same(h, hq, image->rows, image->cols))) return rc;
    }
    // the kernel reads rows ahead of the rows it writes: an output that shares memory with the input would be
    // clobbered mid-flight (the reference's sepFilter2D copies in that case; here it is an error)
    {
        const cvs_plane* outs_chk[11] = {rq.steer ? g : nullptr, rq.steer ? hq : nullptr};
        for (int k = 0; k < 8; ++k) outs_chk[2 + k] = rq.pipe_outs ? rq.pipe_outs[k] : nullptr;
        outs_chk[10] = pyr;
        if ((rc = check_no_overlap(h, image, outs_chk, 11))) return rc;
    }
    const size_t pitch = round_up((size_t)image->cols, 64);
    size_t max_pitch = std::max(pitch, is_u8(image) ? pitch : image->step / sizeof(float));
    if (rq.steer) max_pitch = std::max(max_pitch, std::max(g->step, hq->step) / sizeof(float));
    if (rq.pipe_outs)
        for (int k = 0; k < 8; ++k)
            if (rq.pipe_outs[k]) max_pitch = std::max(max_pitch, rq.pipe_outs[k]->step / sizeof(float));
    if (state_interleaved(h, image->rows, pitch)) max_pitch = std::max(max_pitch, pitch * (size_t)(h->kind == CVS_KIND_G4 ? 6 : 7));
    const bool may_generic = basis_may_need_scratch(h->kind, h->width, h->taps, image->rows, image->cols, max_pitch);
    const size_t scratch = may_generic ? round_up(basis_scratch_elems(h->kind, h->width, image->rows, pitch), 64) : 0;
    Call c;
    const cvs_plane* po[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (rq.pipe_outs)
        for (int k = 0; k < 8; ++k) po[k] = rq.pipe_outs[k];
    const bool u8_bytes = rq.u8 && rq.u8->mode == 1;   // the outputs are the caller's byte planes: nothing to stage for them
    // 8-bit images (what the reference's callers hold: test/test.cpp:73,85, example/steer.cpp:73-86) are read by the strip kernel
    // as bytes: 1 B/pix of input traffic instead of 1 B read + 4 B written by a widening pass + 4 B read
    c.u8_direct = is_u8(image) && !may_generic && !pyr;
    const size_t u8_stage = (c.u8_direct && mem_of(image) == CVS_MEM_HOST) ? u8_stage_elems(image) : 0;
    if (u8_bytes) {
        rc = begin(h, c, {c.u8_direct ? nullptr : image}, scratch + u8_stage);
    } else {
        rc = begin(h, c, {c.u8_direct ? nullptr : image, rq.steer ? g : nullptr, rq.steer ? hq : nullptr, po[0], po[1], po[2], po[3], po[4], po[5], po[6], po[7], pyr},
                   scratch + u8_stage);
    }
    if (rc) return rc;
    // host planes on the fast path of a large enough image: upload, filtering and download overlap band by band
    // (it pays when a sizeable upload can hide behind the downloads: an f32 host image with host outputs -- measured
    // 3.06 vs 3.70 ms per 4096^2 image; with an 8-bit or device image the downloads alone set the pace and the bands
    // only add per-copy overhead, 2.98 vs 2.85 ms: round 2, profiles/HISTORY_rounds_1_3.md)
    bool any_host = false;
    for (const cvs_plane* o : {rq.steer ? g : nullptr, rq.steer ? hq : nullptr, po[0], po[1], po[2], po[3], po[4], po[5], po[6], po[7]})
        any_host = any_host || (o && o->mem == CVS_MEM_HOST);
    any_host = any_host && mem_of(image) == CVS_MEM_HOST && !is_u8(image);
    hipStreamCaptureStatus cap_st = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(h->stream, &cap_st);
    const bool overlap = h->host_overlap && any_host && !may_generic && rq.nframes == 1 && rq.out_row_hi <= rq.out_row_lo && !pyr &&
                         cap_st == hipStreamCaptureStatusNone && (size_t)image->rows * image->cols >= ((size_t)1 << 20) &&
                         image->rows >= 16 * (2 * h->width + 1) && !(h->kind == CVS_KIND_G4 && (flags & CVS_SETUP_ORIENT));
    c.defer = overlap;
    h->have_basis = h->have_orient = false;
    if ((rc = ensure_state(h, image->rows, image->cols, rq.nframes))) return rc;
    h->cur_frame = rq.frame;

    BasisArgs a{};
    PlaneRef in;
    if ((rc = in_ref(c, image, in))) return rc;
    a.in = in.p;
    a.in_pitch = in.pitch;
    a.in_u8 = c.u8_direct ? 1 : 0;
    a.rows = image->rows;
    a.cols = image->cols;
    fill_state_args(h, a, (flags & CVS_SETUP_ORIENT) && h->kind == CVS_KIND_G2);
    a.atan_mode = h->atan_mode;
    // a different input pointer than last time = a stream of fresh images (not resident in the Infinity Cache);
    // the pipeline variants keep the taller strips (round 1 shape sweep)
    // (a handle's FIRST call counts as a fresh image too: the reference's callers build one object per image,
    // example/steer.cpp:86 -- only a handle that is handed the same pointer again is re-filtering a resident image)
    const bool fresh = h->last_image != (const void*)image->data && !rq.pipe_outs;
    h->last_image = image->data;
    a.strip_rows = default_strip_rows(h, a.rows, a.cols, fresh);
    a.block_order = h->block_order >= 0 ? h->block_order : 0;   // the default's order (default_config): what basis_u8_fusable below judges
    // New images of 24 MiB and more: the waves of the launch's first fifth of row bands also touch the rest of the image (four
    // bands each), so that it is requested from HBM while the launch is young and most of the launch streams its writes without
    // reads mixed in.  Same process, alternating settings (profiles/r05_fresh_warm.txt): basis pass on alternating 8192^2 images
    // 0.626 -> 0.744 of the HBM roofline, fused steer on rotating 4096^2 images 0.624 -> 0.716, one object per image 0.614 ->
    // 0.700, full setup 0.624 -> 0.697; a separate read pass in front of the launch (round 4's tuner candidate, removed) reached
    // 0.708 where this reaches 0.729 and cannot serve an 8192^2 image at all.  Not for: the launch that also emits the next pyramid
    // level (-8 %: its cached half-line stores want the L2 for themselves; with streaming stores for the level the launch gains
    // 7-13 % and the next level's launch, which then reads its image from HBM, loses more: config 3 0.658 -> 0.640, measured again in round 6,
    // profiles/r06_c3_chain_localisation.txt), 8-bit images of 4096^2 (-5 ... -6 %) and small images (level to -3 %).  G4 images are requested
    // ahead as well since round 6 (+2.2 ... +2.4 % on rotating 4096^2 images, profiles/r06_fresh_exact_wait.txt).  CVS_OPTS warm=K overrides K (0 = off).
    {
        const size_t in_bytes = (size_t)a.rows * a.cols * (a.in_u8 ? 1 : sizeof(float));
        const int wk = env_opts().warm;
        a.warm_k = (fresh && !pyr && in_bytes >= ((size_t)24 << 20)) ? (wk >= 0 ? wk : 4) : 0;
    }
    a.nt_stores = use_nt_stores(h, (size_t)a.rows * a.cols);
    a.out_row_lo = rq.out_row_lo;
    a.out_row_hi = rq.out_row_hi;
    if (rq.steer) {
        PlaneRef rg, rh;
        if ((rc = out_ref(c, g, rg)) || (rc = out_ref(c, hq, rh))) return rc;
        a.steer_g = rg.p;
        a.steer_g_pitch = rg.pitch;
        a.steer_h = rh.p;
        a.steer_h_pitch = rh.pitch;
        host_steer_weights(h->kind, rq.theta, a.steer_w);
    }
    if (rq.pipe_outs) {
        a.pipe = 1;
        a.no_state = h->persist ? 0 : 1;
        a.find_on_e = h->find_on;
        for (int k = 0; k < 8; ++k) {
            if (u8_bytes) a.pipe_out[k] = po[k] ? PlaneRef{po[k]->data, po[k]->step} : PlaneRef{nullptr, 0};   // (pitch in bytes)
            else if ((rc = out_ref(c, po[k], a.pipe_out[k]))) return rc;
        }
        if (rq.u8) {
            a.u8_mode = rq.u8->mode;
            a.u8_gain = rq.u8->gain;
            a.u8_mm = rq.u8->mm;
        }
    }
    if (pyr) {
        PlaneRef rp;
        if ((rc = out_ref(c, pyr, rp))) return rc;
        a.pyr_out = rp.p;
        a.pyr_pitch = rp.pitch;
    }
    float* scr = scratch ? arena_take(h, scratch) : nullptr;
    if (overlap) {
        if ((rc = host_pipeline(h, c, a, scr))) return rc;
        h->have_basis = !(rq.pipe_outs && !h->persist);
        h->have_orient = h->have_basis && (flags & CVS_SETUP_ORIENT) != 0;
        return CVS_OK;
    }
    if (rq.u8 && !basis_u8_fusable(h->kind, h->width, h->taps, a)) return kNotFused;
    if (rq.u8 && rq.u8->mode == 2) HIP_TRY(h, launch_minmax_init_n(rq.u8->mm, 3, h->stream));
    {
        const bool orient_k = a.orient != nullptr;
        const int variant = (orient_k ? 1 : 0) | (rq.steer ? 2 : 0) | (a.pipe ? 4 : 0) | (a.no_state ? 8 : 0);
        TuneToken tok;
        if ((rc = tune_begin(h, a, variant, fresh, tok))) return rc;
        if ((a.merge_orient != 0) != (h->ngrp == 1 && h->kind == CVS_KIND_G2)) {   // the configuration wants the other grouping of the planes
            layout_state(h, a.merge_orient != 0);
            fill_state_args(h, a, orient_k);
        }
        note_launch(h, a);
        const hipError_t le = launch_basis(h->kind, h->width, h->taps, a, scr, h->stream);
        tune_end(h, tok);
        HIP_TRY(h, le);
    }
    if ((flags & CVS_SETUP_ORIENT) && h->kind == CVS_KIND_G4) {  // extension: one per-pixel pass over the 11 planes
        PointArgs pa{};
        pa.rows = a.rows;
        pa.cols = a.cols;
        pa.atan_mode = h->atan_mode;
        pa.nt_stores = a.nt_stores;
        for (int p = 0; p < 11; ++p) pa.in[p] = state_ref(h, p);
        for (int i = 0; i < 5; ++i) pa.out[i] = state_ref(h, h->nb + i);
        HIP_TRY(h, launch_point(OP_G4_ORIENT, pa, h->stream));
    }
    // a pipeline run with CVS_OPT_PERSIST_STATE = 0 wrote its outputs only: no state to address afterwards
    h->have_basis = !(rq.pipe_outs && !h->persist);
    h->have_orient = h->have_basis && (flags & CVS_SETUP_ORIENT) != 0;
    return finish(c);
}

int cvs::need_state(cvs_handle h, bool orient)
{
    if (!h) return CVS_E_BADARG;
    if (!h->have_basis) return fail(h, CVS_E_STATE, "no setup yet");
    if (orient && !h->have_orient) return fail(h, CVS_E_STATE, "orientation state not computed (setup without CVS_SETUP_ORIENT)");
    return CVS_OK;
}

// the state planes a bank launch reads, as groups at a constant stride (BankArgs::in: basis | C1..C3, or g4 | h4 | C1..C3; C1..C3 only
// with `e`); false = the layout does not allow it.  cvs_peaks.cpp reads the basis groups the same way
bool cvs::bank_inputs(cvs_handle h, bool e, BankPlane in[3])
{
    const int nb = h->nb, split = nb == 7 ? 7 : 5;
    const int first[3] = {0, split, nb}, count[3] = {split, nb - split, 3};
    const int ng = (nb == 7 ? 1 : 2) + (e ? 1 : 0);
    for (int g = 0; g < 3; ++g) in[g] = {nullptr, 0, 0};
    for (int g = 0; g < ng; ++g) {
        const int f = g == ng - 1 && e ? nb : first[g], m = g == ng - 1 && e ? 3 : count[g];
        const PlaneRef p0 = state_ref(h, f);
        const size_t stride = m > 1 ? (size_t)(state_plane(h, f + 1) - p0.p) : 0;
        for (int j = 1; j < m; ++j) {
            const PlaneRef pj = state_ref(h, f + j);
            if (pj.p != p0.p + (size_t)j * stride || pj.pitch != p0.pitch) return false;
        }
        in[g] = {p0.p, p0.pitch, stride};
    }
    return true;
}

namespace {

void basis_inputs(cvs_handle h, PointArgs& a)
{
    for (int p = 0; p < h->nb; ++p) a.in[p] = state_ref(h, p);
}

int steer_common(cvs_handle h, bool map, float theta, const cvs_plane* theta_map, const cvs_plane* g, const cvs_plane* hq,
                 const cvs_plane* e, const cvs_plane* mag, const cvs_plane* phase)
{
    int rc = need_state(h, false);
    if (rc) return rc;
    if ((rc = check_plane(h, g, "g")) || (rc = check_plane(h, hq, "hq"))) return rc;
    const cvs_plane* all[6] = {g, hq, e, mag, phase, theta_map};
    for (const cvs_plane* p : all) {
        if (!p) continue;
        if ((rc = check_plane(h, p, "plane")) || (rc = check_same(h, p, h->rows, h->cols))) return rc;
    }
    if (h->kind == CVS_KIND_G4 && (e || mag || phase) && !h->g4_ext)
        return fail(h, CVS_E_UNSUPPORTED, "G4 has no energy / magnitude / phase in the reference (G4.cpp:88-90); see CVS_OPT_G4_EXTENSIONS");
    if (e && (rc = need_state(h, true))) return rc;
    if (map && !theta_map && (rc = need_state(h, true))) return rc;
    if ((rc = check_point_overlaps(h, {theta_map}, {g, hq, e, mag, phase}))) return rc;

    Call c;
    if ((rc = begin(h, c, {g, hq, e, mag, phase, theta_map}))) return rc;
    PointArgs a{};
    a.rows = h->rows;
    a.cols = h->cols;
    a.atan_mode = h->atan_mode;
    basis_inputs(h, a);
    const int nb = h->nb;
    if (e) {  // C1..C3 follow the basis planes: in[7..9] (G2) / in[11..13] (G4 extension)
        for (int i = 0; i < 3; ++i) a.in[nb + i] = state_ref(h, nb + i);
    }
    if (map) {
        PlaneRef th;
        if (theta_map) {
            if ((rc = in_ref(c, theta_map, th))) return rc;
        } else {
            th = state_ref(h, nb + 3);
        }
        a.in[h->kind == CVS_KIND_G2 ? 10 : 14] = th;
    } else {
        host_steer_weights(h->kind, theta, a.w);
        // G2.cpp:162: float c2t(std::cos(theta * 2.0)) -- double argument, narrowed
        a.c2t = (float)std::cos((double)theta * 2.0);
        a.s2t = (float)std::sin((double)theta * 2.0);
    }
    const cvs_plane* outs[5] = {g, hq, e, mag, phase};
    for (int o = 0; o < 5; ++o)
        if ((rc = out_ref(c, outs[o], a.out[o]))) return rc;
    PointOp op = h->kind == CVS_KIND_G2 ? (map ? OP_G2_STEER_MAP : OP_G2_STEER_SCALAR)
                                        : (map ? OP_G4_STEER_MAP : OP_G4_STEER_SCALAR);
    a.nt_stores = use_nt_stores(h, (size_t)a.rows * a.cols);
    a.nt_loads = a.nt_stores;  // the state planes of an image that large are not cache-resident and are read once here
    HIP_TRY(h, launch_point(op, a, h->stream));
    return finish(c);
}

}  // namespace

extern "C" {

int cvs_abi_version(void) { return CVS_ABI_VERSION; }

const char* cvs_status_string(int s)
{
    switch (s) {
        case CVS_OK: return "ok";
        case CVS_E_BADARG: return "bad argument";
        case CVS_E_SIZE: return "bad size";
        case CVS_E_HIP: return "HIP error";
        case CVS_E_NOMEM: return "out of memory";
        case CVS_E_STATE: return "state not available";
        case CVS_E_UNSUPPORTED: return "unsupported for this kind";
    }
    return "unknown status";
}

int cvs_num_basis(int kind) { return host_num_basis(kind); }

int cvs_make_taps(int kind, int idx, int width, float spacing, float* out)
{
    return host_make_taps(kind, idx, width, spacing, out) ? CVS_E_BADARG : CVS_OK;
}

int cvs_basis_taps(int kind, int p, int* kx, int* ky) { return host_basis_taps(kind, p, kx, ky) ? CVS_E_BADARG : CVS_OK; }

int cvs_steer_weights(int kind, float theta, float* out) { return host_steer_weights(kind, theta, out) ? CVS_E_BADARG : CVS_OK; }

int cvs_create(int kind, int width, float spacing, int device, cvs_handle* out)
{
    if (!out) return CVS_E_BADARG;
    *out = nullptr;
    const int nb = host_num_basis(kind);
    if (nb == 0 || width < 1 || width > kMaxWidth) return CVS_E_BADARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CVS_E_HIP;  // no CPU fallback
    if (device < 0 || device >= ndev) return CVS_E_BADARG;
    if (hipSetDevice(device) != hipSuccess) return CVS_E_HIP;
    cvs_context* h = new (std::nothrow) cvs_context();
    if (!h) return CVS_E_NOMEM;
    h->kind = kind;
    h->width = width;
    h->spacing = spacing;
    h->nb = nb;
    h->device = device;
    std::memset(h->taps, 0, sizeof(h->taps));
    for (int i = 0; i < nb; ++i) host_make_taps(kind, i, width, spacing, h->taps[i]);
    // (nothing is allocated on the device here: the reference's callers build one short-lived object per image,
    // example/steer.cpp:86, and a hipMalloc + hipFree pair per object costs ~20 us of the ~150 us such an object lives;
    // the 8 bytes of min / max scratch are allocated by the first 8-bit conversion that needs them)
    const EnvOpts eo = env_opts();   // CVS_OPTS: process-wide A/B overrides for new handles
    if (eo.autotune >= 0) h->autotune = eo.autotune;
    if (eo.layout >= 0) h->layout = eo.layout;
    if (eo.pyr_strip >= 0) h->pyr_strip = eo.pyr_strip;
    *out = h;
    return CVS_OK;
}

int cvs_destroy(cvs_handle h)
{
    if (!h) return CVS_E_BADARG;
    (void)hipSetDevice(h->device);
    release_state(h);   // no drain: the block is parked with an event
    // staging memory exists only on handles that were given host planes, 8-bit conversions or irregular batches: those wait
    if (h->arena || h->frame_tab || h->point_out || h->u8_scr || h->hy_scr || h->cc_scr || h->ch_scr || h->ct_scr) (void)hipStreamSynchronize(h->stream);
    if (h->arena) (void)hipFree(h->arena);
    if (h->frame_tab) (void)hipFree(h->frame_tab);
    if (h->point_out) (void)hipFree(h->point_out);
    if (h->u8_scr) (void)hipFree(h->u8_scr);
    if (h->hy_scr) (void)hipFree(h->hy_scr);
    if (h->cc_scr) (void)hipFree(h->cc_scr);
    if (h->ch_scr) (void)hipFree(h->ch_scr);
    if (h->ct_scr) (void)hipFree(h->ct_scr);
    if (h->ev_order) (void)hipEventDestroy(h->ev_order);
    for (hipEvent_t e : h->band_ev) (void)hipEventDestroy(e);
    if (h->s_up) (void)hipStreamDestroy(h->s_up);
    if (h->s_down) (void)hipStreamDestroy(h->s_down);
    delete h;
    return CVS_OK;
}

int cvs_release_cached_memory(void)
{
    pool_release_all();
    return CVS_OK;
}

const char* cvs_last_error(cvs_handle h) { return h ? h->err.c_str() : "null handle"; }

int cvs_set_stream(cvs_handle h, void* s)
{
    if (!h) return CVS_E_BADARG;
    hipStream_t ns = static_cast<hipStream_t>(s);
    if (ns == h->stream) return CVS_OK;
    // The handle's state block, staging arena and frame table are reused from call to call: work already queued
    // on the old stream must finish before the new stream touches them.  One event, recorded on the old stream and
    // waited for by the new one (no host synchronisation); skipped while either stream is being captured.
    hipStreamCaptureStatus c0 = hipStreamCaptureStatusNone, c1 = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(h->stream, &c0);
    (void)hipStreamIsCapturing(ns, &c1);
    (void)hipGetLastError();
    if (h->used && c0 == hipStreamCaptureStatusNone && c1 == hipStreamCaptureStatusNone) {
        HIP_TRY(h, hipSetDevice(h->device));
        if (!h->ev_order) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_order, hipEventDisableTiming));
        HIP_TRY(h, hipEventRecord(h->ev_order, h->stream));
        HIP_TRY(h, hipStreamWaitEvent(ns, h->ev_order, 0));
    }
    h->stream = ns;
    return CVS_OK;
}

int cvs_set_option(cvs_handle h, int option, int value)
{
    if (!h) return CVS_E_BADARG;
    switch (option) {
        case CVS_OPT_ATAN_MODE:
            if (value != 0 && value != 1) return fail(h, CVS_E_BADARG, "atan mode");
            h->atan_mode = value;
            return CVS_OK;
        case CVS_OPT_STRIP_ROWS:
            if (value < 0 || value > 1 << 20) return fail(h, CVS_E_BADARG, "strip rows");
            h->strip_rows = value;
            return CVS_OK;
        case CVS_OPT_FIND_ON:
            if (value != 0 && value != 1) return fail(h, CVS_E_BADARG, "find_on");
            h->find_on = value;
            return CVS_OK;
        case CVS_OPT_G4_EXTENSIONS:
            if (value != 0 && value != 1) return fail(h, CVS_E_BADARG, "g4 extensions");
            h->g4_ext = value;
            return CVS_OK;
        case CVS_OPT_PERSIST_STATE:
            if (value != 0 && value != 1) return fail(h, CVS_E_BADARG, "persist");
            h->persist = value;
            return CVS_OK;
        case CVS_OPT_AUTOTUNE:
            if (value != 0 && value != 1) return fail(h, CVS_E_BADARG, "autotune");
            h->autotune = value;
            return CVS_OK;
        case CVS_OPT_BLOCK_ORDER:
            if (value != -1 && value != 0 && value != kOrderXcdColumns && value != kOrderDynamic) return fail(h, CVS_E_BADARG, "block order");
            h->block_order = value;
            return CVS_OK;
        case CVS_OPT_HOST_OVERLAP:
            if (value != 0 && value != 1) return fail(h, CVS_E_BADARG, "host overlap");
            h->host_overlap = value;
            return CVS_OK;
        case CVS_OPT_STATE_LAYOUT:
            if (value < 0 || value > 3) return fail(h, CVS_E_BADARG, "state layout");
            h->layout = value;
            return CVS_OK;
    }
    return fail(h, CVS_E_BADARG, "unknown option");
}

int cvs_get_option(cvs_handle h, int option, int* value)
{
    if (!h || !value) return CVS_E_BADARG;
    switch (option) {
        case CVS_OPT_ATAN_MODE: *value = h->atan_mode; return CVS_OK;
        case CVS_OPT_STRIP_ROWS: *value = h->strip_rows; return CVS_OK;
        case CVS_OPT_FIND_ON: *value = h->find_on; return CVS_OK;
        case CVS_OPT_BLOCK_ORDER: *value = h->block_order; return CVS_OK;
        case CVS_OPT_HOST_OVERLAP: *value = h->host_overlap; return CVS_OK;
        case CVS_OPT_AUTOTUNE: *value = h->autotune; return CVS_OK;
        case CVS_OPT_PERSIST_STATE: *value = h->persist; return CVS_OK;
        case CVS_OPT_G4_EXTENSIONS: *value = h->g4_ext; return CVS_OK;
        case CVS_OPT_STATE_LAYOUT: *value = h->layout; return CVS_OK;
    }
    return fail(h, CVS_E_BADARG, "unknown option");
}

int cvs_get_launch_info(cvs_handle h, cvs_launch_info* out)
{
    if (!h || !out) return CVS_E_BADARG;
    const uint32_t n = out->struct_size;   // the caller's sizeof(cvs_launch_info): never write beyond it
    if (n < sizeof(uint32_t)) return fail(h, CVS_E_BADARG, "cvs_launch_info.struct_size not set");
    cvs_launch_info li = h->last;
    li.struct_size = (uint32_t)std::min<size_t>(n, sizeof(li));
    std::memcpy(out, &li, li.struct_size);
    return CVS_OK;
}

int cvs_taps(cvs_handle h, int idx, float* out)
{
    if (!h || !out || idx < 0 || idx >= h->nb) return CVS_E_BADARG;
    std::memcpy(out, h->taps[idx], (2 * h->width + 1) * sizeof(float));
    return CVS_OK;
}

int cvs_kind(cvs_handle h, int* kind, int* width, float* spacing)
{
    if (!h) return CVS_E_BADARG;
    if (kind) *kind = h->kind;
    if (width) *width = h->width;
    if (spacing) *spacing = h->spacing;
    return CVS_OK;
}

int cvs_shape(cvs_handle h, int* rows, int* cols)
{
    if (!h) return CVS_E_BADARG;
    if (rows) *rows = h->have_basis ? h->rows : 0;
    if (cols) *cols = h->have_basis ? h->cols : 0;
    return CVS_OK;
}

int cvs_sync(cvs_handle h)
{
    if (!h) return CVS_E_BADARG;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return CVS_OK;
}

int cvs_setup(cvs_handle h, const cvs_plane* image, unsigned flags)
{
    return do_setup(h, SetupReq{image, flags});
}

int cvs_setup_steer(cvs_handle h, const cvs_plane* image, unsigned flags, float theta, const cvs_plane* g, const cvs_plane* hq)
{
    SetupReq rq{image, flags};
    rq.steer = true;
    rq.theta = theta;
    rq.g = g;
    rq.hq = hq;
    return do_setup(h, rq);
}

int cvs_setup_pyr(cvs_handle h, const cvs_plane* image, unsigned flags, const cvs_plane* next_level)
{
    if (!h) return CVS_E_BADARG;
    if (!next_level) return fail(h, CVS_E_BADARG, "next_level");
    SetupReq rq{image, flags};
    rq.pyr = next_level;
    return do_setup(h, rq);
}

// BASELINE config 3 in one call: filter every level of a Gaussian pyramid and build the pyramid on the way -- the filter launch
// of level k writes level k + 1 (cvs_setup_pyr: every level image is read once), all on the handles' stream.
// (Measured and NOT done, round 4: filtering the three small levels of a 5-level pyramid of 8192^2 concurrently on side streams
// behind the 4096^2 level -- 57 us of launch-latency-bound launches that could shrink to the longest of them.  The events
// that fork and join the streams cost more than the overlap saves: 0.603 ms against 0.525 ms for the plain chain, same box
// and process.  Nor: ONE launch for the three small levels (grid.z = level, per-level geometry) behind two stand-alone pyrDown
// launches that make their images first: 0.560 ms against 0.545 ms -- what the merged launch saves, the two extra launches
// and the loss of the fused level emission cost again.)
int cvs_pyramid_setup(cvs_handle* hs, int levels, const cvs_plane* image, unsigned flags, const cvs_plane* level_images)
{
    if (!hs || levels < 1 || !hs[0]) return CVS_E_BADARG;
    cvs_handle h0 = hs[0];
    if (!image || (levels > 1 && !level_images)) return fail(h0, CVS_E_BADARG, "image / level_images");
    for (int l = 0; l < levels; ++l) {
        if (!hs[l]) return fail(h0, CVS_E_BADARG, "null level handle");
        if (hs[l]->stream != h0->stream || hs[l]->device != h0->device) return fail(h0, CVS_E_BADARG, "the level handles must share one device and one stream");
        for (int m = 0; m < l; ++m)
            if (hs[m] == hs[l]) return fail(h0, CVS_E_BADARG, "one handle per level");
    }
    auto level_src = [&](int l) { return l == 0 ? image : &level_images[l - 1]; };
    int rc;
    for (int l = 0; l + 1 < levels; ++l) {
        const cvs_plane* s = level_src(l);
        if ((rc = check_plane(h0, &level_images[l], "level image")) || (rc = check_same(h0, &level_images[l], (s->rows + 1) / 2, (s->cols + 1) / 2))) return rc;
    }
    for (int l = 0; l < levels; ++l) {
        SetupReq rq{level_src(l), flags};
        rq.pyr = l + 1 < levels ? &level_images[l] : nullptr;
        rc = do_setup(hs[l], rq);
        if (rc) {
            if (hs[l] != h0) h0->err = hs[l]->err;
            return rc;
        }
    }
    return CVS_OK;
}

int cvs_setup_rows(cvs_handle h, const cvs_plane* image, unsigned flags, int row_lo, int row_hi)
{
    if (!h) return CVS_E_BADARG;
    if (!image || row_lo < 0 || row_hi > image->rows || row_lo >= row_hi) return fail(h, CVS_E_BADARG, "row range");
    if ((flags & CVS_SETUP_ORIENT) && h->kind == CVS_KIND_G4) return fail(h, CVS_E_UNSUPPORTED, "row ranges cover the basis planes only for G4");
    SetupReq rq{image, flags};
    rq.out_row_lo = row_lo;
    rq.out_row_hi = row_hi;
    return do_setup(h, rq);
}

static int state_index(cvs_handle h, int which)
{
    if (which >= CVS_PLANE_BASIS0 && which < CVS_PLANE_BASIS0 + h->nb) return which - CVS_PLANE_BASIS0;
    if (which >= CVS_PLANE_C1 && which <= CVS_PLANE_STRENGTH) return h->nb + (which - CVS_PLANE_C1);
    return -1;
}

int cvs_state_plane(cvs_handle h, int which, cvs_plane* view)
{
    if (!h || !view) return CVS_E_BADARG;
    const int idx = state_index(h, which);
    if (idx < 0) return fail(h, CVS_E_BADARG, "unknown state plane");
    int rc = need_state(h, idx >= h->nb);
    if (rc) return rc;
    view->data = state_plane(h, idx);
    view->rows = h->rows;
    view->cols = h->cols;
    view->step = state_group(h, idx).pitch * sizeof(float);
    view->mem = CVS_MEM_DEVICE;
    return CVS_OK;
}

int cvs_read_state(cvs_handle h, int which, const cvs_plane* dst)
{
    cvs_plane src;
    int rc = cvs_state_plane(h, which, &src);
    if (rc) return rc;
    if ((rc = check_plane(h, dst, "dst")) || (rc = check_same(h, dst, h->rows, h->cols))) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t width = (size_t)h->cols * sizeof(float);
    if (dst->mem == CVS_MEM_HOST && src.step != width && dst->step == width) {
        // a plane of a row-interleaved group on its way to a dense host plane: over the host link a pitched 2-D copy is served
        // row by row at a fraction of the rate of a linear one (cvs_context.h copy_rows), so the rows are gathered on the
        // device first (a device-to-device 2-D copy runs at memory speed) and cross the link as one linear copy
        const size_t elems = (size_t)h->rows * h->cols;
        if ((rc = arena_reserve(h, round_up(elems, 64)))) return rc;
        HIP_TRY(h, hipMemcpy2DAsync(h->arena, width, src.data, src.step, width, h->rows, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(dst->data, h->arena, width * h->rows, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return CVS_OK;
    }
    HIP_TRY(h, copy_rows(dst->data, dst->step, src.data, src.step, width, h->rows,
                                dst->mem == CVS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->stream));
    if (dst->mem == CVS_MEM_HOST) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return CVS_OK;
}

int cvs_steer_scalar(cvs_handle h, float theta, const cvs_plane* g, const cvs_plane* hq, const cvs_plane* e,
                     const cvs_plane* mag, const cvs_plane* phase)
{
    if (!h) return CVS_E_BADARG;
    return steer_common(h, false, theta, nullptr, g, hq, e, mag, phase);
}

int cvs_steer_map(cvs_handle h, const cvs_plane* theta, const cvs_plane* g, const cvs_plane* hq, const cvs_plane* e,
                  const cvs_plane* mag, const cvs_plane* phase)
{
    if (!h) return CVS_E_BADARG;
    return steer_common(h, true, 0.f, theta, g, hq, e, mag, phase);
}

static void bank_angle(cvs_handle h, BankArgs& a, int t, float theta)
{
    host_steer_weights(h->kind, theta, a.w[t]);
    // G2.cpp:162: float c2t(std::cos(theta * 2.0)) -- double argument, narrowed (steer_common)
    a.c2t[t] = (float)std::cos((double)theta * 2.0);
    a.s2t[t] = (float)std::sin((double)theta * 2.0);
}

int cvs_steer_bank(cvs_handle h, const float* thetas, int n, const cvs_plane* outs)
{
    if (!h) return CVS_E_BADARG;
    if (n <= 0 || !thetas || !outs) return fail(h, CVS_E_BADARG, "n > 0 angles, thetas and outs are required");
    int rc = need_state(h, false);
    if (rc) return rc;
    // kind o (g, h, e, magnitude, phase) is written when angle 0's plane has data -- and then for every angle
    bool want[5], any = false;
    for (int o = 0; o < 5; ++o) any |= (want[o] = outs[o].data != nullptr);
    if (!any) return fail(h, CVS_E_BADARG, "no output requested");
    for (int t = 0; t < n; ++t)
        for (int o = 0; o < 5; ++o) {
            const cvs_plane* p = &outs[5 * (size_t)t + o];
            if ((p->data != nullptr) != want[o]) return fail(h, CVS_E_BADARG, "an output kind is requested for some angles but not for others");
            if (want[o] && ((rc = check_plane(h, p, "plane")) || (rc = check_same(h, p, h->rows, h->cols)))) return rc;
        }
    if (h->kind == CVS_KIND_G4 && (want[2] || want[3] || want[4]) && !h->g4_ext)
        return fail(h, CVS_E_UNSUPPORTED, "G4 has no energy / magnitude / phase in the reference (G4.cpp:88-90); see CVS_OPT_G4_EXTENSIONS");
    if (want[2] && (rc = need_state(h, true))) return rc;
    // no two written planes may share memory (the per-pixel rule; the state planes are the engine's own)
    std::vector<const cvs_plane*> all;
    for (int t = 0; t < n; ++t)
        for (int o = 0; o < 5; ++o)
            if (want[o]) all.push_back(&outs[5 * (size_t)t + o]);
    for (size_t i = 0; i < all.size(); ++i)
        for (size_t j = i + 1; j < all.size(); ++j)
            if (planes_overlap(all[i], all[j])) return fail(h, CVS_E_BADARG, "two output planes overlap each other");

    BankArgs a{};
    a.rows = h->rows;
    a.cols = h->cols;
    a.atan_mode = h->atan_mode;
    a.nt_stores = use_nt_stores(h, (size_t)a.rows * a.cols);
    a.nt_loads = a.nt_stores;   // as cvs_steer_scalar: the state planes of an image that large are not cache-resident
    if (!bank_inputs(h, want[2], a.in)) return fail(h, CVS_E_STATE, "state planes not at a constant stride within their group");

    // one launch per kBankMax angles when every written plane is a device plane and each kind's planes lie at one pitch and a
    // constant stride (a [K][H][W] or [H][K][W] block, what the Python side allocates)
    // (each kind has a stride of its own: >= 0 and a whole number of floats)
    bool one = true;
    for (const cvs_plane* p : all) one = one && mem_of(p) == CVS_MEM_DEVICE;
    for (int o = 0; o < 5 && one; ++o) {
        if (!want[o]) continue;
        const PlaneRun run = plane_run(n, 1, [&](int t, int) { return plane_at(outs[5 * (size_t)t + o]); }, true, sizeof(float));
        one = run.ok;
        a.out[o] = {outs[o].data, outs[o].step / sizeof(float), (size_t)run.stride / sizeof(float)};
    }
    if (one) {
        Call c;
        if ((rc = begin(h, c, {}))) return rc;
        for (int t0 = 0; t0 < n; t0 += kBankMax) {
            BankArgs b = a;
            b.n = std::min(kBankMax, n - t0);
            for (int t = 0; t < b.n; ++t) bank_angle(h, b, t, thetas[t0 + t]);
            for (int o = 0; o < 5; ++o)
                if (b.out[o].p) b.out[o].p += (size_t)t0 * b.out[o].stride;
            HIP_TRY(h, launch_steer_bank(h->nb, b, h->stream));
        }
        return finish(c);
    }
    // anything else -- host planes, separate allocations, mixed pitches -- angle by angle, each a launch of one angle (host
    // planes staged and downloaded per angle, as cvs_steer_scalar does): the same values
    for (int t = 0; t < n; ++t) {
        const cvs_plane* p = &outs[5 * (size_t)t];
        const cvs_plane* q[5];
        for (int o = 0; o < 5; ++o) q[o] = want[o] ? &p[o] : nullptr;
        Call c;
        if ((rc = begin(h, c, {q[0], q[1], q[2], q[3], q[4]}))) return rc;
        BankArgs b = a;
        b.n = 1;
        bank_angle(h, b, 0, thetas[t]);
        for (int o = 0; o < 5; ++o) {
            PlaneRef r;
            if ((rc = out_ref(c, q[o], r))) return rc;
            b.out[o] = {r.p, r.pitch, 0};
        }
        HIP_TRY(h, launch_steer_bank(h->nb, b, h->stream));
        if ((rc = finish(c))) return rc;
    }
    return CVS_OK;
}

int cvs_steer_point(cvs_handle h, int x, int y, float theta, float out[5])
{
    if (!h || !out) return CVS_E_BADARG;
    if (h->kind != CVS_KIND_G2) return fail(h, CVS_E_UNSUPPORTED, "point steer exists for G2 only (G2.cpp:115-134)");
    int rc = need_state(h, false);
    if (rc) return rc;
    if (x < 0 || y < 0 || x >= h->cols || y >= h->rows) return fail(h, CVS_E_BADARG, "point outside the image");
    HIP_TRY(h, hipSetDevice(h->device));
    // the scalar weights are host math in the reference too (G2.cpp:118-120); the pixel arithmetic
    // runs on the device, next to the state it reads
    PointArgs a{};
    host_steer_weights(CVS_KIND_G2, theta, a.w);
    a.c2t = (float)std::cos((double)theta * 2.0);  // G2.cpp:132: std::cos(theta * 2.0), double argument
    a.s2t = (float)std::sin((double)theta * 2.0);
    if (!h->point_out) HIP_TRY(h, hipMalloc(&h->point_out, 8 * sizeof(float)));
    const cvs_context::PlaneGroup &gb = state_group(h, 0), &go = state_group(h, h->nb);
    HIP_TRY(h, launch_steer_point(state_plane(h, 0), gb.stride, (size_t)y * gb.pitch + x, h->have_orient ? state_plane(h, h->nb) : nullptr,
                                  go.stride, (size_t)y * go.pitch + x, a, h->point_out, h->stream));
    HIP_TRY(h, hipMemcpyAsync(out, h->point_out, 5 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return CVS_OK;
}

int cvs_mag_phase(cvs_handle h, const cvs_plane* g, const cvs_plane* hq, const cvs_plane* mag, const cvs_plane* phase)
{
    if (!h) return CVS_E_BADARG;
    int rc;
    if ((rc = check_plane(h, g, "g")) || (rc = check_plane(h, hq, "hq"))) return rc;
    if (!mag && !phase) return fail(h, CVS_E_BADARG, "no output requested");
    for (const cvs_plane* p : {hq, mag, phase}) {
        if (!p) continue;
        if ((rc = check_plane(h, p, "plane")) || (rc = check_same(h, p, g->rows, g->cols))) return rc;
    }
    if ((rc = check_point_overlaps(h, {g, hq}, {mag, phase}))) return rc;
    Call c;
    if ((rc = begin(h, c, {g, hq, mag, phase}))) return rc;
    PointArgs a{};
    a.rows = g->rows;
    a.cols = g->cols;
    a.atan_mode = h->atan_mode;
    if ((rc = in_ref(c, g, a.in[0])) || (rc = in_ref(c, hq, a.in[1]))) return rc;
    if ((rc = out_ref(c, mag, a.out[0])) || (rc = out_ref(c, phase, a.out[1]))) return rc;
    a.nt_stores = use_nt_stores(h, (size_t)a.rows * a.cols);
    HIP_TRY(h, launch_point(OP_MAG_PHASE, a, h->stream));
    return finish(c);
}

int cvs_phase_weights(cvs_handle h, const cvs_plane* phase, const cvs_plane* lambda, float phi, int signum, float k)
{
    (void)k;  // accepted and ignored, like the reference (G2.cpp:179-186)
    if (!h) return CVS_E_BADARG;
    int rc;
    if ((rc = check_plane(h, phase, "phase")) || (rc = check_plane(h, lambda, "lambda"))) return rc;
    if ((rc = check_same(h, lambda, phase->rows, phase->cols))) return rc;
    if ((rc = check_point_overlaps(h, {phase}, {lambda}))) return rc;
    Call c;
    if ((rc = begin(h, c, {phase, lambda}))) return rc;
    PointArgs a{};
    a.rows = phase->rows;
    a.cols = phase->cols;
    a.phi = phi;
    a.signum = signum ? 1 : 0;
    if ((rc = in_ref(c, phase, a.in[0])) || (rc = out_ref(c, lambda, a.out[0]))) return rc;
    a.nt_stores = use_nt_stores(h, (size_t)a.rows * a.cols);
    HIP_TRY(h, launch_point(OP_PHASE_WEIGHTS, a, h->stream));
    return finish(c);
}

int cvs_wrap(cvs_handle h, const cvs_plane* angle, const cvs_plane* out)
{
    if (!h) return CVS_E_BADARG;
    int rc;
    if ((rc = check_plane(h, angle, "angle")) || (rc = check_plane(h, out, "out"))) return rc;
    if ((rc = check_same(h, out, angle->rows, angle->cols))) return rc;
    if ((rc = check_point_overlaps(h, {angle}, {out}))) return rc;
    Call c;
    if ((rc = begin(h, c, {angle, out}))) return rc;
    PointArgs a{};
    a.rows = angle->rows;
    a.cols = angle->cols;
    if ((rc = in_ref(c, angle, a.in[0])) || (rc = out_ref(c, out, a.out[0]))) return rc;
    a.nt_stores = use_nt_stores(h, (size_t)a.rows * a.cols);
    HIP_TRY(h, launch_point(OP_WRAP, a, h->stream));
    return finish(c);
}

int cvs_find(cvs_handle h, const cvs_plane* e, const cvs_plane* phase, const cvs_plane* edges, const cvs_plane* dark,
             const cvs_plane* bright)
{
    if (!h) return CVS_E_BADARG;
    int rc;
    if ((rc = check_plane(h, e, "e")) || (rc = check_plane(h, phase, "phase"))) return rc;
    if (!edges && !dark && !bright) return fail(h, CVS_E_BADARG, "no output requested");
    for (const cvs_plane* p : {phase, edges, dark, bright}) {
        if (!p) continue;
        if ((rc = check_plane(h, p, "plane")) || (rc = check_same(h, p, e->rows, e->cols))) return rc;
    }
    if ((rc = check_point_overlaps(h, {e, phase}, {edges, dark, bright}))) return rc;
    Call c;
    if ((rc = begin(h, c, {e, phase, edges, dark, bright}))) return rc;
    PointArgs a{};
    a.rows = e->rows;
    a.cols = e->cols;
    if ((rc = in_ref(c, e, a.in[0])) || (rc = in_ref(c, phase, a.in[1]))) return rc;
    if ((rc = out_ref(c, edges, a.out[0])) || (rc = out_ref(c, dark, a.out[1])) || (rc = out_ref(c, bright, a.out[2]))) return rc;
    a.nt_stores = use_nt_stores(h, (size_t)a.rows * a.cols);
    HIP_TRY(h, launch_point(OP_FIND, a, h->stream));
    return finish(c);
}

int cvs_set_u8_gain(cvs_handle h, float gain)
{
    if (!h) return CVS_E_BADARG;
    if (!(gain >= 0.f)) return fail(h, CVS_E_BADARG, "u8 gain: 0 (normalise) or > 0 (convertTo)");   // (NaN fails the test as well)
    h->u8_gain = gain;
    return CVS_OK;
}

int cvs_get_u8_gain(cvs_handle h, float* gain)
{
    if (!h || !gain) return CVS_E_BADARG;
    *gain = h->u8_gain;
    return CVS_OK;
}

int cvs_select_frame(cvs_handle h, int frame)
{
    if (!h) return CVS_E_BADARG;
    if (frame < 0 || frame >= h->num_frames) return fail(h, CVS_E_BADARG, "frame index");
    h->cur_frame = frame;
    return CVS_OK;
}

int cvs_num_frames(cvs_handle h, int* n)
{
    if (!h || !n) return CVS_E_BADARG;
    *n = h->have_basis ? h->num_frames : 0;
    return CVS_OK;
}

int cvs_pyr_down(cvs_handle h, const cvs_plane* src, const cvs_plane* dst)
{
    if (!h) return CVS_E_BADARG;
    int rc;
    if ((rc = check_plane(h, src, "src")) || (rc = check_plane(h, dst, "dst"))) return rc;
    if ((rc = check_same(h, dst, (src->rows + 1) / 2, (src->cols + 1) / 2))) return rc;
    if (planes_overlap(src, dst)) return fail(h, CVS_E_BADARG, "the level overlaps the image it is made from");
    Call c;
    if ((rc = begin(h, c, {src, dst}))) return rc;
    PlaneRef in, out;
    if ((rc = in_ref(c, src, in)) || (rc = out_ref(c, dst, out))) return rc;
    hipError_t pe = hipSuccess;
    if (h->pyr_strip && launch_pyr_strip(in.p, in.pitch, src->rows, src->cols, out.p, out.pitch, h->stream, &pe)) HIP_TRY(h, pe);
    else HIP_TRY(h, launch_pyr_down(in.p, in.pitch, src->rows, src->cols, out.p, out.pitch, h->stream));
    return finish(c);
}

}  // extern "C"
