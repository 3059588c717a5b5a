// cvs_pipeline.cpp -- the caller pipeline (cvs_pipeline, cvs_pipeline_batch), its 8-bit routes and the 8-bit conversions they are built
// on.  Which launches a call becomes is decided here, from how the caller's planes lie in memory (cvs_layout.h).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <vector>

#include "cvs_context.h"
#include "cvs_layout.h"

using namespace cvs;

namespace {

// the flat [n][8] table of optional outputs (a plane without data is not requested; the table may be absent): plane k of frame i, and
// frame i's eight as pointers
PlaneAt out_at(const cvs_plane* outs, int i, int k) { return outs ? plane_at(outs[(size_t)i * 8 + k]) : PlaneAt{0, 0}; }
void frame_outs(const cvs_plane* outs, int i, const cvs_plane* po[8])
{
    for (int k = 0; k < 8; ++k) po[k] = (outs && outs[(size_t)i * 8 + k].data) ? &outs[(size_t)i * 8 + k] : nullptr;
}

// what every launch of the G4 per-pixel stage (k_g4_pipeline) is told alike: geometry, modes and the eleven basis planes of `nframes`
// frames from the current frame on
void g4_pipe_args(cvs_handle h, int nframes, G4PipeArgs& a)
{
    a.rows = h->rows;
    a.cols = h->cols;
    a.frames = nframes;
    a.atan_mode = h->atan_mode;
    a.find_on_e = h->find_on;
    for (int p = 0; p < h->nb; ++p) {
        const PlaneRef r = state_ref(h, p);
        a.in[p] = {r.p, r.pitch, h->frame_stride};
    }
    a.nt_stores = use_nt_stores(h, (size_t)a.rows * a.cols * nframes);
    a.nt_loads = a.nt_stores;   // the basis planes of an image that large are not cache-resident and are read once here
}

// G4 caller pipeline (CVS_OPT_G4_EXTENSIONS), second stage: the pair launches have written the basis planes of `nframes` frames
// from the current frame on; ONE per-pixel launch (k_g4_pipeline, blockIdx.z = frame) writes the orientation planes (state kept
// only) and the requested outputs -- outs[k] is frame 0's plane k, frame z's lies out_fstride elements further (device planes;
// host planes only with nframes = 1).  The values are those of setup(FULL) + steer_map(NULL, ...) + find(...), bit for bit.
int g4_pipe_stage(cvs_handle h, const cvs_plane* const outs[8], int nframes, size_t out_fstride)
{
    Call c;
    int rc = begin(h, c, {outs[0], outs[1], outs[2], outs[3], outs[4], outs[5], outs[6], outs[7]});
    if (rc) return rc;
    G4PipeArgs a{};
    g4_pipe_args(h, nframes, a);
    if (h->persist) {   // c1, c2, c3, theta, strength: the state setup(FULL) leaves behind
        for (int i = 0; i < 5; ++i) {
            const PlaneRef r = state_ref(h, h->nb + i);
            a.out[G4P_C1 + i] = {r.p, r.pitch, h->frame_stride};
        }
    }
    for (int k = 0; k < 8; ++k) {
        PlaneRef r;
        if ((rc = out_ref(c, outs[k], r))) return rc;
        a.out[G4P_G + k] = {r.p, r.pitch, out_fstride};
    }
    HIP_TRY(h, launch_g4_pipeline(a, h->stream));
    // CVS_OPT_PERSIST_STATE = 0: the basis planes were scratch for this call, nothing addressable is left
    h->have_basis = h->have_orient = h->persist != 0;
    return finish(c);
}

// the pair launch of a basis-only setup of frame `frame` of `nframes` -- the tuner key of cvs_setup(BASIS)
int g4_basis_frame(cvs_handle h, const cvs_plane* image, int nframes, int frame)
{
    SetupReq rq{image, CVS_SETUP_BASIS};
    rq.nframes = nframes;
    rq.frame = frame;
    return do_setup(h, rq);
}

// one G4 image (frame `frame` of `nframes`): the pair launch and the stage
int g4_pipeline_one(cvs_handle h, const cvs_plane* image, const cvs_plane* const outs[8], int nframes, int frame)
{
    const int rc = g4_basis_frame(h, image, nframes, frame);
    return rc ? rc : g4_pipe_stage(h, outs, 1, 0);
}

// G4 frame batch (cvs_pipeline_batch, arguments checked).  f32 device frames whose outputs lie at one constant frame stride (an
// [n, K, H, W] block, the usual case): one pair launch per frame, each writing its frame's state block, then ONE per-pixel launch
// over all frames.  Anything else -- host or 8-bit frames, outputs anywhere -- goes frame by frame.
int g4_pipeline_frames(cvs_handle h, const cvs_plane* images, int n, const cvs_plane* outs, bool all_dev)
{
    // (a stride of 0 would have every frame write the same planes: refused here, while the regular block of batch_run takes it)
    const PlaneRun run = plane_run(n, 8, [&](int i, int k) { return out_at(outs, i, k); }, false);
    const bool block = all_dev && run.ok;
    const cvs_plane* po[8];
    for (int i = 0; i < n; ++i) {
        frame_outs(outs, i, po);
        if (const int rc = block ? g4_basis_frame(h, &images[i], n, i) : g4_pipeline_one(h, &images[i], po, n, i)) return rc;
    }
    h->cur_frame = 0;
    if (!block) return CVS_OK;
    frame_outs(outs, 0, po);
    return g4_pipe_stage(h, po, n, (size_t)run.stride / sizeof(float));
}

// cvs_pipeline_batch with checked arguments.  u8 (the three-maps launch with 8-bit outputs, G2): mode 1 = `outs` holds the caller's byte
// planes, mode 2 = f32 scratch planes; kNotFused = the call would not be ONE such launch, nothing was launched.
int batch_run(cvs_handle h, const cvs_plane* images, int n, const cvs_plane* outs, const U8Req* u8)
{
    int rc;
    const int rows = images[0].rows, cols = images[0].cols;
    bool ins_dev = true, outs_dev = true;
    size_t max_bytes = 0;
    for (int i = 0; i < n; ++i) {
        ins_dev = ins_dev && images[i].mem == CVS_MEM_DEVICE;  // f32 on the device; 8-bit / host frames go frame by frame
        if (!is_u8(&images[i])) max_bytes = std::max(max_bytes, (size_t)rows * images[i].step);
        for (int k = 0; outs && k < 8; ++k) {
            const cvs_plane* o = &outs[(size_t)i * 8 + k];
            if (!o->data) continue;
            outs_dev = outs_dev && mem_of(o) == CVS_MEM_DEVICE;
            max_bytes = std::max(max_bytes, (size_t)rows * o->step);
        }
    }
    if (h->kind == CVS_KIND_G4) return g4_pipeline_frames(h, images, n, outs, ins_dev && outs_dev);
    // gain mode: the outputs are the caller's byte planes of the three maps (pitches, offsets and strides in bytes) and must be ONE
    // resource per frame -- frame 0's planes within 2 GiB of the lowest, a common row step -- with every frame strictly behind the one
    // before.  f32 outputs: a stride of 0 (every frame the same planes) counts as regular, which g4_pipeline_frames refuses.
    const bool gain = u8 && u8->mode == 1;
    const size_t out_unit = gain ? 1 : sizeof(float);
    PlaneAt out0[8];
    for (int k = 0; k < 8; ++k) out0[k] = out_at(outs, 0, k);
    const OneResource res = one_resource(out0, rows, kMaxResourceBytes);
    const PlaneRun out_run = plane_run(n, 8, [&](int i, int k) { return out_at(outs, i, k); }, !gain);
    if (gain && (!res.ok || !out_run.ok)) return kNotFused;
    // the frames themselves: one row step, one stride >= 0 (f32 or bytes alike)
    const PlaneRun in_run = plane_run(n, 1, [&](int i, int) { return plane_at(images[i]); }, true);
    // 8-bit frames that lie back to back on the device (a driver's upload of a block of byte images): the one-launch path
    // below reads the bytes itself (BasisArgs::in_u8), like any regular f32 batch -- no widened copy
    const size_t u8_frame = (size_t)rows * images[0].step;
    bool u8_batch = images[0].mem == (CVS_MEM_DEVICE | CVS_DEPTH_U8) && in_run.ok && (n == 1 || (size_t)in_run.stride == u8_frame) &&
                    u8_frame <= kMaxResourceBytes;
    for (int i = 1; i < n && u8_batch; ++i) u8_batch = images[i].mem == images[0].mem;
    const size_t pitch = round_up((size_t)cols, 64);
    // one launch over grid.z needs every plane below 2 GiB (huge frames are filtered in row bands, frame by frame)
    const bool small_planes = std::max(max_bytes, (size_t)rows * pitch * sizeof(float)) <= kMaxResourceBytes;
    // ... and a grid inside the bounds of cvs_grid.h whatever order and strip height the launch ends up with (very tall frames, or
    // more than 65534 of them: frame by frame as well)
    const bool fast = (ins_dev || u8_batch) && outs_dev && small_planes && strip_batch_fits(rows, cols, h->strip_rows > 0 ? h->strip_rows : 1, n) &&
                      !basis_may_need_scratch(h->kind, h->width, h->taps, rows, cols, std::max(pitch, max_bytes / sizeof(float) / rows));
    if (!fast && u8) return kNotFused;
    if (!fast) {
        // host planes, tiny or huge images, non-default taps: frame by frame through the single-image path
        for (int i = 0; i < n; ++i) {
            const cvs_plane* po[8];
            frame_outs(outs, i, po);
            SetupReq rq{&images[i], CVS_SETUP_FULL};
            rq.pipe_outs = po;
            rq.nframes = n;
            rq.frame = i;
            if ((rc = do_setup(h, rq))) return rc;
        }
        h->cur_frame = 0;
        return CVS_OK;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    h->used = true;
    h->have_basis = h->have_orient = false;
    if ((rc = ensure_state(h, rows, cols, n))) return rc;
    h->cur_frame = 0;
    auto out_ref_of = [&](int i, int k) {   // (f32 outputs only: the byte planes of the gain mode go through the resource)
        const cvs_plane* o = outs && !gain ? &outs[(size_t)i * 8 + k] : nullptr;
        return (o && o->data) ? PlaneRef{o->data, o->step / sizeof(float)} : PlaneRef{nullptr, 0};
    };
    const size_t in_unit = u8_batch ? 1 : sizeof(float);   // pitch and stride of the frames in elements of the image's own type
    // Regularly strided frames -- one [n, H, W] block in, one [n, K, H, W] block out, the usual case -- need no
    // table: frame z is frame 0 plus z strides, computed in the kernel from its arguments.  Anything else (a list
    // of unrelated planes) goes through a device table, uploaded on the handle's stream.
    const bool regular = in_run.ok && out_run.ok;
    if (!regular && u8) return kNotFused;
    if (!regular) {
        std::vector<BatchFrame> tab(n);
        for (int i = 0; i < n; ++i) {
            tab[i].in = images[i].data;
            tab[i].in_pitch = images[i].step / in_unit;
            for (int k = 0; k < 8; ++k) tab[i].out[k] = out_ref_of(i, k);
        }
        if ((rc = grow_scratch(h, "hipMalloc(&h->frame_tab, (size_t)n * sizeof(BatchFrame))", h->frame_tab, h->frame_tab_cap, n, sizeof(BatchFrame)))) return rc;
        // pageable source: the runtime stages it before returning, so `tab` may go out of scope
        HIP_TRY(h, hipMemcpyAsync(h->frame_tab, tab.data(), (size_t)n * sizeof(BatchFrame), hipMemcpyHostToDevice, h->stream));
    }
    BasisArgs a{};
    a.rows = rows;
    a.cols = cols;
    a.in_pitch = pitch;
    a.in_u8 = u8_batch ? 1 : 0;
    if (regular) {
        a.batch_regular = 1;
        a.in = images[0].data;
        a.in_pitch = images[0].step / in_unit;
        a.in_frame_stride = (size_t)in_run.stride / in_unit;
        a.out_frame_stride = (size_t)out_run.stride / out_unit;
        for (int k = 0; k < 8; ++k) a.pipe_out[k] = out_ref_of(0, k);
        // one buffer resource per frame for all outputs, if frame 0's outputs share a pitch and lie within 2 GiB
        if (res.ok) {
            a.out_one = 1;
            a.out_mask = res.mask;
            a.out_base = reinterpret_cast<float*>(res.base);
            a.out_pitch = res.step / out_unit;
            a.out_bytes = res.span;
            for (int k = 0; k < 8; ++k) a.out_off[k] = res.off[k];
        }
    }
    fill_state_args(h, a, true);   // frame 0 (cur_frame was reset above); frame z adds z * frame_stride in the kernel
    a.atan_mode = h->atan_mode;
    a.strip_rows = default_strip_rows(h, rows, cols);
    a.block_order = h->block_order >= 0 ? h->block_order : 0;   // the default's order (default_config)
    a.nt_stores = use_nt_stores(h, (size_t)rows * cols * n);
    a.pipe = 1;
    a.no_state = h->persist ? 0 : 1;
    a.find_on_e = h->find_on;
    a.frames = regular ? nullptr : h->frame_tab;
    a.batch = n;
    // state kept: frames from the two halves of the batch in flight together (see k_basis); the stateless launch is bound by
    // the SIMDs and does not care.  CVS_OPTS batch_ways=<n> is a tuning aid (1 = frames in order).
    a.z_ways = (!a.no_state && n >= 4) ? 2 : 1;
    // ... and on 10-row strips: round 3 sweep (profiles/r03_c4_strip_probe.txt), 32 x 1080p, five state blocks of the allocation lottery, one handle
    // each: against 19 rows in the plain order 0.634 / 0.70 / 0.70 / 0.796 / 0.795 for 0.644 / 0.70 / 0.70 / 0.762 / 0.764 --
    // level on the slow and middle blocks, +4.5 % on the fast ones
    if (!a.no_state && n >= 4 && h->strip_rows <= 0) a.strip_rows = 2 * (2 * h->width + 1) - 2 * h->width;
    if (const int ways = env_opts().batch_ways; ways > 0) a.z_ways = std::max(1, std::min(n, ways));
    a.frame_stride = h->frame_stride;
    // state kept: every frame is a new image -- the waves of a frame's first row bands also request the rest of the FRAME (two bands each:
    // BasisArgs::warm_k, per frame).  32 x 1080p, same handle, alternating, sustained: +1.2 ... +2.3 % in 7 of 7 processes on three boxes
    // (four bands +1.3 %, eight +0.3 %; profiles/r06_c4_warm.txt).  Not for the outputs-only batches (-1 %: they are bound by the SIMDs).
    if (!a.no_state && regular && (size_t)rows * cols >= ((size_t)1 << 20)) a.warm_k = env_opts().warm >= 0 ? env_opts().warm : 2;
    if (u8) {
        a.u8_mode = u8->mode;
        a.u8_gain = u8->gain;
        a.u8_mm = u8->mm;
        if (!basis_u8_fusable(h->kind, h->width, h->taps, a)) return kNotFused;
        if (u8->mode == 2) HIP_TRY(h, launch_minmax_init_n(u8->mm, 3 * n, h->stream));
    }
    TuneToken tok;
    if ((rc = tune_begin(h, a, 16 | 1 | 4 | (a.no_state ? 8 : 0), false, tok))) return rc;
    note_launch(h, a);
    const hipError_t le = launch_basis(h->kind, h->width, h->taps, a, nullptr, h->stream);
    tune_end(h, tok);
    HIP_TRY(h, le);
    h->have_basis = h->have_orient = h->persist != 0;
    return CVS_OK;
}

int to_u8(cvs_handle h, const cvs_plane* src, uint8_t* dst, size_t dst_step, int dst_mem, bool minmax, float alpha, float beta)
{
    if (!h || !dst) return CVS_E_BADARG;
    int rc = check_plane(h, src, "src");
    if (rc) return rc;
    if (dst_step < (size_t)src->cols) return fail(h, CVS_E_SIZE, "dst_step");
    if (dst_mem != CVS_MEM_HOST && dst_mem != CVS_MEM_DEVICE) return fail(h, CVS_E_BADARG, "dst_mem");
    const size_t dpitch = round_up((size_t)src->cols, 256);
    const size_t u8_elems = dst_mem == CVS_MEM_HOST ? round_up(dpitch * src->rows / 4 + 64, 64) : 0;
    Call c;
    if ((rc = begin(h, c, {src}, u8_elems + (minmax ? 64 : 0)))) return rc;
    PlaneRef in;
    if ((rc = in_ref(c, src, in))) return rc;
    float* mm = minmax ? arena_take(h, 64) : nullptr;   // min / max scratch from the arena (no allocation of its own, cf. to_u8_batch)
    uint8_t* d = dst;
    size_t dstep = dst_step;
    if (dst_mem == CVS_MEM_HOST) {
        d = reinterpret_cast<uint8_t*>(arena_take(h, u8_elems));
        dstep = dpitch;
    }
    if (minmax) {
        HIP_TRY(h, launch_minmax(in.p, in.pitch, src->rows, src->cols, mm, h->stream));
        HIP_TRY(h, launch_quantize_u8(in.p, in.pitch, src->rows, src->cols, mm, d, dstep, h->stream));
    } else {
        HIP_TRY(h, launch_convert_u8(in.p, in.pitch, src->rows, src->cols, alpha, beta, d, dstep, h->stream));
    }
    if (dst_mem == CVS_MEM_DEVICE) return finish(c);
    HIP_TRY(h, copy_rows(dst, dst_step, d, dstep, (size_t)src->cols, src->rows, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return CVS_OK;
}

// n planes at once: one min/max launch, one quantise launch, the copies to the host queued behind them and ONE
// synchronisation -- what a driver wants that turns a rank's whole block of feature maps into files (per plane, the
// launch + copy + sync of the single-plane call costs more than the work).  Planes that are not equally sized device
// planes at a constant stride go one by one.
int to_u8_batch(cvs_handle h, const cvs_plane* src, int n, uint8_t* const* dst, size_t dst_step, int dst_mem, bool minmax, float alpha, float beta)
{
    if (!h || !src || !dst || n < 1) return CVS_E_BADARG;
    if (dst_mem != CVS_MEM_HOST && dst_mem != CVS_MEM_DEVICE) return fail(h, CVS_E_BADARG, "dst_mem");
    int rc;
    bool regular = true;
    for (int i = 0; i < n; ++i) {
        if ((rc = check_plane(h, &src[i], "src"))) return rc;
        if (!dst[i]) return fail(h, CVS_E_BADARG, "dst");
        regular = regular && src[i].mem == CVS_MEM_DEVICE && src[i].rows == src[0].rows && src[i].cols == src[0].cols;
    }
    if (dst_step < (size_t)src[0].cols) return fail(h, CVS_E_SIZE, "dst_step");
    // sources and destinations: one row step (the destinations share dst_step), one stride >= 0
    const PlaneRun srun = plane_run(n, 1, [&](int i, int) { return plane_at(src[i]); }, true);
    const PlaneRun drun = plane_run(n, 1, [&](int i, int) { return PlaneAt{reinterpret_cast<uintptr_t>(dst[i]), dst_step}; }, true);
    regular = regular && srun.ok && (size_t)src[0].rows * src[0].step <= kMaxResourceBytes;
    auto one_by_one = [&]() {
        for (int i = 0; i < n; ++i)
            if ((rc = to_u8(h, &src[i], dst[i], dst_step, dst_mem, minmax, alpha, beta))) return rc;
        return (int)CVS_OK;
    };
    if (!regular) return one_by_one();
    const int rows = src[0].rows, cols = src[0].cols;
    const size_t stride = (size_t)srun.stride / sizeof(float);
    HIP_TRY(h, hipSetDevice(h->device));
    h->used = true;
    // scratch: 2n floats of min / max, and (host destinations) n staged byte planes
    // host destinations that lie back to back ([n][rows][dst_step], the usual block) are staged in exactly that layout
    // and come down as ONE linear copy (a pitched 2-D copy of the same bytes runs at a third of the link rate)
    const bool packed = dst_mem == CVS_MEM_HOST && dst_step == (size_t)cols &&  // padded rows keep their padding: copied row by row
                        drun.ok && (n == 1 || (size_t)drun.stride == (size_t)rows * dst_step);
    const size_t dpitch = packed ? dst_step : round_up((size_t)cols, 256), plane_b = dpitch * rows;
    const size_t mm_elems = round_up((size_t)2 * n, 64);
    const size_t stage_elems = dst_mem == CVS_MEM_HOST ? round_up(plane_b * n / 4 + 64, 64) : 0;
    if ((rc = arena_reserve(h, mm_elems + stage_elems))) return rc;
    h->arena_used = 0;
    float* mm = arena_take(h, mm_elems);
    if (dst_mem == CVS_MEM_HOST) {
        uint8_t* stage = reinterpret_cast<uint8_t*>(arena_take(h, stage_elems));
        HIP_TRY(h, launch_to_u8_n(src[0].data, stride, src[0].step / sizeof(float), rows, cols, n, minmax, mm, alpha, beta, stage, plane_b, dpitch, h->stream));
        if (packed) {
            HIP_TRY(h, hipMemcpyAsync(dst[0], stage, plane_b * n, hipMemcpyDeviceToHost, h->stream));
        } else {
            for (int i = 0; i < n; ++i)
                HIP_TRY(h, copy_rows(dst[i], dst_step, stage + (size_t)i * plane_b, dpitch, (size_t)cols, rows, hipMemcpyDeviceToHost, h->stream));
        }
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return CVS_OK;
    }
    // device destinations: regular too?  then straight into them, else plane by plane
    if (drun.ok) {
        HIP_TRY(h, launch_to_u8_n(src[0].data, stride, src[0].step / sizeof(float), rows, cols, n, minmax, mm, alpha, beta, dst[0], (size_t)drun.stride, dst_step, h->stream));
        return CVS_OK;
    }
    return one_by_one();
}

// The handle's scratch for the 8-bit pipeline outputs: `slots` min / max pairs, then `planes` f32 planes of rows x pitch (grown only;
// the state block is never used for this: it may be parked in the process-wide cache)
int u8_scratch(cvs_handle h, int slots, size_t planes, int rows, size_t pitch, int** mm, float** scr)
{
    const size_t head = round_up((size_t)2 * slots, 64), need = head + planes * rows * pitch;
    if (const int rc = grow_scratch(h, "hipMalloc(&h->u8_scr, need * sizeof(float))", h->u8_scr, h->u8_scr_elems, need, sizeof(float))) return rc;
    *mm = reinterpret_cast<int*>(h->u8_scr);
    *scr = h->u8_scr + head;
    return CVS_OK;
}

// Normalise mode, after the launch: plane i of the 3n f32 scratch planes (constant stride) with min / max pair i into byte map i % 3 of
// frame i / 3 of `outs` -- one quantise launch when those lie at one constant stride with one step, else one per plane
int quantize_maps(cvs_handle h, const float* scr, size_t plane_stride, size_t pitch, int rows, int cols, int n, const int* mm, const cvs_plane* outs)
{
    auto dst = [&](int i) -> const cvs_plane& { return outs[(size_t)(i / 3) * 8 + 5 + i % 3]; };
    const PlaneRun run = plane_run(3 * n, 1, [&](int i, int) { return plane_at(dst(i)); }, true);
    if (run.ok) {
        HIP_TRY(h, launch_quantize_n(scr, plane_stride, pitch, rows, cols, 3 * n, mm, reinterpret_cast<uint8_t*>(dst(0).data), (size_t)run.stride, dst(0).step, h->stream));
        return CVS_OK;
    }
    for (int i = 0; i < 3 * n; ++i)
        HIP_TRY(h, launch_quantize_n(scr + (size_t)i * plane_stride, plane_stride, pitch, rows, cols, 1, mm + 2 * i, reinterpret_cast<uint8_t*>(dst(i).data), 0,
                                     dst(i).step, h->stream));
    return CVS_OK;
}

// the one-launch G2 pipeline of a single image with request `u8` on the outputs `outs` (a flat table of eight)
int setup_full_u8(cvs_handle h, const cvs_plane* image, const cvs_plane* outs, const U8Req& u8)
{
    const cvs_plane* po[8];
    frame_outs(outs, 0, po);
    SetupReq rq{image, CVS_SETUP_FULL};
    rq.pipe_outs = po;
    rq.u8 = &u8;
    return do_setup(h, rq);
}

// Three maps as bytes in the filter launch (G2, no state, find on magnitude, the compatible arctangent, device planes): kNotFused when
// the launch would not be one three-maps instance
int pipeline_u8_fused(cvs_handle h, const cvs_plane* images, int n, const cvs_plane* outs, bool batch)
{
    const int rows = images[0].rows, cols = images[0].cols;
    const bool gain = h->u8_gain > 0.f;
    int rc;
    if (gain) {   // the caller's byte planes straight from the epilogue
        const U8Req rq{1, h->u8_gain, nullptr};
        rc = batch ? batch_run(h, images, n, outs, &rq) : setup_full_u8(h, images, outs, rq);
        if (rc == CVS_OK) h->last.u8_out = 1;
        return rc;
    }
    // normalise: f32 maps into the handle's scratch ([n][3][rows][pitch]) with min / max reduced in the same launch, then ONE quantise launch
    const size_t pitch = round_up((size_t)cols, 64), pstride = pitch * rows;
    int* mm = nullptr;
    float* scr = nullptr;
    if ((rc = u8_scratch(h, 3 * n, (size_t)3 * n, rows, pitch, &mm, &scr))) return rc;
    std::vector<cvs_plane> so((size_t)n * 8, cvs_plane{nullptr, 0, 0, 0, 0});
    for (int i = 0; i < n; ++i)
        for (int k = 5; k < 8; ++k)
            so[(size_t)i * 8 + k] = cvs_plane{scr + ((size_t)i * 3 + (k - 5)) * pstride, rows, cols, pitch * sizeof(float), CVS_MEM_DEVICE};
    const U8Req rq{2, 0.f, mm};
    rc = batch ? batch_run(h, images, n, so.data(), &rq) : setup_full_u8(h, images, so.data(), rq);
    if (rc) return rc;
    if ((rc = quantize_maps(h, scr, pstride, pitch, rows, cols, n, mm, outs))) return rc;
    h->last.u8_out = 2;
    return CVS_OK;
}

// Any other call with 8-bit outputs: the f32 call with scratch planes in place of the byte planes, then the quantise kernels of
// cvs_normalize_u8 / cvs_convert_u8 (to_u8_batch) -- the same bytes, by construction.  Host byte planes come down as bytes.
int pipeline_u8_composed(cvs_handle h, const cvs_plane* images, int n, const cvs_plane* outs, bool batch)
{
    const int rows = images[0].rows, cols = images[0].cols;
    const size_t pitch = round_up((size_t)cols, 64), pstride = pitch * rows;
    size_t m = 0;
    for (size_t i = 0; i < (size_t)n * 8; ++i) m += (outs[i].data && is_u8(&outs[i])) ? 1 : 0;
    int* mm = nullptr;
    float* scr = nullptr;
    int rc;
    if ((rc = u8_scratch(h, 0, m, rows, pitch, &mm, &scr))) return rc;
    std::vector<cvs_plane> so(outs, outs + (size_t)n * 8), src;
    std::vector<const cvs_plane*> dst;
    for (size_t i = 0; i < (size_t)n * 8; ++i) {
        if (!outs[i].data || !is_u8(&outs[i])) continue;
        so[i] = cvs_plane{scr + src.size() * pstride, rows, cols, pitch * sizeof(float), CVS_MEM_DEVICE};
        src.push_back(so[i]);
        dst.push_back(&outs[i]);
    }
    if (batch) rc = cvs_pipeline_batch(h, images, n, so.data());
    else {
        const cvs_plane* po[8];
        frame_outs(so.data(), 0, po);
        rc = cvs_pipeline(h, images, po);
    }
    if (rc) return rc;
    // one to_u8_batch call per (row step, memory) of the destinations -- one of them in the usual case
    std::vector<bool> done(dst.size(), false);
    for (size_t i = 0; i < dst.size(); ++i) {
        if (done[i]) continue;
        std::vector<cvs_plane> gs;
        std::vector<uint8_t*> gd;
        for (size_t j = i; j < dst.size(); ++j)
            if (!done[j] && dst[j]->step == dst[i]->step && mem_of(dst[j]) == mem_of(dst[i])) {
                gs.push_back(src[j]);
                gd.push_back(reinterpret_cast<uint8_t*>(dst[j]->data));
                done[j] = true;
            }
        const bool minmax = !(h->u8_gain > 0.f);
        if ((rc = to_u8_batch(h, gs.data(), (int)gs.size(), gd.data(), dst[i]->step, mem_of(dst[i]), minmax, minmax ? 0.f : h->u8_gain, 0.f))) return rc;
    }
    h->last.u8_out = 3;
    return CVS_OK;
}

// G4 with extensions: the pair launch of every frame, then ONE k_g4_pipeline launch over all frames that writes the three maps as bytes
// (gain; byte planes at one constant frame stride with one row step) or as f32 scratch with their min / max reduced, followed by one
// quantise launch (normalise).  kNotFused (before anything is launched) when the byte planes do not lie that way.
int g4_u8_fused(cvs_handle h, const cvs_plane* images, int n, const cvs_plane* outs)
{
    const int rows = images[0].rows, cols = images[0].cols;
    const bool gain = h->u8_gain > 0.f;
    G4PipeArgs a{};
    int* mm = nullptr;
    float* scr = nullptr;
    const size_t pitch = round_up((size_t)cols, 64), pstride = pitch * rows;
    int rc;
    if (gain) {
        // one row step for the three maps of every frame; a stride of 0 passes here (the gain mode of batch_run refuses it)
        const PlaneRun run = plane_run(n, 3, [&](int i, int k) { return plane_at(outs[(size_t)i * 8 + 5 + k]); }, true);
        if (!run.ok || outs[6].step != outs[5].step || outs[7].step != outs[5].step) return kNotFused;
        for (int k = 0; k < 3; ++k) a.out[G4P_EDGES + k] = {outs[5 + k].data, outs[5].step, (size_t)run.stride};   // (byte planes: pitch and stride in bytes)
        a.u8_mode = 1;
        a.u8_gain = h->u8_gain;
    } else {
        if ((rc = u8_scratch(h, 3 * n, (size_t)3 * n, rows, pitch, &mm, &scr))) return rc;
        for (int k = 0; k < 3; ++k) a.out[G4P_EDGES + k] = {scr + (size_t)k * pstride, pitch, 3 * pstride};
        a.u8_mode = 2;
        a.u8_mm = mm;
    }
    for (int i = 0; i < n; ++i)
        if ((rc = g4_basis_frame(h, &images[i], n, i))) return rc;
    h->cur_frame = 0;
    g4_pipe_args(h, n, a);
    if (mm) HIP_TRY(h, launch_minmax_init_n(mm, 3 * n, h->stream));
    HIP_TRY(h, launch_g4_pipeline(a, h->stream));
    h->have_basis = h->have_orient = false;   // (no state kept: CVS_OPT_PERSIST_STATE = 0)
    if (!gain && (rc = quantize_maps(h, scr, pstride, pitch, rows, cols, n, mm, outs))) return rc;
    h->last.u8_out = gain ? 1 : 2;
    return CVS_OK;
}

// device images, exactly the outputs 5..7 (edges, dark, bright) requested and all of them device bytes: what both fused routes need
bool three_byte_maps(const cvs_plane* images, int n, const cvs_plane* outs)
{
    for (int i = 0; i < n; ++i) {
        if (mem_of(&images[i]) != CVS_MEM_DEVICE) return false;
        for (int k = 0; k < 8; ++k) {
            const cvs_plane& o = outs[(size_t)i * 8 + k];
            if ((o.data != nullptr) != (k >= 5) || (o.data && o.mem != (CVS_MEM_DEVICE | CVS_DEPTH_U8))) return false;
        }
    }
    return true;
}

int pipeline_u8(cvs_handle h, const cvs_plane* images, int n, const cvs_plane* outs, bool batch)
{
    const bool g4 = h->kind == CVS_KIND_G4;   // (extensions on: checked by the entry points)
    const bool modes = g4 ? !h->persist : h->kind == CVS_KIND_G2 && !h->persist && !h->find_on && h->atan_mode == 0;
    if (modes && three_byte_maps(images, n, outs)) {
        const int rc = g4 ? g4_u8_fused(h, images, n, outs) : pipeline_u8_fused(h, images, n, outs, batch);
        if (rc != kNotFused) return rc;
    }
    return pipeline_u8_composed(h, images, n, outs, batch);
}

}  // namespace

extern "C" {

int cvs_pipeline(cvs_handle h, const cvs_plane* image, const cvs_plane* const outs[8])
{
    if (!h || !outs) return CVS_E_BADARG;
    if (h->kind != CVS_KIND_G2 && !h->g4_ext) return fail(h, CVS_E_UNSUPPORTED, "the caller pipeline exists for G2, and for G4 with CVS_OPT_G4_EXTENSIONS");
    int rc = check_plane(h, image, "image", true);
    if (rc) return rc;
    bool any_u8 = false;
    for (int o = 0; o < 8; ++o) {
        if (!outs[o]) continue;
        if ((rc = check_plane(h, outs[o], "out", true)) || (rc = check_same(h, outs[o], image->rows, image->cols))) return rc;
        any_u8 = any_u8 || is_u8(outs[o]);
    }
    h->last.u8_out = 0;
    if (any_u8) {
        if ((rc = check_no_overlap(h, image, outs, 8))) return rc;
        cvs_plane flat[8] = {};
        for (int o = 0; o < 8; ++o)
            if (outs[o]) flat[o] = *outs[o];
        return pipeline_u8(h, image, 1, flat, false);
    }
    if (h->kind == CVS_KIND_G4) {   // the pair launch, then one per-pixel launch over its 11 planes
        if ((rc = check_no_overlap(h, image, outs, 8))) return rc;
        return g4_pipeline_one(h, image, outs, 1, 0);
    }
    // one launch: filter bank, orientation and the whole caller sequence in the kernel's epilogue
    SetupReq rq{image, CVS_SETUP_FULL};
    rq.pipe_outs = outs;
    return do_setup(h, rq);
}

int cvs_pipeline_batch(cvs_handle h, const cvs_plane* images, int n, const cvs_plane* outs)
{
    if (!h || !images || n < 1) return CVS_E_BADARG;
    if (h->kind != CVS_KIND_G2 && !h->g4_ext) return fail(h, CVS_E_UNSUPPORTED, "the caller pipeline exists for G2, and for G4 with CVS_OPT_G4_EXTENSIONS");
    int rc;
    const int rows = images[0].rows, cols = images[0].cols;
    bool any_u8 = false;
    for (int i = 0; i < n; ++i) {
        if ((rc = check_plane(h, &images[i], "image", true)) || (rc = check_same(h, &images[i], rows, cols))) return rc;
        for (int k = 0; outs && k < 8; ++k) {
            const cvs_plane* o = &outs[(size_t)i * 8 + k];
            if (!o->data) continue;
            if ((rc = check_plane(h, o, "out", true)) || (rc = check_same(h, o, rows, cols))) return rc;
            if (outs[k].data && is_u8(o) != is_u8(&outs[k])) return fail(h, CVS_E_BADARG, "an output has another depth than in frame 0");
            any_u8 = any_u8 || is_u8(o);
        }
        if (outs) {
            const cvs_plane* po[8];
            frame_outs(outs, i, po);
            if ((rc = check_no_overlap(h, &images[i], po, 8))) return rc;
        }
    }
    h->last.u8_out = 0;
    if (any_u8) return pipeline_u8(h, images, n, outs, true);
    return batch_run(h, images, n, outs, nullptr);
}

int cvs_normalize_u8_batch(cvs_handle h, const cvs_plane* src, int n, uint8_t* const* dst, size_t dst_step, int dst_mem)
{
    return to_u8_batch(h, src, n, dst, dst_step, dst_mem, true, 0.f, 0.f);
}

int cvs_convert_u8_batch(cvs_handle h, const cvs_plane* src, int n, float alpha, float beta, uint8_t* const* dst, size_t dst_step, int dst_mem)
{
    return to_u8_batch(h, src, n, dst, dst_step, dst_mem, false, alpha, beta);
}

int cvs_normalize_u8(cvs_handle h, const cvs_plane* src, uint8_t* dst, size_t dst_step, int dst_mem)
{
    return to_u8(h, src, dst, dst_step, dst_mem, true, 0.f, 0.f);
}

int cvs_convert_u8(cvs_handle h, const cvs_plane* src, float alpha, float beta, uint8_t* dst, size_t dst_step, int dst_mem)
{
    return to_u8(h, src, dst, dst_step, dst_mem, false, alpha, beta);
}

}  // extern "C"
