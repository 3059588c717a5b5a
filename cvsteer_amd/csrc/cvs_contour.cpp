// cvs_contour.cpp -- the C ABI of contour thinning (extension): cvs_nonmax, cvs_nonmax_batch and cvs_hysteresis in front of
// cvs_kernels_contour.hip, and the host helpers the whole contour tail shares (cvs_contour_host.h).  Argument checks, the handle's scratch,
// staging of host planes and the launch sequences.  No arithmetic on image data happens here.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "cvs_contour.h"
#include "cvs_contour_host.h"
#include "cvs_layout.h"

namespace cvs {

int need_image(cvs_handle h)
{
    if (h->rows <= 0) return fail(h, CVS_E_STATE, "no setup yet: the handle has no image size");
    return CVS_OK;
}

int check_sized(cvs_handle h, const cvs_plane* p, const char* name, int rows, int cols, bool allow_u8)
{
    const int rc = check_plane(h, p, name, allow_u8);
    return rc ? rc : check_same(h, p, rows, cols);
}

int capturing(cvs_handle h, bool& yes)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_TRY(h, hipStreamIsCapturing(h->stream, &cap));
    yes = cap != hipStreamCaptureStatusNone;
    return CVS_OK;
}

int refuse_capture(cvs_handle h, const char* what)
{
    bool yes = false;
    const int rc = capturing(h, yes);
    return rc ? rc : yes ? fail(h, CVS_E_UNSUPPORTED, what) : CVS_OK;
}

int grow_cc(cvs_handle h, size_t need)
{
    if (need > h->cc_scr_bytes) HIP_TRY(h, hipSetDevice(h->device));
    return grow_scratch(h, "hipMalloc(&h->cc_scr, need)", h->cc_scr, h->cc_scr_bytes, need, 1);
}

int mask_ref(Call& c, const cvs_plane* p, MaskRef& m)
{
    if (direct_u8(p)) {
        m = {p->data, p->step, 1};
        return CVS_OK;
    }
    PlaneRef r;
    const int rc = in_ref(c, p, r);
    m = {r.p, r.pitch, 0};
    return rc;
}

int mask_out(Call& c, const cvs_plane* o, bool u8, unsigned char* slot, size_t slot_pitch, void*& p, size_t& pitch)
{
    if (!u8) {
        PlaneRef r;
        const int rc = out_ref(c, o, r);
        p = r.p;
        pitch = r.pitch;
        return rc;
    }
    p = staged_bytes(o, u8) ? static_cast<void*>(slot) : o->data;
    pitch = staged_bytes(o, u8) ? slot_pitch : o->step;
    return CVS_OK;
}

int fetch_mask(Call& c, const cvs_plane* o, bool u8, const void* p, size_t pitch)
{
    if (!staged_bytes(o, u8)) return CVS_OK;
    HIP_TRY(c.h, copy_rows(o->data, o->step, p, pitch, (size_t)o->cols, o->rows, hipMemcpyDeviceToHost, c.h->stream));
    return CVS_OK;
}

cvs_plane array_plane(const void* p, long long n, int words, int mem)
{
    cvs_plane q{};
    q.data = n > 0 ? const_cast<float*>(static_cast<const float*>(p)) : nullptr;
    q.rows = (int)n;
    q.cols = words;
    q.step = (size_t)words * 4;
    q.mem = mem;
    return q;
}

int Staged::commit()
{
    if (n_ == 0) return CVS_OK;
    if (sc_.need > h_->ch_scr_bytes) {
        bool cap = false;
        if (const int rc = capturing(h_, cap)) return rc;
        if (cap)
            return fail(h_, CVS_E_UNSUPPORTED,
                        (std::string(call_) + " would have to grow the handle's scratch during capture: call once eagerly first").c_str());
    }
    if (const int rc = grow_scratch(h_, "hipMalloc(&h->ch_scr, need)", h_->ch_scr, h_->ch_scr_bytes, sc_.need, 1)) return rc;
    for (int i = 0; i < n_; ++i) {
        unsigned char* p = h_->ch_scr + items_[i].off;
        std::memcpy(items_[i].field, &p, sizeof(p));   // (the field is an object pointer of some type: all of one representation)
    }
    return CVS_OK;
}

int Staged::copy(hipStream_t s, Dir dir)
{
    for (int i = 0; i < n_; ++i) {
        const Item& t = items_[i];
        if (t.dir != dir || t.bytes == 0) continue;
        if (dir == kUp) HIP_TRY(h_, hipMemcpyAsync(h_->ch_scr + t.off, t.host, t.bytes, hipMemcpyHostToDevice, s));
        else HIP_TRY(h_, hipMemcpyAsync(t.host, h_->ch_scr + t.off, t.bytes, hipMemcpyDeviceToHost, s));
    }
    return CVS_OK;
}

int Staged::upload(hipStream_t s) { return copy(s, kUp); }
int Staged::download(hipStream_t s) { return copy(s, kDown); }

int Staged::fetch(hipStream_t s)
{
    if (const int rc = download(s)) return rc;
    if (host_) HIP_TRY(h_, hipStreamSynchronize(s));
    return CVS_OK;
}

}  // namespace cvs

using namespace cvs;

extern "C" {

int cvs_nonmax(cvs_handle h, const cvs_plane* theta, int n, const cvs_plane* in, const cvs_plane* out)
{
    if (!h) return CVS_E_BADARG;
    if (n < 1 || n > kNmsMax || !in || !out) return fail(h, CVS_E_BADARG, "1..3 maps, in and out are required");
    int rc;
    if (!theta && (rc = need_state(h, true))) return rc;
    if ((rc = need_image(h))) return rc;
    if (theta && (rc = check_sized(h, theta, "theta", h->rows, h->cols))) return rc;
    for (int k = 0; k < n; ++k)
        if ((rc = check_sized(h, &in[k], "in", h->rows, h->cols)) || (rc = check_sized(h, &out[k], "out", h->rows, h->cols))) return rc;
    // theta == NULL: the handle's own theta plane of the selected frame -- an output must not overlap that either
    const PlaneRef own = theta ? PlaneRef{nullptr, 0} : state_ref(h, h->nb + 3);
    cvs_plane ins[1 + kNmsMax];
    ins[0] = theta ? *theta : device_plane(own.p, h->rows, h->cols, own.pitch);
    std::copy(in, in + n, ins + 1);
    if ((rc = check_disjoint(h, ins, 1 + (size_t)n, out, (size_t)n))) return rc;

    const cvs_plane* pin[kNmsMax] = {nullptr, nullptr, nullptr};
    const cvs_plane* pout[kNmsMax] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < n; ++k) {
        pin[k] = &in[k];
        pout[k] = &out[k];
    }
    Call c;
    if ((rc = begin(h, c, {theta, pin[0], pin[1], pin[2], pout[0], pout[1], pout[2]}))) return rc;
    NmsArgs a{};
    a.rows = h->rows;
    a.cols = h->cols;
    a.n = n;
    if (theta) {
        if ((rc = in_ref(c, theta, a.theta))) return rc;
    } else {
        a.theta = state_ref(h, h->nb + 3);
    }
    for (int k = 0; k < n; ++k)
        if ((rc = in_ref(c, pin[k], a.in[k])) || (rc = out_ref(c, pout[k], a.out[k]))) return rc;
    a.nt_stores = use_nt_stores(h, (size_t)a.rows * a.cols);
    HIP_TRY(h, launch_nonmax(a, h->stream));
    return finish(c);
}

int cvs_nonmax_batch(cvs_handle h, int frames, int n_maps, const cvs_plane* theta, const cvs_plane* in, const cvs_plane* out)
{
    if (!h) return CVS_E_BADARG;
    if (frames < 1 || n_maps < 1 || n_maps > kNmsMax || !in || !out) return fail(h, CVS_E_BADARG, "frames >= 1, 1..3 maps, in and out are required");
    int rc;
    if (!theta && (rc = need_state(h, true))) return rc;
    if ((rc = need_image(h))) return rc;
    if (!theta && frames > h->num_frames) return fail(h, CVS_E_STATE, "the handle holds the state of fewer frames");
    const int rows = h->rows, cols = h->cols;
    const size_t np = (size_t)frames * n_maps;
    for (int f = 0; theta && f < frames; ++f)
        if ((rc = check_sized(h, &theta[f], "theta", rows, cols))) return rc;
    for (size_t k = 0; k < np; ++k)
        if ((rc = check_sized(h, &in[k], "in", rows, cols)) || (rc = check_sized(h, &out[k], "out", rows, cols))) return rc;
    // theta == NULL: the theta state planes of frames 0 .. frames - 1 -- an output must not overlap those either
    std::vector<cvs_plane> own;
    if (!theta) {
        const PlaneRef r = state_ref(h, h->nb + 3);   // of the selected frame; frame f lies (f - cur_frame) frame strides from it
        for (int f = 0; f < frames; ++f) own.push_back(device_plane(r.p + ((ptrdiff_t)f - h->cur_frame) * (ptrdiff_t)h->frame_stride, rows, cols, r.pitch));
        theta = own.data();
    }
    std::vector<cvs_plane> ins(theta, theta + frames);
    ins.insert(ins.end(), in, in + np);
    if ((rc = check_disjoint(h, ins.data(), ins.size(), out, np))) return rc;

    // one launch when every plane is on the device and frame f's planes lie f strides behind frame 0's (an [F][K][H][W] block, the
    // state blocks of a batch); otherwise frame by frame, the single-frame launch
    bool dev = true;
    for (int f = 0; f < frames; ++f) dev = dev && mem_of(&theta[f]) == CVS_MEM_DEVICE;
    for (size_t k = 0; k < np; ++k) dev = dev && mem_of(&in[k]) == CVS_MEM_DEVICE && mem_of(&out[k]) == CVS_MEM_DEVICE;
    const ptrdiff_t f32 = (ptrdiff_t)sizeof(float);
    PlaneRun t_run{false, 0}, i_run[kNmsMax], o_run[kNmsMax];
    bool regular = dev && frames <= 65535;
    if (regular) {
        t_run = plane_run(frames, 1, [&](int i, int) { return plane_at(theta[i]); }, true, f32);
        regular = t_run.ok;
        for (int k = 0; k < n_maps && regular; ++k) {
            i_run[k] = plane_run(frames, 1, [&](int i, int) { return plane_at(in[(size_t)i * n_maps + k]); }, true, f32);
            o_run[k] = plane_run(frames, 1, [&](int i, int) { return plane_at(out[(size_t)i * n_maps + k]); }, false, f32);
            regular = i_run[k].ok && o_run[k].ok;
        }
    }
    if (!regular) {
        for (int f = 0; f < frames; ++f)
            if ((rc = cvs_nonmax(h, &theta[f], n_maps, in + (size_t)f * n_maps, out + (size_t)f * n_maps))) return rc;
        return CVS_OK;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    h->used = true;
    NmsArgs a{};
    NmsBatch b{};
    a.rows = rows;
    a.cols = cols;
    a.n = n_maps;
    a.theta = {static_cast<float*>(theta[0].data), theta[0].step / sizeof(float)};
    b.frames = frames;
    b.theta_stride = t_run.stride / f32;
    for (int k = 0; k < n_maps; ++k) {
        a.in[k] = {static_cast<float*>(in[k].data), in[k].step / sizeof(float)};
        a.out[k] = {static_cast<float*>(out[k].data), out[k].step / sizeof(float)};
        b.in_stride[k] = i_run[k].stride / f32;
        b.out_stride[k] = o_run[k].stride / f32;
    }
    a.nt_stores = use_nt_stores(h, (size_t)rows * cols * frames);
    HIP_TRY(h, launch_nonmax_batch(a, b, h->stream));
    return CVS_OK;
}

int cvs_hysteresis(cvs_handle h, int n, const cvs_plane* in, float low, float high, const cvs_plane* out, int* passes)
{
    if (!h) return CVS_E_BADARG;
    if (n < 1 || !in || !out) return fail(h, CVS_E_BADARG, "n >= 1 planes, in and out are required");
    if (std::isnan(low) || std::isnan(high) || low > high) return fail(h, CVS_E_BADARG, "thresholds: low <= high, neither NaN");
    int rc;
    if ((rc = need_image(h))) return rc;
    const bool u8 = is_u8(&out[0]);
    for (int k = 0; k < n; ++k) {
        if ((rc = check_sized(h, &in[k], "in", h->rows, h->cols)) || (rc = check_sized(h, &out[k], "out", h->rows, h->cols, true))) return rc;
        if (is_u8(&out[k]) != u8) return fail(h, CVS_E_BADARG, "the outputs are all bytes or all f32");
    }
    if ((rc = check_disjoint(h, in, (size_t)n, out, (size_t)n))) return rc;
    if ((rc = refuse_capture(h, "hysteresis reads its pass flag back: not capturable"))) return rc;

    // scratch: the flag word, then kHystMax label planes
    const int rows = h->rows, cols = h->cols;
    const size_t lab_pitch = round_up((size_t)cols, 64), lab_stride = round_up(lab_pitch * rows, 256);
    const size_t need = 256 + (size_t)kHystMax * lab_stride;
    if (need > h->hy_scr_bytes) HIP_TRY(h, hipSetDevice(h->device));   // (only a call that allocates sets the device: grow_scratch's own condition)
    if ((rc = grow_scratch(h, "hipMalloc(&h->hy_scr, need)", h->hy_scr, h->hy_scr_bytes, need, 1))) return rc;
    unsigned* flag = reinterpret_cast<unsigned*>(h->hy_scr);
    // a pass that is not the last promotes at least one pixel: more passes than pixels (+ the last group) would be a fault of ours
    const long long max_passes = (long long)rows * cols * kHystMax + 64;
    int total = 0;
    for (int z0 = 0; z0 < n; z0 += kHystMax) {
        const int m = std::min(kHystMax, n - z0);
        const cvs_plane* pin[kHystMax] = {nullptr, nullptr, nullptr};
        const cvs_plane* pout[kHystMax] = {nullptr, nullptr, nullptr};   // f32 outputs go through the staging arena
        for (int k = 0; k < m; ++k) {
            pin[k] = &in[z0 + k];
            if (!u8) pout[k] = &out[z0 + k];
        }
        Call c;
        if ((rc = begin(h, c, {pin[0], pin[1], pin[2], pout[0], pout[1], pout[2]}))) return rc;
        HystArgs a{};
        a.rows = rows;
        a.cols = cols;
        a.n = m;
        a.low = low;
        a.high = high;
        a.lab = h->hy_scr + 256;
        a.lab_pitch = lab_pitch;
        a.lab_stride = lab_stride;
        a.out_u8 = u8 ? 1 : 0;
        for (int k = 0; k < m; ++k) {
            void* p = nullptr;   // host bytes: written over the label plane, downloaded from there
            if ((rc = in_ref(c, pin[k], a.in[k])) || (rc = mask_out(c, &out[z0 + k], u8, a.lab + (size_t)k * lab_stride, lab_pitch, p, a.out_pitch[k])))
                return rc;
            if (u8) a.out8[k] = static_cast<unsigned char*>(p);
            else a.out32[k] = static_cast<float*>(p);
        }
        HIP_TRY(h, launch_hyst_classify(a, h->stream));
        // passes in groups (1, 2, 4 .. 16) between read-backs of the flag; the group that changes nothing ends the loop
        for (int group = 1;; group = std::min(2 * group, 16)) {
            HIP_TRY(h, launch_hyst_flag_reset(flag, h->stream));
            for (int i = 0; i < group; ++i) HIP_TRY(h, launch_hyst_pass(a, flag, h->stream));
            total += group;
            unsigned changed = 0;
            HIP_TRY(h, hipMemcpyAsync(&changed, flag, sizeof(changed), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            if (!changed) break;
            if (total > max_passes) return fail(h, CVS_E_HIP, "hysteresis did not converge");
        }
        HIP_TRY(h, launch_hyst_emit(a, h->stream));
        for (int k = 0; k < m; ++k)
            if ((rc = fetch_mask(c, &out[z0 + k], u8, a.out8[k], lab_pitch))) return rc;
        if ((rc = finish(c))) return rc;
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if (passes) *passes = total;
    return CVS_OK;
}

}  // extern "C"
