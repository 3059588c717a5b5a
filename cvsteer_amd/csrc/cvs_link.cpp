// cvs_link.cpp -- the C ABI of the contour chain on the batch axis (extension): cvs_link, hysteresis and prune as one labelling over any
// number of planes (cvs_kernels_link.hip), and cvs_contours_batch, the whole chain for n frames.  Argument checks, the handle's scratch,
// staging of host planes and the fixed launch sequence.  No arithmetic on image data happens here, and nothing is read back.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "cvs_contour_host.h"
#include "cvs_layout.h"
#include "cvs_link.h"

using namespace cvs;

namespace {

// planes per chain: what fits the scratch bound with their parent, area and peak planes (at least one; the descriptor table and the byte
// staging of host outputs come on top), what one grid dimension counts, and -- with host planes, which are staged
// on the device for the duration of a chain -- a handful
int chain_planes(size_t plane_stride, bool any_host)
{
    const size_t fit = kLinkScratchMax / (plane_stride * 12);
    size_t m = std::max<size_t>(1, std::min<size_t>(fit, (size_t)kLinkChainMax));
    if (any_host) m = std::min<size_t>(m, 8);
    return (int)m;
}

}  // namespace

extern "C" {

int cvs_link(cvs_handle h, int n, const cvs_plane* in, float low, float high, int min_area, float min_peak, const cvs_plane* out,
             int32_t* kept_dev)
{
    if (!h) return CVS_E_BADARG;
    if (n < 1 || !in || !out) return fail(h, CVS_E_BADARG, "n >= 1 planes, in and out are required");
    if (std::isnan(low) || std::isnan(high) || low > high) return fail(h, CVS_E_BADARG, "thresholds: low <= high, neither NaN");
    if (min_area < 0 || std::isnan(min_peak)) return fail(h, CVS_E_BADARG, "min_area >= 0, min_peak not NaN");
    int rc;
    if ((rc = need_image(h))) return rc;
    const int rows = h->rows, cols = h->cols;
    if ((long long)rows * cols > 0x7fffffffLL - 1) return fail(h, CVS_E_SIZE, "more than 2^31 - 2 pixels");
    const bool u8 = is_u8(&out[0]);
    bool any_host = false;
    for (int k = 0; k < n; ++k) {
        if ((rc = check_sized(h, &in[k], "in", rows, cols)) || (rc = check_sized(h, &out[k], "out", rows, cols, true))) return rc;
        if (is_u8(&out[k]) != u8) return fail(h, CVS_E_BADARG, "the outputs are all bytes or all f32");
        any_host = any_host || mem_of(&in[k]) == CVS_MEM_HOST || mem_of(&out[k]) == CVS_MEM_HOST;
    }
    if ((rc = check_disjoint(h, in, (size_t)n, out, (size_t)n))) return rc;
    if (kept_dev && reinterpret_cast<uintptr_t>(kept_dev) % alignof(int32_t)) return fail(h, CVS_E_BADARG, "kept_dev not aligned to 4 bytes");

    // scratch of one chain: parent, area and peak of its planes, the descriptor table, byte staging of host outputs
    const size_t npix = (size_t)rows * cols, plane_stride = round_up(npix, 64), bpitch = round_up((size_t)cols, 64);
    const int per_chain = std::min(n, chain_planes(plane_stride, any_host));
    const size_t words = (size_t)per_chain * plane_stride * 4, bstride = round_up(bpitch * rows, 256);
    Scratch sc;
    const size_t o_parent = sc.reserve(words), o_area = sc.reserve(words), o_peak = sc.reserve(words);
    const size_t o_tab = sc.reserve((size_t)per_chain * sizeof(LinkDesc));
    const size_t o_bytes = (u8 && any_host) ? sc.reserve((size_t)per_chain * bstride) : 0;
    bool cap = false;
    if ((rc = capturing(h, cap))) return rc;
    if (cap) {
        if (any_host) return fail(h, CVS_E_UNSUPPORTED, "cvs_link with host planes copies and synchronises: not capturable");
        if (sc.need > h->cc_scr_bytes)
            return fail(h, CVS_E_UNSUPPORTED, "cvs_link would have to grow the handle's scratch during capture: call once eagerly first");
    }
    if ((rc = grow_cc(h, sc.need))) return rc;
    LinkDesc* dtab = reinterpret_cast<LinkDesc*>(h->cc_scr + o_tab);

    std::vector<LinkDesc> desc((size_t)per_chain);
    for (int z0 = 0; z0 < n; z0 += per_chain) {
        const int m = std::min(per_chain, n - z0);
        Call c;
        size_t stage = 0;
        for (int k = 0; any_host && k < m; ++k) stage += staged_elems(&in[z0 + k]) + (u8 ? 0 : staged_elems(&out[z0 + k]));
        if ((rc = begin(h, c, {}, stage))) return rc;
        for (int k = 0; k < m; ++k) {
            const cvs_plane* o = &out[z0 + k];
            PlaneRef r;
            if ((rc = in_ref(c, &in[z0 + k], r))) return rc;
            desc[k].in = r.p;
            desc[k].in_pitch = r.pitch;
            if ((rc = mask_out(c, o, u8, h->cc_scr + o_bytes + (size_t)k * bstride, bpitch, desc[k].out, desc[k].out_pitch))) return rc;
        }
        LinkArgs a{};
        a.rows = rows;
        a.cols = cols;
        a.n = m;
        a.low = low;
        a.high = high;
        a.min_area = min_area;
        a.min_peak = min_peak;
        a.out_u8 = u8 ? 1 : 0;
        a.parent = reinterpret_cast<int32_t*>(h->cc_scr + o_parent);
        a.area = reinterpret_cast<int32_t*>(h->cc_scr + o_area);
        a.peak = reinterpret_cast<uint32_t*>(h->cc_scr + o_peak);
        a.plane_stride = plane_stride;
        a.kept = kept_dev ? kept_dev + z0 : nullptr;
        // planes at one stride (an [N, H, W] block, the staged copies of host planes) are addressed arithmetically; anything else through
        // the device table, which launches fill from their arguments
        const PlaneRun in_run = plane_run(m, 1, [&](int i, int) { return PlaneAt{reinterpret_cast<uintptr_t>(desc[i].in), desc[i].in_pitch}; }, true,
                                          (ptrdiff_t)sizeof(float));
        const PlaneRun out_run = plane_run(m, 1, [&](int i, int) { return PlaneAt{reinterpret_cast<uintptr_t>(desc[i].out), desc[i].out_pitch}; }, false);
        if (in_run.ok && out_run.ok) {
            a.first = desc[0];
            a.in_stride = in_run.stride / (ptrdiff_t)sizeof(float);
            a.out_stride = out_run.stride;
        } else {
            for (int k0 = 0; k0 < m; k0 += kLinkTableBatch) {
                LinkTableArgs t{};
                t.first = k0;
                t.count = std::min(kLinkTableBatch, m - k0);
                for (int k = 0; k < t.count; ++k) t.d[k] = desc[k0 + k];
                HIP_TRY(h, launch_link_table(t, dtab, h->stream));
            }
            a.tab = dtab;
        }
        HIP_TRY(h, launch_link_tiles(a, h->stream));
        HIP_TRY(h, launch_link_borders(a, h->stream));
        HIP_TRY(h, launch_link_stats(a, h->stream));
        HIP_TRY(h, launch_link_emit(a, h->stream));
        for (int k = 0; k < m; ++k) {
            if ((rc = fetch_mask(c, &out[z0 + k], u8, desc[k].out, desc[k].out_pitch))) return rc;
            if (staged_bytes(&out[z0 + k], u8)) c.touched_host = true;
        }
        if ((rc = finish(c))) return rc;   // host planes: the data has landed, and the staging of the next chain may reuse the memory
    }
    return CVS_OK;
}

int cvs_contours_batch(cvs_handle h, const cvs_plane* images, int n, float low, float high, int min_area, float min_peak,
                       const cvs_plane* outs)
{
    if (!h) return CVS_E_BADARG;
    if (!images || n < 1 || !outs) return fail(h, CVS_E_BADARG, "n >= 1 frames, images and outs are required");
    if (h->kind != CVS_KIND_G2 && !h->g4_ext) return fail(h, CVS_E_UNSUPPORTED, "the caller pipeline exists for G2, and for G4 with CVS_OPT_G4_EXTENSIONS");
    if (!h->persist)
        return fail(h, CVS_E_STATE, "cvs_contours_batch thins across the theta plane of every frame: it needs CVS_OPT_PERSIST_STATE = 1");
    if (std::isnan(low) || std::isnan(high) || low > high) return fail(h, CVS_E_BADARG, "thresholds: low <= high, neither NaN");
    if (min_area < 0 || std::isnan(min_peak)) return fail(h, CVS_E_BADARG, "min_area >= 0, min_peak not NaN");
    int rc;
    const int rows = images[0].rows, cols = images[0].cols;
    std::vector<cvs_plane> want_out;
    std::vector<size_t> want_idx;
    for (int i = 0; i < n; ++i) {
        if ((rc = check_sized(h, &images[i], "image", rows, cols, true))) return rc;
        for (int k = 0; k < 3; ++k) {
            const cvs_plane* o = &outs[(size_t)i * 3 + k];
            if (!o->data) continue;
            if ((rc = check_sized(h, o, "out", rows, cols, true))) return rc;
            want_out.push_back(*o);
            want_idx.push_back((size_t)i * 3 + k);
        }
    }
    for (size_t k = 0; k < want_out.size(); ++k)
        if (is_u8(&want_out[k]) != is_u8(&want_out[0])) return fail(h, CVS_E_BADARG, "the outputs are all bytes or all f32");
    // every output against the image of EVERY frame and against every other output
    if ((rc = check_disjoint(h, images, (size_t)n, want_out.data(), want_out.size()))) return rc;
    // the handle's own planes: [n][3] maps and [n][3] thinned maps, dense rows of `pitch` elements
    const size_t pitch = round_up((size_t)cols, 64), plane = pitch * rows, total = (size_t)n * 6 * plane;
    if (total > h->ct_scr_elems) HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = grow_scratch(h, "hipMalloc(&h->ct_scr, total * sizeof(float))", h->ct_scr, h->ct_scr_elems, total, sizeof(float)))) return rc;
    auto own = [&](size_t idx) { return device_plane(h->ct_scr + idx * plane, rows, cols, pitch); };
    std::vector<cvs_plane> pipe_outs((size_t)n * 8), maps((size_t)n * 3), thin((size_t)n * 3);
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            maps[(size_t)i * 3 + k] = own((size_t)i * 3 + k);
            thin[(size_t)i * 3 + k] = own((size_t)n * 3 + (size_t)i * 3 + k);
            pipe_outs[(size_t)i * 8 + 5 + k] = maps[(size_t)i * 3 + k];
        }
    if ((rc = cvs_pipeline_batch(h, images, n, pipe_outs.data()))) return rc;
    if ((rc = cvs_nonmax_batch(h, n, 3, nullptr, maps.data(), thin.data()))) return rc;
    if (want_out.empty()) return CVS_OK;
    std::vector<cvs_plane> want_in;
    for (size_t idx : want_idx) want_in.push_back(thin[idx]);
    return cvs_link(h, (int)want_in.size(), want_in.data(), low, high, min_area, min_peak, want_out.data(), nullptr);
}

}  // extern "C"
