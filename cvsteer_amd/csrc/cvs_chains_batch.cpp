// cvs_chains_batch.cpp -- the C ABI of the contour chains and the sub-pixel chain points on the batch axis (extension):
// cvs_contour_chains_batch and cvs_chain_refine_batch.  Argument checks, the handle's scratch (the stacked planes in cvs_context::cc_scr, the
// arc arrays and staged lists in cvs_context::ch_scr), staging of host planes, the single-stride-or-table decision of cvs_link.cpp, and the
// launch sequences of cvs_kernels_chains_batch.hip around the unchanged launches of cvs_kernels_chains.hip.  No arithmetic on image data
// happens here, and no loop over pixels or chains (the check of a HOST point list is that of cvs_refine.cpp).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <vector>

#include "cvs_chains_batch.h"
#include "cvs_contour_host.h"
#include "cvs_layout.h"

using namespace cvs;

static_assert(sizeof(cvs_chain) == 16, "cvs_chain: four 4-byte fields (k_chb_head_apply writes it as four words)");

namespace {

constexpr long long kMaxPixels = 1LL << 28;

int ceil_log2(int n)
{
    int r = 0;
    while ((1LL << r) < n) ++r;
    return r;
}

// planes at one stride (an [N, H, W] block, the staged copies of host planes, the state blocks of a batch) are addressed arithmetically;
// anything else through the device table at `tab`, which launches fill from their arguments
int plane_set(cvs_handle h, const std::vector<MaskRef>& d, MaskRef* tab, PlaneSet& out)
{
    const int n = (int)d.size();
    bool one_depth = true;
    for (int k = 1; k < n; ++k) one_depth = one_depth && d[k].u8 == d[0].u8;
    const size_t esz = d[0].u8 ? 1 : sizeof(float);
    const PlaneRun run = one_depth ? plane_run(n, 1, [&](int i, int) { return PlaneAt{reinterpret_cast<uintptr_t>(d[i].p), d[i].pitch * esz}; }, true)
                                   : PlaneRun{false, 0};
    if (run.ok) {
        out = PlaneSet{d[0], (long long)run.stride, nullptr};
        return CVS_OK;
    }
    for (int k0 = 0; k0 < n; k0 += kChbTableBatch) {
        ChbTableArgs t{};
        t.first = k0;
        t.count = std::min(kChbTableBatch, n - k0);
        for (int k = 0; k < t.count; ++k) t.d[k] = d[k0 + k];
        HIP_TRY(h, launch_chb_table(t, tab, h->stream));
    }
    out = PlaneSet{MaskRef{nullptr, 0, 0}, 0, tab};
    return CVS_OK;
}

}  // namespace

extern "C" {

int cvs_contour_chains_batch(cvs_handle h, int n, const cvs_plane* masks, int32_t* points, int point_capacity, cvs_chain* chains,
                             int chain_capacity, int32_t* ranges, int mem, int* n_points, int* n_chains)
{
    if (!h) return CVS_E_BADARG;
    if (n < 1 || !masks) return fail(h, CVS_E_BADARG, "n >= 1 planes, masks is required");
    int rc;
    if ((rc = need_image(h))) return rc;
    const int rows = h->rows, cols = h->cols;
    for (int k = 0; k < n; ++k) {
        if ((rc = check_sized(h, &masks[k], "mask", rows, cols, true))) return rc;
        if (mem_of(&masks[k]) != mem_of(&masks[0])) return fail(h, CVS_E_BADARG, "the masks are all on the device or all on the host");
    }
    if ((long long)n * rows * cols > kMaxPixels) return fail(h, CVS_E_SIZE, "more than 2^28 pixels in all planes");
    if (!n_points || !n_chains) return fail(h, CVS_E_BADARG, "n_points and n_chains are required");
    if (point_capacity < 0 || (point_capacity > 0 && !points)) return fail(h, CVS_E_BADARG, "point_capacity >= 0, and points for a capacity > 0");
    if (chain_capacity < 0 || (chain_capacity > 0 && !chains)) return fail(h, CVS_E_BADARG, "chain_capacity >= 0, and chains for a capacity > 0");
    if ((point_capacity > 0 || chain_capacity > 0) && !ranges) return fail(h, CVS_E_BADARG, "a filling call needs ranges");
    if (mem != CVS_MEM_HOST && mem != CVS_MEM_DEVICE) return fail(h, CVS_E_BADARG, "mem");
    if (misaligned(points) || misaligned(chains) || misaligned(ranges)) return fail(h, CVS_E_BADARG, "points / chains / ranges not aligned to 4 bytes");
    const cvs_plane outs[3] = {array_plane(points, point_capacity, 2, mem), array_plane(chains, chain_capacity, 4, mem),
                               array_plane(ranges, (long long)n + 1, 2, mem)};
    if ((rc = check_disjoint(h, masks, (size_t)n, outs, 3))) return rc;
    if ((rc = refuse_capture(h, "cvs_contour_chains_batch reads its counts back: not capturable"))) return rc;

    const int srows = n * rows, blocks = scan_blocks(srows, cols);   // the stacked block
    const size_t npix = (size_t)srows * cols;
    hipStream_t s = h->stream;

    // ---- the stacked planes: links, components, nodes, and the counters every size follows from ----
    Scratch sc;
    const size_t o_parent = sc.reserve(npix * 4), o_aux = sc.reserve(npix * 4), o_link = sc.reserve(npix * 2);
    const size_t o_cnt = sc.reserve(kChCounters * 4), o_part = sc.reserve(((size_t)blocks + 1) * 4), o_tab = sc.reserve((size_t)n * sizeof(MaskRef));
    Call c;
    size_t stage = 0;
    for (int k = 0; k < n; ++k) stage += direct_u8(&masks[k]) ? 0 : staged_elems(&masks[k]);
    if ((rc = begin(h, c, {}, stage))) return rc;
    if ((rc = grow_cc(h, sc.need))) return rc;
    int32_t* parent = reinterpret_cast<int32_t*>(h->cc_scr + o_parent);
    int32_t* aux = reinterpret_cast<int32_t*>(h->cc_scr + o_aux);   // first the node flags at the roots, then the arc bases
    uint16_t* link = reinterpret_cast<uint16_t*>(h->cc_scr + o_link);
    int32_t* dcnt = reinterpret_cast<int32_t*>(h->cc_scr + o_cnt);
    int32_t* part = reinterpret_cast<int32_t*>(h->cc_scr + o_part);

    std::vector<MaskRef> desc((size_t)n);
    for (int k = 0; k < n; ++k)
        if ((rc = mask_ref(c, &masks[k], desc[k]))) return rc;
    ChbArgs a{};
    a.rows = rows;
    a.cols = cols;
    a.n = n;
    a.link = link;
    a.parent = parent;
    a.aux = aux;
    if ((rc = plane_set(h, desc, reinterpret_cast<MaskRef*>(h->cc_scr + o_tab), a.masks))) return rc;
    HIP_TRY(h, launch_zero_ints(dcnt, kChCounters, s));
    HIP_TRY(h, launch_chb_links(a, s));
    HIP_TRY(h, launch_chb_tiles(a, s));
    HIP_TRY(h, launch_chb_borders(a, s));
    HIP_TRY(h, launch_ch_nodes(srows, cols, link, parent, aux, s));
    HIP_TRY(h, launch_ch_roots(srows, cols, link, parent, aux, dcnt, s));
    int cnt[kChCounters] = {0, 0, 0, 0};
    HIP_TRY(h, hipMemcpyAsync(cnt, dcnt, sizeof(cnt), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    // open chains = half the degrees of the nodes, closed chains = components without a node; points = links + open chains + isolated
    const int open = cnt[kChNodeDeg] / 2, arcs = cnt[kChSumDeg] + cnt[kChIsolated];
    const int total_chains = open + cnt[kChClosed] + cnt[kChIsolated];
    const int total_points = cnt[kChSumDeg] / 2 + open + cnt[kChIsolated];
    *n_points = total_points;
    *n_chains = total_chains;
    if (total_points > point_capacity || total_chains > chain_capacity)
        return fail(h, CVS_E_SIZE, "more points or chains than capacity (n_points and n_chains say how many)");
    const bool host = mem == CVS_MEM_HOST;
    const int nr = 2 * (n + 1);
    if (arcs == 0) {   // every plane empty: a table of zeros
        if (ranges && host) std::fill_n(ranges, nr, 0);
        if (ranges && !host) {
            HIP_TRY(h, launch_zero_ints(ranges, nr, s));
            HIP_TRY(h, hipStreamSynchronize(s));
        }
        return CVS_OK;
    }

    // ---- the arcs: sized by the count just read ----
    const int ablocks = ch_scan_blocks(arcs);
    Scratch sa;
    const size_t o_to = sa.reserve((size_t)arcs * 4), o_rev = sa.reserve((size_t)arcs * 4);
    const size_t o_rec0 = sa.reserve((size_t)arcs * sizeof(ArcRec)), o_rec1 = sa.reserve((size_t)arcs * sizeof(ArcRec));
    const size_t o_pn = sa.reserve(((size_t)ablocks + 1) * 4), o_pl = sa.reserve(((size_t)ablocks + 1) * 4);
    const size_t o_pts = host ? sa.reserve((size_t)total_points * 8) : 0, o_chn = host ? sa.reserve((size_t)total_chains * sizeof(cvs_chain)) : 0;
    const size_t o_rng = host ? sa.reserve((size_t)nr * 4) : 0;
    if ((rc = grow_scratch(h, "hipMalloc(&h->ch_scr, need)", h->ch_scr, h->ch_scr_bytes, sa.need, 1))) return rc;
    int32_t* to = reinterpret_cast<int32_t*>(h->ch_scr + o_to);
    int32_t* rev = reinterpret_cast<int32_t*>(h->ch_scr + o_rev);
    ArcRec* rec[2] = {reinterpret_cast<ArcRec*>(h->ch_scr + o_rec0), reinterpret_cast<ArcRec*>(h->ch_scr + o_rec1)};
    int32_t* part_n = reinterpret_cast<int32_t*>(h->ch_scr + o_pn);
    int32_t* part_len = reinterpret_cast<int32_t*>(h->ch_scr + o_pl);
    int32_t* dpts = host ? reinterpret_cast<int32_t*>(h->ch_scr + o_pts) : points;
    int32_t* dchn = host ? reinterpret_cast<int32_t*>(h->ch_scr + o_chn) : reinterpret_cast<int32_t*>(chains);
    int32_t* drng = host ? reinterpret_cast<int32_t*>(h->ch_scr + o_rng) : ranges;

    HIP_TRY(h, launch_ch_arc_count(srows, cols, link, part, s));
    HIP_TRY(h, launch_scan_partials(part, blocks, s));
    HIP_TRY(h, launch_ch_arc_base(srows, cols, link, part, aux, s));
    HIP_TRY(h, launch_ch_arcs(srows, cols, link, aux, arcs, to, rev, rec[0], s));
    const int rounds = ceil_log2(arcs);   // no direction is longer than all the arcs there are
    for (int r = 0; r < rounds; ++r) HIP_TRY(h, launch_ch_jump(arcs, rec[r & 1], rec[(r + 1) & 1], s));
    const ArcRec* ranked = rec[rounds & 1];
    HeadRec* head = reinterpret_cast<HeadRec*>(rec[(rounds + 1) & 1]);   // the buffer the ranking has left over
    static_assert(sizeof(HeadRec) == sizeof(ArcRec), "the head records live in the spare ranking buffer");
    HIP_TRY(h, launch_ch_heads(arcs, link, to, rev, ranked, head, s));
    HIP_TRY(h, launch_ch_head_count(arcs, head, part_n, part_len, s));
    HIP_TRY(h, launch_scan_partials(part_n, ablocks, s));
    HIP_TRY(h, launch_scan_partials(part_len, ablocks, s));
    HIP_TRY(h, launch_chb_head_apply(arcs, head, part_n, part_len, to, rev, rows * cols, dchn, total_chains, s));
    HIP_TRY(h, launch_chb_emit(arcs, rows, cols, to, rev, ranked, head, dpts, total_points, s));
    HIP_TRY(h, launch_chb_ranges(dchn, total_chains, total_points, n, drng, s));
    if (host) {
        HIP_TRY(h, hipMemcpyAsync(points, dpts, (size_t)total_points * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(chains, dchn, (size_t)total_chains * sizeof(cvs_chain), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(ranges, drng, (size_t)nr * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    return CVS_OK;
}

int cvs_chain_refine_batch(cvs_handle h, int frames, int n_maps, const cvs_plane* maps, const cvs_plane* theta, const int32_t* points,
                           int n_points, const int32_t* ranges, float* xy, float* strength, int mem)
{
    if (!h) return CVS_E_BADARG;
    if (frames < 1 || n_maps < 1 || n_maps > 3 || !maps) return fail(h, CVS_E_BADARG, "frames >= 1, 1..3 maps per frame, maps is required");
    if (n_points < 0) return fail(h, CVS_E_BADARG, "n_points is >= 0");
    if (mem != CVS_MEM_HOST && mem != CVS_MEM_DEVICE) return fail(h, CVS_E_BADARG, "mem");
    int rc;
    if (!theta && (rc = need_state(h, true))) return rc;
    if ((rc = need_image(h))) return rc;
    if (!theta && frames > h->num_frames) return fail(h, CVS_E_STATE, "the handle holds the state of fewer frames");
    if ((long long)frames * n_maps > 0x7fffffffLL / 2 - 1) return fail(h, CVS_E_SIZE, "more planes than a range table can hold");
    const int rows = h->rows, cols = h->cols, n = frames * n_maps;
    for (int k = 0; k < n; ++k)
        if ((rc = check_sized(h, &maps[k], "map", rows, cols))) return rc;
    for (int f = 0; theta && f < frames; ++f)
        if ((rc = check_sized(h, &theta[f], "theta", rows, cols))) return rc;
    if (n_points > 0 && (!points || !xy || !ranges)) return fail(h, CVS_E_BADARG, "points / ranges / xy missing");
    if (misaligned(points) || misaligned(ranges) || misaligned(xy) || misaligned(strength)) return fail(h, CVS_E_BADARG, "an array is not aligned to 4 bytes");
    if (n_points > (1 << 30)) return fail(h, CVS_E_SIZE, "more than 2^30 points");
    // theta == NULL: the theta state planes of frames 0 .. frames - 1 -- an output must not overlap those either
    std::vector<cvs_plane> own;
    if (!theta) {
        const PlaneRef r = state_ref(h, h->nb + 3);   // of the selected frame; frame f lies (f - cur_frame) frame strides from it
        for (int f = 0; f < frames; ++f) own.push_back(device_plane(r.p + ((ptrdiff_t)f - h->cur_frame) * (ptrdiff_t)h->frame_stride, rows, cols, r.pitch));
        theta = own.data();
    }
    std::vector<cvs_plane> ins(maps, maps + n);
    ins.insert(ins.end(), theta, theta + frames);
    ins.push_back(array_plane(points, n_points, 2, mem));
    ins.push_back(array_plane(ranges, n_points > 0 ? (long long)n + 1 : 0, 2, mem));
    const cvs_plane outs[2] = {array_plane(xy, n_points, 2, mem), array_plane(strength, n_points, 1, mem)};
    if ((rc = check_disjoint(h, ins.data(), ins.size(), outs, 2))) return rc;
    const bool host = mem == CVS_MEM_HOST;
    if (host && n_points > 0) {
        if (ranges[1] != 0 || ranges[2 * (size_t)n + 1] != n_points) return fail(h, CVS_E_BADARG, "the point column of ranges goes from 0 to n_points");
        for (int z = 0; z < n; ++z)
            if (ranges[2 * (size_t)z + 1] > ranges[2 * (size_t)z + 3]) return fail(h, CVS_E_BADARG, "the point column of ranges decreases");
        for (int i = 0; i < n_points; ++i)
            if ((unsigned)points[2 * (size_t)i] >= (unsigned)cols || (unsigned)points[2 * (size_t)i + 1] >= (unsigned)rows)
                return fail(h, CVS_E_BADARG, "a point lies outside the image");
    }
    size_t stage = 0;   // (only host planes are staged)
    for (int k = 0; k < n + frames; ++k) stage += staged_elems(k < n ? &maps[k] : &theta[k - n]);
    const bool sync = host || stage > 0;
    if (sync && (rc = refuse_capture(h, "cvs_chain_refine_batch stages host memory and synchronises: not capturable"))) return rc;
    if (n_points == 0) return CVS_OK;

    // planes at no constant stride: their descriptor tables live in the staging arena (cc_scr may hold the planes of a chain call, ch_scr
    // the staged arrays).  Device planes say before anything is reserved whether a table is needed
    std::vector<MaskRef> dm((size_t)n), dt((size_t)frames);
    bool need_tab = stage > 0;
    if (!need_tab) {
        auto at = [](const MaskRef& m) { return PlaneAt{reinterpret_cast<uintptr_t>(m.p), m.pitch * sizeof(float)}; };
        for (int k = 0; k < n + frames; ++k) {
            const cvs_plane* p = k < n ? &maps[k] : &theta[k - n];
            (k < n ? dm[k] : dt[k - n]) = MaskRef{p->data, p->step / sizeof(float), 0};
        }
        need_tab = !plane_run(n, 1, [&](int i, int) { return at(dm[i]); }, true).ok || !plane_run(frames, 1, [&](int i, int) { return at(dt[i]); }, true).ok;
    }
    const size_t tab_elems = need_tab ? round_up(((size_t)n + frames) * sizeof(MaskRef), 256) / sizeof(float) : 0;
    bool cap = false;
    if ((rc = capturing(h, cap))) return rc;
    if (cap && tab_elems > h->arena_elems)
        return fail(h, CVS_E_UNSUPPORTED, "cvs_chain_refine_batch would have to grow the handle's scratch during capture: call once eagerly first");
    Call c;
    if ((rc = begin(h, c, {}, stage + tab_elems))) return rc;
    hipStream_t s = h->stream;
    RefineBatchArgs a{};
    a.rows = rows;
    a.cols = cols;
    a.n = n;
    a.n_maps = n_maps;
    a.n_points = n_points;
    Staged st(h, "cvs_chain_refine_batch", host);   // (the arrays; the planes go through the arena)
    st.in(a.points, points, (size_t)n_points * 8);
    st.in(a.ranges, ranges, ((size_t)n + 1) * 8);
    st.out(a.xy, xy, (size_t)n_points * 8);
    st.out(a.strength, strength, (size_t)n_points * 4);
    if ((rc = st.commit()) || (rc = st.upload(s))) return rc;
    MaskRef* tab = need_tab ? reinterpret_cast<MaskRef*>(arena_take(h, tab_elems)) : nullptr;
    for (int k = 0; k < n + frames; ++k) {
        PlaneRef r;
        if ((rc = in_ref(c, k < n ? &maps[k] : &theta[k - n], r))) return rc;
        (k < n ? dm[k] : dt[k - n]) = MaskRef{r.p, r.pitch, 0};
    }
    if ((rc = plane_set(h, dm, tab, a.maps)) || (rc = plane_set(h, dt, tab + n, a.theta))) return rc;
    HIP_TRY(h, launch_chain_refine_batch(a, s));
    if ((rc = st.download(s))) return rc;
    if (sync) HIP_TRY(h, hipStreamSynchronize(s));
    return CVS_OK;
}

}  // extern "C"
