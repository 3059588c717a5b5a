// cvs_chains.cpp -- the C ABI of the contour chains (extension): cvs_contour_chains.  Argument checks, the handle's scratch (the planes in
// cvs_context::cc_scr, the arc arrays in cvs_context::ch_scr), staging of host planes and lists, and the launch sequence of
// cvs_kernels_chains.hip.  No arithmetic on image data happens here, and no loop over chains or pixels.
#include <hip/hip_runtime_api.h>

#include <algorithm>

#include "cvs_chains.h"
#include "cvs_contour_host.h"

using namespace cvs;

static_assert(sizeof(cvs_chain) == 16, "cvs_chain: four 4-byte fields (k_ch_head_apply writes it as four words)");
static_assert(CVS_CHAIN_CLOSED == kChainClosed && CVS_CHAIN_HEAD_JUNCTION == kChainHeadJunction && CVS_CHAIN_TAIL_JUNCTION == kChainTailJunction,
              "the kernels' flag values are the public ones");

namespace {

int ceil_log2(int n)
{
    int r = 0;
    while ((1LL << r) < n) ++r;
    return r;
}

}  // namespace

int cvs_contour_chains(cvs_handle h, const cvs_plane* mask, int32_t* points, int point_capacity, cvs_chain* chains, int chain_capacity, int mem,
                       int* n_points, int* n_chains)
{
    if (!h) return CVS_E_BADARG;
    int rc;
    if ((rc = need_image(h))) return rc;
    if ((long long)h->rows * h->cols > (1LL << 28)) return fail(h, CVS_E_SIZE, "more than 2^28 pixels");
    if ((rc = check_sized(h, mask, "mask", h->rows, h->cols, true))) return rc;
    if (!n_points || !n_chains) return fail(h, CVS_E_BADARG, "n_points and n_chains are required");
    if (point_capacity < 0 || (point_capacity > 0 && !points)) return fail(h, CVS_E_BADARG, "point_capacity >= 0, and points for a capacity > 0");
    if (chain_capacity < 0 || (chain_capacity > 0 && !chains)) return fail(h, CVS_E_BADARG, "chain_capacity >= 0, and chains for a capacity > 0");
    if (mem != CVS_MEM_HOST && mem != CVS_MEM_DEVICE) return fail(h, CVS_E_BADARG, "mem");
    if (reinterpret_cast<uintptr_t>(points) % alignof(int32_t) || reinterpret_cast<uintptr_t>(chains) % alignof(int32_t))
        return fail(h, CVS_E_BADARG, "points / chains not aligned to 4 bytes");
    if ((rc = refuse_capture(h, "cvs_contour_chains reads its counts back: not capturable"))) return rc;

    const int rows = h->rows, cols = h->cols, blocks = scan_blocks(rows, cols);
    const size_t npix = (size_t)rows * cols;
    hipStream_t s = h->stream;

    // ---- the planes: links, components, nodes, and the counters every size follows from ----
    Scratch sc;
    const size_t o_parent = sc.reserve(npix * 4), o_aux = sc.reserve(npix * 4), o_link = sc.reserve(npix * 2);
    const size_t o_cnt = sc.reserve(kChCounters * 4), o_part = sc.reserve(((size_t)blocks + 1) * 4);
    Call c;
    if ((rc = begin(h, c, {direct_u8(mask) ? nullptr : mask}))) return rc;
    if ((rc = grow_cc(h, sc.need))) return rc;
    int32_t* parent = reinterpret_cast<int32_t*>(h->cc_scr + o_parent);
    int32_t* aux = reinterpret_cast<int32_t*>(h->cc_scr + o_aux);   // first the node flags at the roots, then the arc bases
    uint16_t* link = reinterpret_cast<uint16_t*>(h->cc_scr + o_link);
    int32_t* dcnt = reinterpret_cast<int32_t*>(h->cc_scr + o_cnt);
    int32_t* part = reinterpret_cast<int32_t*>(h->cc_scr + o_part);

    MaskRef m;
    if ((rc = mask_ref(c, mask, m))) return rc;
    HIP_TRY(h, launch_zero_ints(dcnt, kChCounters, s));
    HIP_TRY(h, launch_ch_links(m, rows, cols, link, s));
    HIP_TRY(h, launch_cc_tiles(m, rows, cols, parent, aux, nullptr, s));
    HIP_TRY(h, launch_cc_borders(rows, cols, parent, s));
    HIP_TRY(h, launch_ch_nodes(rows, cols, link, parent, aux, s));
    HIP_TRY(h, launch_ch_roots(rows, cols, link, parent, aux, dcnt, s));
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
    if (arcs == 0) return CVS_OK;

    // ---- the arcs: sized by the count just read ----
    const bool host = mem == CVS_MEM_HOST;
    const int ablocks = ch_scan_blocks(arcs);
    Scratch sa;
    const size_t o_to = sa.reserve((size_t)arcs * 4), o_rev = sa.reserve((size_t)arcs * 4);
    const size_t o_rec0 = sa.reserve((size_t)arcs * sizeof(ArcRec)), o_rec1 = sa.reserve((size_t)arcs * sizeof(ArcRec));
    const size_t o_pn = sa.reserve(((size_t)ablocks + 1) * 4), o_pl = sa.reserve(((size_t)ablocks + 1) * 4);
    const size_t o_pts = host ? sa.reserve((size_t)total_points * 8) : 0, o_chn = host ? sa.reserve((size_t)total_chains * sizeof(cvs_chain)) : 0;
    if ((rc = grow_scratch(h, "hipMalloc(&h->ch_scr, need)", h->ch_scr, h->ch_scr_bytes, sa.need, 1))) return rc;
    int32_t* to = reinterpret_cast<int32_t*>(h->ch_scr + o_to);
    int32_t* rev = reinterpret_cast<int32_t*>(h->ch_scr + o_rev);
    ArcRec* rec[2] = {reinterpret_cast<ArcRec*>(h->ch_scr + o_rec0), reinterpret_cast<ArcRec*>(h->ch_scr + o_rec1)};
    int32_t* part_n = reinterpret_cast<int32_t*>(h->ch_scr + o_pn);
    int32_t* part_len = reinterpret_cast<int32_t*>(h->ch_scr + o_pl);
    int32_t* dpts = host ? reinterpret_cast<int32_t*>(h->ch_scr + o_pts) : points;
    int32_t* dchn = host ? reinterpret_cast<int32_t*>(h->ch_scr + o_chn) : reinterpret_cast<int32_t*>(chains);

    HIP_TRY(h, launch_ch_arc_count(rows, cols, link, part, s));
    HIP_TRY(h, launch_scan_partials(part, blocks, s));
    HIP_TRY(h, launch_ch_arc_base(rows, cols, link, part, aux, s));
    HIP_TRY(h, launch_ch_arcs(rows, cols, link, aux, arcs, to, rev, rec[0], s));
    const int rounds = ceil_log2(arcs);   // no direction is longer than all the arcs there are
    for (int r = 0; r < rounds; ++r) HIP_TRY(h, launch_ch_jump(arcs, rec[r & 1], rec[(r + 1) & 1], s));
    const ArcRec* ranked = rec[rounds & 1];
    HeadRec* head = reinterpret_cast<HeadRec*>(rec[(rounds + 1) & 1]);   // the buffer the ranking has left over
    static_assert(sizeof(HeadRec) == sizeof(ArcRec), "the head records live in the spare ranking buffer");
    HIP_TRY(h, launch_ch_heads(arcs, link, to, rev, ranked, head, s));
    HIP_TRY(h, launch_ch_head_count(arcs, head, part_n, part_len, s));
    HIP_TRY(h, launch_scan_partials(part_n, ablocks, s));
    HIP_TRY(h, launch_scan_partials(part_len, ablocks, s));
    HIP_TRY(h, launch_ch_head_apply(arcs, head, part_n, part_len, dchn, total_chains, s));
    HIP_TRY(h, launch_ch_emit(arcs, cols, to, rev, ranked, head, dpts, total_points, s));
    if (host) {
        HIP_TRY(h, hipMemcpyAsync(points, dpts, (size_t)total_points * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(chains, dchn, (size_t)total_chains * sizeof(cvs_chain), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    return CVS_OK;
}
