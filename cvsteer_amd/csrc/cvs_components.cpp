// cvs_components.cpp -- the C ABI of the contour components (extension): cvs_label, cvs_component_stats, cvs_contour_prune and
// cvs_contour_points.  Argument checks, the handle's scratch (cvs_context::cc_scr), staging of host planes, and the fixed launch
// sequences of cvs_kernels_components.hip.  No arithmetic on image data happens here.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "cvs_contour_host.h"

using namespace cvs;

namespace {

bool is_s32(const cvs_plane* p) { return (p->mem & CVS_DEPTH_S32) != 0; }

// a CVS_DEPTH_S32 plane: what check_plane asks of an f32 plane, for the int32 depth
int check_s32(cvs_handle h, const cvs_plane* p, const char* name)
{
    if (!p) return fail(h, CVS_E_BADARG, name);
    if (p->rows <= 0 || p->cols <= 0) return fail(h, CVS_E_SIZE, "empty plane");
    if (!p->data) return fail(h, CVS_E_BADARG, name);
    if ((p->mem & ~0xff) != CVS_DEPTH_S32) return fail(h, CVS_E_BADARG, "the plane must be CVS_DEPTH_S32");
    if (mem_of(p) != CVS_MEM_HOST && mem_of(p) != CVS_MEM_DEVICE) return fail(h, CVS_E_BADARG, "bad mem kind");
    if (p->step < (size_t)p->cols * sizeof(int32_t) || p->step % sizeof(int32_t)) return fail(h, CVS_E_SIZE, "bad step");
    if (reinterpret_cast<uintptr_t>(p->data) % alignof(int32_t)) return fail(h, CVS_E_BADARG, "s32 plane not aligned to 4 bytes");
    return CVS_OK;
}

// the same plane as the staging helpers see it: four bytes per pixel, no depth flag (in_ref / out_ref copy bytes, whatever they mean)
cvs_plane as_words(const cvs_plane* p)
{
    cvs_plane q = *p;
    q.mem = mem_of(p);
    return q;
}

// before any plane is looked at: the handle has an image size, and its pixels can be indexed with an int32
int need_size(cvs_handle h)
{
    const int rc = need_image(h);
    if (rc) return rc;
    if ((long long)h->rows * h->cols > 0x7fffffffLL - 1) return fail(h, CVS_E_SIZE, "more than 2^31 - 2 pixels");
    return CVS_OK;
}

// what begin() must reserve in the staging arena for a mask
const cvs_plane* staged(const cvs_plane* p) { return direct_u8(p) ? nullptr : p; }

// steps 1 and 2 on the handle's stream
int build_parents(cvs_handle h, const MaskRef& m, int32_t* parent, int32_t* zero_a, uint32_t* zero_b)
{
    HIP_TRY(h, launch_cc_tiles(m, h->rows, h->cols, parent, zero_a, zero_b, h->stream));
    HIP_TRY(h, launch_cc_borders(h->rows, h->cols, parent, h->stream));
    return CVS_OK;
}

}  // namespace

int cvs_label(cvs_handle h, const cvs_plane* mask, const cvs_plane* labels, int* count)
{
    if (!h) return CVS_E_BADARG;
    int rc;
    if ((rc = need_size(h))) return rc;
    if ((rc = check_sized(h, mask, "mask", h->rows, h->cols, true))) return rc;
    if (!labels) return fail(h, CVS_E_BADARG, "labels");
    if (!is_s32(labels)) return fail(h, CVS_E_BADARG, "labels must be a CVS_DEPTH_S32 plane");
    if ((rc = check_s32(h, labels, "labels")) || (rc = check_same(h, labels, h->rows, h->cols))) return rc;
    if (planes_overlap(mask, labels)) return fail(h, CVS_E_BADARG, "labels overlaps the mask");
    if ((rc = refuse_capture(h, "cvs_label reads the count back: not capturable"))) return rc;

    const int rows = h->rows, cols = h->cols, blocks = scan_blocks(rows, cols);
    const size_t npix = (size_t)rows * cols;
    Scratch sc;
    const size_t o_parent = sc.reserve(npix * 4), o_rank = sc.reserve(npix * 4), o_part = sc.reserve(((size_t)blocks + 1) * 4);
    if ((rc = grow_cc(h, sc.need))) return rc;
    int32_t* parent = reinterpret_cast<int32_t*>(h->cc_scr + o_parent);
    int32_t* rank = reinterpret_cast<int32_t*>(h->cc_scr + o_rank);
    int32_t* part = reinterpret_cast<int32_t*>(h->cc_scr + o_part);

    const cvs_plane lab_w = as_words(labels);
    Call c;
    if ((rc = begin(h, c, {staged(mask), &lab_w}))) return rc;
    MaskRef m;
    PlaneRef lr;
    if ((rc = mask_ref(c, mask, m)) || (rc = out_ref(c, &lab_w, lr))) return rc;
    const IntPlane lab = {reinterpret_cast<int32_t*>(lr.p), lr.pitch};
    if ((rc = build_parents(h, m, parent, nullptr, nullptr))) return rc;
    // dense numbering: the roots are the pixels that are their own parent; their exclusive scan in raster order is the label - 1
    const IntPlane pp = {parent, (size_t)cols};
    HIP_TRY(h, launch_scan_count(kScanRoots, pp, rows, cols, part, h->stream));
    HIP_TRY(h, launch_scan_partials(part, blocks, h->stream));
    HIP_TRY(h, launch_scan_apply(kScanRoots, pp, rows, cols, part, rank, h->stream));
    HIP_TRY(h, launch_cc_relabel(rows, cols, parent, rank, lab, h->stream));
    int total = 0;
    HIP_TRY(h, hipMemcpyAsync(&total, part + blocks, sizeof(total), hipMemcpyDeviceToHost, h->stream));
    if ((rc = finish(c))) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (count) *count = total;
    return CVS_OK;
}

int cvs_component_stats(cvs_handle h, const cvs_plane* labels, int count, const cvs_plane* weight, cvs_component* table, int table_mem)
{
    static_assert(sizeof(cvs_component) == 40, "cvs_component: ten 4-byte fields (k_stats_table writes it as ten words)");
    if (!h) return CVS_E_BADARG;
    int rc;
    if ((rc = need_size(h))) return rc;
    if (!labels) return fail(h, CVS_E_BADARG, "labels");
    if (!is_s32(labels)) return fail(h, CVS_E_BADARG, "labels must be a CVS_DEPTH_S32 plane");
    if ((rc = check_s32(h, labels, "labels")) || (rc = check_same(h, labels, h->rows, h->cols))) return rc;
    if (weight && (rc = check_sized(h, weight, "weight", h->rows, h->cols))) return rc;
    if (count < 0 || (count > 0 && !table)) return fail(h, CVS_E_BADARG, "count >= 0, and a table for count > 0");
    if (table_mem != CVS_MEM_HOST && table_mem != CVS_MEM_DEVICE) return fail(h, CVS_E_BADARG, "table_mem");
    if (reinterpret_cast<uintptr_t>(table) % alignof(int32_t)) return fail(h, CVS_E_BADARG, "table not aligned to 4 bytes");
    if ((rc = refuse_capture(h, "cvs_component_stats returns with the table written: not capturable"))) return rc;
    if (count == 0) return CVS_OK;

    const int rows = h->rows, cols = h->cols;
    const bool host_table = table_mem == CVS_MEM_HOST;
    Scratch sc;
    const size_t o_acc = sc.reserve((size_t)count * sizeof(CcAcc));
    const size_t o_tab = host_table ? sc.reserve((size_t)count * sizeof(cvs_component)) : 0;
    if ((rc = grow_cc(h, sc.need))) return rc;
    CcAcc* acc = reinterpret_cast<CcAcc*>(h->cc_scr + o_acc);
    void* dtab = host_table ? static_cast<void*>(h->cc_scr + o_tab) : static_cast<void*>(table);

    const cvs_plane lab_w = as_words(labels);
    Call c;
    if ((rc = begin(h, c, {&lab_w, weight}))) return rc;
    PlaneRef lr, wr = {nullptr, 0};
    if ((rc = in_ref(c, &lab_w, lr))) return rc;
    if (weight && (rc = in_ref(c, weight, wr))) return rc;
    const IntPlane lab = {reinterpret_cast<int32_t*>(lr.p), lr.pitch};
    HIP_TRY(h, launch_stats_init(acc, count, h->stream));
    HIP_TRY(h, launch_stats(lab, rows, cols, count, wr, acc, h->stream));
    HIP_TRY(h, launch_stats_table(acc, count, cols, dtab, h->stream));
    if (host_table) HIP_TRY(h, hipMemcpyAsync(table, dtab, (size_t)count * sizeof(cvs_component), hipMemcpyDeviceToHost, h->stream));
    if ((rc = finish(c))) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return CVS_OK;
}

int cvs_contour_prune(cvs_handle h, int n, const cvs_plane* mask, const cvs_plane* weight, int min_area, float min_peak,
                      const cvs_plane* out, int* kept)
{
    if (!h) return CVS_E_BADARG;
    if (n < 1 || !mask || !out) return fail(h, CVS_E_BADARG, "n >= 1 planes, mask and out are required");
    if (min_area < 0 || std::isnan(min_peak)) return fail(h, CVS_E_BADARG, "min_area >= 0, min_peak not NaN");
    int rc;
    if ((rc = need_size(h))) return rc;
    const bool u8 = is_u8(&out[0]);
    for (int k = 0; k < n; ++k) {
        if ((rc = check_sized(h, &mask[k], "mask", h->rows, h->cols, true))) return rc;
        if (weight && (rc = check_sized(h, &weight[k], "weight", h->rows, h->cols))) return rc;
        if ((rc = check_sized(h, &out[k], "out", h->rows, h->cols, true))) return rc;
        if (is_u8(&out[k]) != u8) return fail(h, CVS_E_BADARG, "the outputs are all bytes or all f32");
    }
    std::vector<cvs_plane> ins(mask, mask + n);
    if (weight) ins.insert(ins.end(), weight, weight + n);
    if ((rc = check_disjoint(h, ins.data(), ins.size(), out, (size_t)n))) return rc;
    if ((rc = refuse_capture(h, "cvs_contour_prune reads its counts back: not capturable"))) return rc;

    const int rows = h->rows, cols = h->cols;
    const size_t npix = (size_t)rows * cols, bpitch = round_up((size_t)cols, 64);
    Scratch sc;
    const size_t o_parent = sc.reserve(npix * 4), o_root = sc.reserve(npix * 4), o_area = sc.reserve(npix * 4);
    const size_t o_peak = weight ? sc.reserve(npix * 4) : 0;
    const size_t o_kept = sc.reserve((size_t)n * 4);
    const size_t o_bytes = u8 ? sc.reserve(bpitch * rows) : 0;   // host byte outputs are staged here
    if ((rc = grow_cc(h, sc.need))) return rc;
    int32_t* parent = reinterpret_cast<int32_t*>(h->cc_scr + o_parent);
    int32_t* root = reinterpret_cast<int32_t*>(h->cc_scr + o_root);
    int32_t* area = reinterpret_cast<int32_t*>(h->cc_scr + o_area);
    uint32_t* peak = weight ? reinterpret_cast<uint32_t*>(h->cc_scr + o_peak) : nullptr;
    int32_t* dkept = reinterpret_cast<int32_t*>(h->cc_scr + o_kept);
    unsigned char* dbytes = h->cc_scr + o_bytes;

    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, launch_zero_ints(dkept, n, h->stream));
    for (int k = 0; k < n; ++k) {
        const cvs_plane* o = &out[k];
        Call c;
        if ((rc = begin(h, c, {staged(&mask[k]), weight ? &weight[k] : nullptr, u8 ? nullptr : o}))) return rc;
        MaskRef m;
        PlaneRef wr = {nullptr, 0};
        if ((rc = mask_ref(c, &mask[k], m))) return rc;
        if (weight && (rc = in_ref(c, &weight[k], wr))) return rc;
        PruneEmit e{};
        e.rows = rows;
        e.cols = cols;
        e.root = root;
        e.area = area;
        e.peak = peak;
        e.min_area = min_area;
        e.min_peak = min_peak;
        e.out_u8 = u8 ? 1 : 0;
        e.kept = dkept + k;
        if ((rc = mask_out(c, o, u8, dbytes, bpitch, e.out, e.out_pitch))) return rc;
        if ((rc = build_parents(h, m, parent, area, peak))) return rc;
        HIP_TRY(h, launch_cc_flatten(rows, cols, parent, root, h->stream));
        HIP_TRY(h, launch_prune_stats(rows, cols, root, wr, area, peak, h->stream));
        HIP_TRY(h, launch_prune_emit(e, h->stream));
        if ((rc = fetch_mask(c, o, u8, e.out, e.out_pitch)) || (rc = finish(c))) return rc;
        if (staged_bytes(o, u8)) HIP_TRY(h, hipStreamSynchronize(h->stream));   // the staging bytes are reused by the next plane
    }
    std::vector<int> counts((size_t)n);
    HIP_TRY(h, hipMemcpyAsync(counts.data(), dkept, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (kept)
        for (int k = 0; k < n; ++k) kept[k] = counts[(size_t)k];
    return CVS_OK;
}

int cvs_contour_points(cvs_handle h, const cvs_plane* labels, int32_t* points, int capacity, int points_mem, int* n_points)
{
    if (!h) return CVS_E_BADARG;
    int rc;
    if ((rc = need_size(h))) return rc;
    if (!labels || !n_points) return fail(h, CVS_E_BADARG, "labels and n_points are required");
    if (!is_s32(labels)) return fail(h, CVS_E_BADARG, "labels must be a CVS_DEPTH_S32 plane");
    if ((rc = check_s32(h, labels, "labels")) || (rc = check_same(h, labels, h->rows, h->cols))) return rc;
    if (capacity < 0 || (capacity > 0 && !points)) return fail(h, CVS_E_BADARG, "capacity >= 0, and points for capacity > 0");
    if (points_mem != CVS_MEM_HOST && points_mem != CVS_MEM_DEVICE) return fail(h, CVS_E_BADARG, "points_mem");
    if (reinterpret_cast<uintptr_t>(points) % alignof(int32_t)) return fail(h, CVS_E_BADARG, "points not aligned to 4 bytes");
    if ((rc = refuse_capture(h, "cvs_contour_points reads the number of points back: not capturable"))) return rc;

    const int rows = h->rows, cols = h->cols, blocks = scan_blocks(rows, cols);
    const bool host_points = points_mem == CVS_MEM_HOST;
    Scratch sc;
    const size_t o_part = sc.reserve(((size_t)blocks + 1) * 4);
    // host lists are staged behind the partials: at most what the caller has room for
    const size_t o_pts = host_points ? sc.reserve(std::min((size_t)capacity, (size_t)rows * cols) * 12) : 0;
    if ((rc = grow_cc(h, sc.need))) return rc;
    int32_t* part = reinterpret_cast<int32_t*>(h->cc_scr + o_part);
    int32_t* dpts = host_points ? reinterpret_cast<int32_t*>(h->cc_scr + o_pts) : points;

    const cvs_plane lab_w = as_words(labels);
    Call c;
    if ((rc = begin(h, c, {&lab_w}))) return rc;
    PlaneRef lr;
    if ((rc = in_ref(c, &lab_w, lr))) return rc;
    const IntPlane lab = {reinterpret_cast<int32_t*>(lr.p), lr.pitch};
    HIP_TRY(h, launch_scan_count(kScanNonZero, lab, rows, cols, part, h->stream));
    HIP_TRY(h, launch_scan_partials(part, blocks, h->stream));
    int total = 0;
    HIP_TRY(h, hipMemcpyAsync(&total, part + blocks, sizeof(total), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *n_points = total;
    if (total > capacity) return fail(h, CVS_E_SIZE, "more points than capacity (n_points says how many)");
    if (total == 0) return CVS_OK;
    HIP_TRY(h, launch_scan_apply(kScanNonZero, lab, rows, cols, part, dpts, h->stream));
    if (host_points) HIP_TRY(h, hipMemcpyAsync(points, dpts, (size_t)total * 12, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return CVS_OK;
}
