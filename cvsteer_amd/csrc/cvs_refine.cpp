// cvs_refine.cpp -- the C ABI of the contour edgels (extension): cvs_chain_refine and cvs_chain_measures.  Argument checks, the check of a
// host point list and of a host table, staging of host arrays in the handle's scratch (cvs_context::ch_scr) and of host planes in the
// arena, and the launches of cvs_kernels_refine.hip.  Neither call reads anything back; no arithmetic on coordinates or values happens here.
#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "cvs_contour_host.h"
#include "cvs_refine.h"

using namespace cvs;

static_assert(sizeof(cvs_chain_measure) == kMeasureWords * 4 && offsetof(cvs_chain_measure, peak_index) == 12 &&
                  offsetof(cvs_chain_measure, peak) == 16 && offsetof(cvs_chain_measure, weakest) == 20 &&
                  offsetof(cvs_chain_measure, sum) == 24 && offsetof(cvs_chain_measure, length) == 32,
              "cvs_chain_measure: the ten words ms_store writes");

namespace {

bool misaligned(const void* p) { return reinterpret_cast<uintptr_t>(p) % alignof(int32_t) != 0; }

// an array of `n` records of `words` 4-byte words as a plane, for the overlap rule of the contour tail (check_disjoint)
cvs_plane array_plane(const void* p, int n, int words, int mem)
{
    cvs_plane q{};
    q.data = n > 0 ? const_cast<float*>(static_cast<const float*>(p)) : nullptr;
    q.rows = n;
    q.cols = words;
    q.step = (size_t)words * 4;
    q.mem = mem;
    return q;
}

}  // namespace

int cvs_chain_refine(cvs_handle h, const cvs_plane* map, const cvs_plane* theta, const int32_t* points, int n_points, float* xy, float* strength,
                     int mem)
{
    if (!h) return CVS_E_BADARG;
    if (n_points < 0) return fail(h, CVS_E_BADARG, "n_points is >= 0");
    if (mem != CVS_MEM_HOST && mem != CVS_MEM_DEVICE) return fail(h, CVS_E_BADARG, "mem");
    int rc;
    if (!theta && (rc = need_state(h, true))) return rc;
    if ((rc = need_image(h))) return rc;
    if ((rc = check_sized(h, map, "map", h->rows, h->cols))) return rc;
    if (theta && (rc = check_sized(h, theta, "theta", h->rows, h->cols))) return rc;
    if (n_points > 0 && (!points || !xy)) return fail(h, CVS_E_BADARG, "points / xy missing");
    if (misaligned(points) || misaligned(xy) || misaligned(strength)) return fail(h, CVS_E_BADARG, "an array is not aligned to 4 bytes");
    if (n_points > (1 << 30)) return fail(h, CVS_E_SIZE, "more than 2^30 points");
    // theta == NULL: the handle's own theta plane of the selected frame -- an output must not overlap that either
    const PlaneRef own = theta ? PlaneRef{nullptr, 0} : state_ref(h, h->nb + 3);
    const cvs_plane ins[3] = {array_plane(points, n_points, 2, mem), *map, theta ? *theta : device_plane(own.p, h->rows, h->cols, own.pitch)};
    const cvs_plane outs[2] = {array_plane(xy, n_points, 2, mem), array_plane(strength, strength ? n_points : 0, 1, mem)};
    if ((rc = check_disjoint(h, ins, 3, outs, 2))) return rc;
    const bool host = mem == CVS_MEM_HOST;
    if (host)
        for (int i = 0; i < n_points; ++i)
            if ((unsigned)points[2 * (size_t)i] >= (unsigned)h->cols || (unsigned)points[2 * (size_t)i + 1] >= (unsigned)h->rows)
                return fail(h, CVS_E_BADARG, "a point lies outside the image");
    const bool sync = host || mem_of(map) == CVS_MEM_HOST || (theta && mem_of(theta) == CVS_MEM_HOST);
    if (sync && (rc = refuse_capture(h, "cvs_chain_refine stages host memory and synchronises: not capturable"))) return rc;
    if (n_points == 0) return CVS_OK;

    Call c;
    if ((rc = begin(h, c, {map, theta}))) return rc;
    hipStream_t s = h->stream;
    RefineArgs a{};
    a.rows = h->rows;
    a.cols = h->cols;
    a.n_points = n_points;
    a.points = points;
    a.xy = xy;
    a.strength = strength;
    if (host) {
        Scratch sc;
        const size_t o_pts = sc.reserve((size_t)n_points * 8), o_xy = sc.reserve((size_t)n_points * 8), o_str = sc.reserve((size_t)n_points * 4);
        if ((rc = grow_scratch(h, "hipMalloc(&h->ch_scr, need)", h->ch_scr, h->ch_scr_bytes, sc.need, 1))) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->ch_scr + o_pts, points, (size_t)n_points * 8, hipMemcpyHostToDevice, s));
        a.points = reinterpret_cast<const int32_t*>(h->ch_scr + o_pts);
        a.xy = reinterpret_cast<float*>(h->ch_scr + o_xy);
        a.strength = strength ? reinterpret_cast<float*>(h->ch_scr + o_str) : nullptr;
    }
    if ((rc = in_ref(c, map, a.map))) return rc;
    if (theta) {
        if ((rc = in_ref(c, theta, a.theta))) return rc;
    } else {
        a.theta = own;
    }
    HIP_TRY(h, launch_chain_refine(a, s));
    if (host) {
        HIP_TRY(h, hipMemcpyAsync(xy, a.xy, (size_t)n_points * 8, hipMemcpyDeviceToHost, s));
        if (strength) HIP_TRY(h, hipMemcpyAsync(strength, a.strength, (size_t)n_points * 4, hipMemcpyDeviceToHost, s));
    }
    if (sync) HIP_TRY(h, hipStreamSynchronize(s));
    return CVS_OK;
}

int cvs_chain_measures(cvs_handle h, const int32_t* points, int n_points, const cvs_chain* chains, int n_chains, const float* xy,
                       const float* strength, cvs_chain_measure* table, int mem)
{
    if (!h) return CVS_E_BADARG;
    if (n_points < 0 || n_chains < 0) return fail(h, CVS_E_BADARG, "n_points and n_chains are >= 0");
    if ((n_points > 0 && !points) || (n_chains > 0 && (!chains || !table))) return fail(h, CVS_E_BADARG, "points / chains / table missing");
    if (mem != CVS_MEM_HOST && mem != CVS_MEM_DEVICE) return fail(h, CVS_E_BADARG, "mem");
    if (misaligned(points) || misaligned(chains) || misaligned(xy) || misaligned(strength) || misaligned(table))
        return fail(h, CVS_E_BADARG, "an array is not aligned to 4 bytes");
    if (n_points > (1 << 30)) return fail(h, CVS_E_SIZE, "more than 2^30 points");
    const cvs_plane ins[4] = {array_plane(points, n_points, 2, mem), array_plane(chains, n_chains, 4, mem),
                              array_plane(xy, xy ? n_points : 0, 2, mem), array_plane(strength, strength ? n_points : 0, 1, mem)};
    const cvs_plane out = array_plane(table, n_chains, kMeasureWords, mem);
    int rc;
    if ((rc = check_disjoint(h, ins, 4, &out, 1))) return rc;
    const bool host = mem == CVS_MEM_HOST;
    if (host)
        for (int c = 0; c < n_chains; ++c)
            if (chains[c].start < 0 || chains[c].length < 1 || (long long)chains[c].start + chains[c].length > n_points)
                return fail(h, CVS_E_BADARG, "a chain does not lie inside points");
    if (host && (rc = refuse_capture(h, "cvs_chain_measures stages host memory and synchronises: not capturable"))) return rc;
    if (n_chains == 0) return CVS_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    h->used = true;

    hipStream_t s = h->stream;
    MeasureArgs a{};
    a.points = points;
    a.n_points = n_points;
    a.chains = reinterpret_cast<const int32_t*>(chains);
    a.n_chains = n_chains;
    a.xy = xy;
    a.strength = strength;
    a.table = reinterpret_cast<uint32_t*>(table);
    if (host) {
        Scratch sc;
        const size_t o_pts = sc.reserve((size_t)n_points * 8), o_chn = sc.reserve((size_t)n_chains * sizeof(cvs_chain));
        const size_t o_xy = sc.reserve(xy ? (size_t)n_points * 8 : 0), o_str = sc.reserve(strength ? (size_t)n_points * 4 : 0);
        const size_t o_tab = sc.reserve((size_t)n_chains * sizeof(cvs_chain_measure));
        if ((rc = grow_scratch(h, "hipMalloc(&h->ch_scr, need)", h->ch_scr, h->ch_scr_bytes, sc.need, 1))) return rc;
        if (n_points) HIP_TRY(h, hipMemcpyAsync(h->ch_scr + o_pts, points, (size_t)n_points * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(h->ch_scr + o_chn, chains, (size_t)n_chains * sizeof(cvs_chain), hipMemcpyHostToDevice, s));
        if (xy && n_points) HIP_TRY(h, hipMemcpyAsync(h->ch_scr + o_xy, xy, (size_t)n_points * 8, hipMemcpyHostToDevice, s));
        if (strength && n_points) HIP_TRY(h, hipMemcpyAsync(h->ch_scr + o_str, strength, (size_t)n_points * 4, hipMemcpyHostToDevice, s));
        a.points = reinterpret_cast<const int32_t*>(h->ch_scr + o_pts);
        a.chains = reinterpret_cast<const int32_t*>(h->ch_scr + o_chn);
        a.xy = xy ? reinterpret_cast<const float*>(h->ch_scr + o_xy) : nullptr;
        a.strength = strength ? reinterpret_cast<const float*>(h->ch_scr + o_str) : nullptr;
        a.table = reinterpret_cast<uint32_t*>(h->ch_scr + o_tab);
    }
    // two launches for any table: the launch sequence is a function of (n_points, n_chains) alone
    HIP_TRY(h, launch_measure_wave(a, s));
    HIP_TRY(h, launch_measure_block(a, s));
    if (host) {
        HIP_TRY(h, hipMemcpyAsync(table, a.table, (size_t)n_chains * sizeof(cvs_chain_measure), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
    }
    return CVS_OK;
}
