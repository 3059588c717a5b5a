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
    Staged st(h, "cvs_chain_refine", host);
    st.in(a.points, points, (size_t)n_points * 8);
    st.out(a.xy, xy, (size_t)n_points * 8);
    st.out(a.strength, strength, (size_t)n_points * 4);
    if ((rc = st.commit()) || (rc = st.upload(s))) return rc;
    if ((rc = in_ref(c, map, a.map))) return rc;
    if (theta) {
        if ((rc = in_ref(c, theta, a.theta))) return rc;
    } else {
        a.theta = own;
    }
    HIP_TRY(h, launch_chain_refine(a, s));
    if ((rc = st.download(s))) return rc;
    if (sync) HIP_TRY(h, hipStreamSynchronize(s));   // (a DEVICE call with a host plane waits too)
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
        if (const char* what = chain_table_outside(n_points, reinterpret_cast<const int32_t*>(chains), n_chains)) return fail(h, CVS_E_BADARG, what);
    if (host && (rc = refuse_capture(h, "cvs_chain_measures stages host memory and synchronises: not capturable"))) return rc;
    if (n_chains == 0) return CVS_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    h->used = true;

    hipStream_t s = h->stream;
    MeasureArgs a{};
    a.n_points = n_points;
    a.n_chains = n_chains;
    Staged st(h, "cvs_chain_measures", host);
    st.in(a.points, points, (size_t)n_points * 8);
    st.in(a.chains, chains, (size_t)n_chains * sizeof(cvs_chain));
    st.in(a.xy, xy, (size_t)n_points * 8);
    st.in(a.strength, strength, (size_t)n_points * 4);
    st.out(a.table, table, (size_t)n_chains * sizeof(cvs_chain_measure));
    if ((rc = st.commit()) || (rc = st.upload(s))) return rc;
    // two launches for any table: the launch sequence is a function of (n_points, n_chains) alone
    HIP_TRY(h, launch_measure_wave(a, s));
    HIP_TRY(h, launch_measure_block(a, s));
    return st.fetch(s);
}
