// cvs_polyline.cpp -- the C ABI of the contour polylines (extension): cvs_chain_polylines.  Argument checks, the check of a host table, the
// handle's scratch (cvs_context::ch_scr: a chains call before this one has finished with it), staging of host arrays and the launch sequence
// of cvs_kernels_polyline.hip.  No arithmetic on coordinates happens here.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>

#include "cvs_contour_host.h"
#include "cvs_polyline.h"

using namespace cvs;

static_assert(sizeof(cvs_chain) == 16, "cvs_chain: four 4-byte fields (k_pl_apply writes it as four words)");

int cvs_chain_polylines(cvs_handle h, const int32_t* points, int n_points, const cvs_chain* chains, int n_chains, float eps, int32_t* vertices,
                        int vertex_capacity, int32_t* index, cvs_chain* polylines, int mem, int* n_vertices)
{
    if (!h) return CVS_E_BADARG;
    if (!n_vertices) return fail(h, CVS_E_BADARG, "n_vertices is required");
    if (!(eps >= 0.0f)) return fail(h, CVS_E_BADARG, "eps is NaN or negative");
    if (n_points < 0 || n_chains < 0 || vertex_capacity < 0) return fail(h, CVS_E_BADARG, "n_points, n_chains and vertex_capacity are >= 0");
    if ((n_points > 0 && !points) || (n_chains > 0 && !chains)) return fail(h, CVS_E_BADARG, "points / chains missing");
    if (vertex_capacity > 0 && (!vertices || (n_chains > 0 && !polylines)))
        return fail(h, CVS_E_BADARG, "vertices and polylines for a vertex_capacity > 0");
    if (mem != CVS_MEM_HOST && mem != CVS_MEM_DEVICE) return fail(h, CVS_E_BADARG, "mem");
    if (misaligned(points) || misaligned(chains) || misaligned(vertices) || misaligned(index) || misaligned(polylines))
        return fail(h, CVS_E_BADARG, "an array is not aligned to 4 bytes");
    if (n_points > (1 << 30)) return fail(h, CVS_E_SIZE, "more than 2^30 points");
    const bool host = mem == CVS_MEM_HOST;
    if (host)
        if (const char* what = chain_table_outside(n_points, reinterpret_cast<const int32_t*>(chains), n_chains)) return fail(h, CVS_E_BADARG, what);
    int rc;
    if ((rc = refuse_capture(h, "cvs_chain_polylines reads its count back: not capturable"))) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    h->used = true;
    if (n_chains == 0) {
        *n_vertices = 0;
        return CVS_OK;
    }

    // n_vertices <= n_points: the staged outputs never need more than that
    const int cap_v = std::min(vertex_capacity, n_points), blocks = pl_scan_blocks(n_chains);
    hipStream_t s = h->stream;
    uint8_t* keep;
    int32_t *cnt, *part, *dvtx, *didx, *dpol;
    const int32_t *dpts, *dchn;
    Staged st(h, "cvs_chain_polylines", host);
    st.scratch(keep, (size_t)n_points);
    st.scratch(cnt, (size_t)n_chains * 4);
    st.scratch(part, ((size_t)blocks + 1) * 4);
    st.in(dpts, points, (size_t)n_points * 8);
    st.in(dchn, chains, (size_t)n_chains * sizeof(cvs_chain));
    st.out(dvtx, vertices, (size_t)cap_v * 8);   // (fetched below, once the count is known: `total` records, not cap_v)
    st.out(didx, index, (size_t)cap_v * 4);
    st.out(dpol, polylines, (size_t)n_chains * sizeof(cvs_chain));
    if ((rc = st.commit()) || (rc = st.upload(s))) return rc;

    // the launch sequence: a function of (n_points, n_chains) alone; the kernels themselves hold back every store when the total does not fit
    const double e2 = (double)eps * (double)eps;
    const int cap_k = host ? cap_v : vertex_capacity;
    HIP_TRY(h, launch_pl_keep_wave(dpts, n_points, dchn, n_chains, e2, keep, cnt, s));
    HIP_TRY(h, launch_pl_keep_block(dpts, n_points, dchn, n_chains, e2, keep, cnt, s));
    HIP_TRY(h, launch_pl_count(cnt, n_chains, part, s));
    HIP_TRY(h, launch_scan_partials(part, blocks, s));
    HIP_TRY(h, launch_pl_apply(cnt, n_chains, part, dchn, cap_k, polylines ? dpol : nullptr, s));
    if (cap_k > 0) {
        HIP_TRY(h, launch_pl_emit_wave(dpts, n_points, dchn, n_chains, keep, cnt, part, cap_k, dvtx, didx, s));
        HIP_TRY(h, launch_pl_emit_block(dpts, n_points, dchn, n_chains, keep, cnt, part, cap_k, dvtx, didx, s));
    }
    int total = 0;
    HIP_TRY(h, hipMemcpyAsync(&total, part + blocks, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    *n_vertices = total;
    if (total < 0 || total > vertex_capacity) return fail(h, CVS_E_SIZE, "more vertices than vertex_capacity (n_vertices says how many)");
    if (host) {
        if (total) HIP_TRY(h, hipMemcpyAsync(vertices, dvtx, (size_t)total * 8, hipMemcpyDeviceToHost, s));
        if (total && index) HIP_TRY(h, hipMemcpyAsync(index, didx, (size_t)total * 4, hipMemcpyDeviceToHost, s));
        if (polylines) HIP_TRY(h, hipMemcpyAsync(polylines, dpol, (size_t)n_chains * sizeof(cvs_chain), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
    }
    return CVS_OK;
}
