// cvs_segments.cpp -- the C ABI of the contour segments (extension): cvs_polyline_segments.  Argument checks, the check of host tables,
// staging of host arrays in the handle's scratch (cvs_context::ch_scr) and the two launches of cvs_kernels_segments.hip.  Nothing is read
// back; no arithmetic on coordinates or values happens here.
#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "cvs_contour_host.h"
#include "cvs_segments.h"

using namespace cvs;

static_assert(sizeof(cvs_segment) == kSegmentWords * 4 && offsetof(cvs_segment, flags) == 12 && offsetof(cvs_segment, w) == 16 &&
                  offsetof(cvs_segment, syy) == 56 && offsetof(cvs_segment, cx) == 64 && offsetof(cvs_segment, t0) == 96 &&
                  offsetof(cvs_segment, dmax) == 120,
              "cvs_segment: the thirty-two words sg_store writes");
static_assert(CVS_SEG_WRAPS == kSegWraps && CVS_SEG_DEGENERATE == kSegDegenerate, "the flags sg_store writes");

namespace {

// what a HOST call is refused for: nullptr if the three tables say what the contract says (entry by entry: the chain, then its polyline)
const char* host_tables_wrong(int n_points, const cvs_chain* chains, const cvs_chain* polylines, int n_chains, const int32_t* index,
                              int n_vertices)
{
    long long at = 0;
    for (int c = 0; c < n_chains; ++c) {
        const cvs_chain &t = chains[c], &p = polylines[c];
        if (const char* what = chain_entry_outside(n_points, reinterpret_cast<const int32_t*>(chains), (size_t)c)) return what;
        if (p.start != at || p.length < 0 || at + p.length > n_vertices) return "the polyline starts are not the running sum of the lengths";
        for (long long k = at; k < at + p.length; ++k) {
            if (index[k] < t.start || index[k] >= t.start + t.length) return "an index leaves its chain";
            if (k > at && index[k] <= index[k - 1]) return "the index does not increase inside a polyline";
        }
        at += p.length;
    }
    return at == n_vertices ? nullptr : "the polyline lengths do not add up to n_vertices";
}

}  // namespace

int cvs_polyline_segments(cvs_handle h, const int32_t* points, int n_points, const cvs_chain* chains, const cvs_chain* polylines, int n_chains,
                          const int32_t* index, int n_vertices, const float* xy, const float* strength, cvs_segment* table, int mem)
{
    if (!h) return CVS_E_BADARG;
    if (n_points < 0 || n_chains < 0 || n_vertices < 0) return fail(h, CVS_E_BADARG, "n_points, n_chains and n_vertices are >= 0");
    if ((n_points > 0 && !points) || (n_chains > 0 && (!chains || !polylines)) || (n_vertices > 0 && (!index || !table)))
        return fail(h, CVS_E_BADARG, "points / chains / polylines / index / table missing");
    if (mem != CVS_MEM_HOST && mem != CVS_MEM_DEVICE) return fail(h, CVS_E_BADARG, "mem");
    if (misaligned(points) || misaligned(chains) || misaligned(polylines) || misaligned(index) || misaligned(xy) || misaligned(strength))
        return fail(h, CVS_E_BADARG, "an array is not aligned to 4 bytes");
    if (misaligned(table, alignof(double))) return fail(h, CVS_E_BADARG, "table is not aligned to 8 bytes");
    if (n_points > (1 << 30)) return fail(h, CVS_E_SIZE, "more than 2^30 points");
    if (n_vertices > 0 && n_chains == 0) return fail(h, CVS_E_BADARG, "vertices without a polyline");
    const cvs_plane ins[6] = {array_plane(points, n_points, 2, mem),          array_plane(chains, n_chains, 4, mem),
                              array_plane(polylines, n_chains, 4, mem),       array_plane(index, n_vertices, 1, mem),
                              array_plane(xy, xy ? n_points : 0, 2, mem),     array_plane(strength, strength ? n_points : 0, 1, mem)};
    const cvs_plane out = array_plane(table, n_vertices, kSegmentWords, mem);
    int rc;
    if ((rc = check_disjoint(h, ins, 6, &out, 1))) return rc;
    const bool host = mem == CVS_MEM_HOST;
    if (host)
        if (const char* what = host_tables_wrong(n_points, chains, polylines, n_chains, index, n_vertices)) return fail(h, CVS_E_BADARG, what);
    if (host && (rc = refuse_capture(h, "cvs_polyline_segments stages host memory and synchronises: not capturable"))) return rc;
    if (n_vertices == 0) return CVS_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    h->used = true;

    hipStream_t s = h->stream;
    SegmentArgs a{};
    a.n_points = n_points;
    a.n_chains = n_chains;
    a.n_vertices = n_vertices;
    Staged st(h, "cvs_polyline_segments", host);
    st.in(a.points, points, (size_t)n_points * 8);
    st.in(a.chains, chains, (size_t)n_chains * sizeof(cvs_chain));
    st.in(a.polylines, polylines, (size_t)n_chains * sizeof(cvs_chain));
    st.in(a.index, index, (size_t)n_vertices * 4);
    st.in(a.xy, xy, (size_t)n_points * 8);
    st.in(a.strength, strength, (size_t)n_points * 4);
    st.out(a.table, table, (size_t)n_vertices * sizeof(cvs_segment));
    if ((rc = st.commit()) || (rc = st.upload(s))) return rc;
    // two launches for any table: the launch sequence is a function of n_vertices alone
    HIP_TRY(h, launch_segments_wave(a, s));
    HIP_TRY(h, launch_segments_block(a, s));
    return st.fetch(s);
}
