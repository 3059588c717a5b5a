// cvs_paths.cpp -- the C ABI of the contour paths (extension): cvs_chain_paths.  Argument checks, the check of a host chain table
// (chain_table_not_running_sum, cvs_chain_table.h), the scratch of the ranking and the staging of host arrays in the handle's scratch
// (cvs_context::ch_scr) and the launch sequence of cvs_kernels_paths.hip.  A DEVICE call reads nothing back; a HOST call reads the two
// counts and then copies out the records and points they count, no more.
#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "cvs_contour_host.h"
#include "cvs_paths.h"

using namespace cvs;

static_assert(sizeof(cvs_path_member) == 16 && offsetof(cvs_path_member, flags) == 4 && offsetof(cvs_path_member, path) == 8 &&
                  offsetof(cvs_path_member, start) == 12,
              "cvs_path_member: the four words k_path_emit writes");
static_assert(sizeof(cvs_path_info) == 16 && offsetof(cvs_path_info, n_members) == 4 && offsetof(cvs_path_info, first_end) == 8 &&
                  offsetof(cvs_path_info, last_end) == 12,
              "cvs_path_info: the four words k_path_apply writes");
static_assert(CVS_MEMBER_REVERSED == kMemberReversed && sizeof(cvs_chain) == 16 && sizeof(cvs_chain_join) == kJoinWords * 4 &&
                  offsetof(cvs_chain_join, partner) == 12 && offsetof(cvs_chain_join, flags) == 16,
              "the words the path kernels read and write");
static_assert(CVS_PATH_SCRATCH_PER_END == kPathEndBytes, "the scratch per end the header names");

int cvs_chain_paths(cvs_handle h, const int32_t* points, int n_points, const cvs_chain* chains, int n_chains, const cvs_chain_join* joins,
                    const float* xy, int32_t* path_points, cvs_chain* paths, cvs_path_info* info, cvs_path_member* members, int32_t* index,
                    float* path_xy, int32_t* counts, int mem)
{
    if (!h) return CVS_E_BADARG;
    if (n_points < 0 || n_chains < 0) return fail(h, CVS_E_BADARG, "n_points and n_chains are >= 0");
    if (!counts) return fail(h, CVS_E_BADARG, "counts missing");
    if ((n_points > 0 && (!points || !path_points)) || (n_chains > 0 && (!chains || !joins || !paths || !info || !members)))
        return fail(h, CVS_E_BADARG, "points / chains / joins / path_points / paths / info / members missing");
    if ((xy != nullptr) != (path_xy != nullptr)) return fail(h, CVS_E_BADARG, "xy and path_xy: both or neither");
    if (mem != CVS_MEM_HOST && mem != CVS_MEM_DEVICE) return fail(h, CVS_E_BADARG, "mem");
    if (misaligned(points) || misaligned(chains) || misaligned(joins) || misaligned(xy) || misaligned(path_points) || misaligned(paths) ||
        misaligned(info) || misaligned(members) || misaligned(index) || misaligned(path_xy) || misaligned(counts))
        return fail(h, CVS_E_BADARG, "an array is not aligned to 4 bytes");
    if (n_points > (1 << 30)) return fail(h, CVS_E_SIZE, "more than 2^30 points");
    if (n_chains > kPathMaxChains) return fail(h, CVS_E_SIZE, "more than 2^26 chains");
    if (n_points > 0 && n_chains == 0) return fail(h, CVS_E_BADARG, "points without a chain");
    const cvs_plane ins[4] = {array_plane(points, n_points, 2, mem), array_plane(chains, n_chains, 4, mem),
                              array_plane(joins, 2ll * n_chains, kJoinWords, mem), array_plane(xy, xy ? n_points : 0, 2, mem)};
    const cvs_plane outs[7] = {array_plane(path_points, n_points, 2, mem), array_plane(paths, n_chains, 4, mem),
                               array_plane(info, n_chains, 4, mem),        array_plane(members, n_chains, 4, mem),
                               array_plane(index, index ? n_points : 0, 1, mem), array_plane(path_xy, path_xy ? n_points : 0, 2, mem),
                               array_plane(counts, 1, 2, mem)};
    int rc;
    if ((rc = check_disjoint(h, ins, 4, outs, 7))) return rc;
    const bool host = mem == CVS_MEM_HOST;
    if (host)
        if (const char* what = chain_table_not_running_sum(n_points, reinterpret_cast<const int32_t*>(chains), n_chains)) return fail(h, CVS_E_BADARG, what);
    if (host && (rc = refuse_capture(h, "cvs_chain_paths stages host memory and synchronises: not capturable"))) return rc;
    hipStream_t s = h->stream;
    if (n_chains == 0) {
        if (host) {
            counts[0] = counts[1] = 0;
            return CVS_OK;
        }
        HIP_TRY(h, hipSetDevice(h->device));
        h->used = true;
        HIP_TRY(h, hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), s));
        return CVS_OK;
    }

    // the scratch: the ranking first (a function of n_chains alone), then what a host call stages (no points: a null list)
    PathArgs a{};
    a.n_points = n_points;
    a.n_chains = n_chains;
    Staged st(h, "cvs_chain_paths", host);
    st.scratch(a.scratch, path_scratch_bytes(n_chains));
    st.in(a.points, host && !n_points ? nullptr : points, (size_t)n_points * 8);
    st.in(a.chains, chains, (size_t)n_chains * sizeof(cvs_chain));
    st.in(a.joins, joins, 2 * (size_t)n_chains * sizeof(cvs_chain_join));
    st.in(a.xy, xy, (size_t)n_points * 8);
    st.out(a.path_points, host && !n_points ? nullptr : path_points, (size_t)n_points * 8);
    st.out(a.paths, paths, (size_t)n_chains * sizeof(cvs_chain));
    st.out(a.info, info, (size_t)n_chains * sizeof(cvs_path_info));
    st.out(a.members, members, (size_t)n_chains * sizeof(cvs_path_member));
    st.out(a.index, index, (size_t)n_points * 4);
    st.out(a.path_xy, path_xy, (size_t)n_points * 8);
    st.out(a.counts, counts, 2 * sizeof(int32_t));
    HIP_TRY(h, hipSetDevice(h->device));   // (this call allocates, DEVICE arrays or not)
    if ((rc = st.commit())) return rc;
    h->used = true;
    if ((rc = st.upload(s))) return rc;

    // 2 ceil(log2 n_chains) + 8 launches for any table: the launch sequence is a function of n_chains alone
    HIP_TRY(h, launch_paths(a, s));
    if (!host) return CVS_OK;

    // HOST: the counts first, then what they count -- records and points past the counts are not written
    int32_t got[2] = {0, 0};
    HIP_TRY(h, hipMemcpyAsync(got, a.counts, sizeof(got), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    const size_t np = (size_t)got[0], npp = (size_t)got[1];
    if (got[0] < 0 || got[0] > n_chains || got[1] < 0 || got[1] > n_points) return fail(h, CVS_E_HIP, "cvs_chain_paths: counts outside the table");
    const size_t nm = (size_t)n_chains;   // (a checked HOST table: every entry is valid, and every valid entry is one member)
    if (npp) HIP_TRY(h, hipMemcpyAsync(path_points, a.path_points, npp * 8, hipMemcpyDeviceToHost, s));
    if (np) HIP_TRY(h, hipMemcpyAsync(paths, a.paths, np * sizeof(cvs_chain), hipMemcpyDeviceToHost, s));
    if (np) HIP_TRY(h, hipMemcpyAsync(info, a.info, np * sizeof(cvs_path_info), hipMemcpyDeviceToHost, s));
    if (nm) HIP_TRY(h, hipMemcpyAsync(members, a.members, nm * sizeof(cvs_path_member), hipMemcpyDeviceToHost, s));
    if (npp && index) HIP_TRY(h, hipMemcpyAsync(index, a.index, npp * 4, hipMemcpyDeviceToHost, s));
    if (npp && path_xy) HIP_TRY(h, hipMemcpyAsync(path_xy, a.path_xy, npp * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    counts[0] = got[0];
    counts[1] = got[1];
    return CVS_OK;
}
