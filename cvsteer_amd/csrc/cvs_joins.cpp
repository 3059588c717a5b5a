// cvs_joins.cpp -- the C ABI of the contour joins (extension): cvs_chain_joins.  Argument checks, the check of a host chain table
// (chain_table_not_running_sum, cvs_chain_table.h), the scratch of the node grouping and the staging of host arrays in the handle's scratch
// (cvs_context::ch_scr) and the three launches of cvs_kernels_joins.hip.  Nothing is read back; no arithmetic on coordinates happens here.
#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "cvs_contour_host.h"
#include "cvs_joins.h"

using namespace cvs;

static_assert(sizeof(cvs_chain_join) == kJoinWords * 4 && offsetof(cvs_chain_join, degree) == 4 && offsetof(cvs_chain_join, next) == 8 &&
                  offsetof(cvs_chain_join, partner) == 12 && offsetof(cvs_chain_join, flags) == 16 && offsetof(cvs_chain_join, n) == 20 &&
                  offsetof(cvs_chain_join, cos) == 24 && offsetof(cvs_chain_join, sin) == 28,
              "cvs_chain_join: the eight words jn_store writes");
static_assert(CVS_JOIN_MUTUAL == kJoinMutual && CVS_JOIN_NONE == kJoinNone && CVS_JOIN_CROWDED == kJoinCrowded && CVS_JOIN_SHORT == kJoinShort &&
                  CVS_JOIN_DEGENERATE == kJoinDegenerate && CVS_JOIN_NO_CHAIN == kJoinNoChain,
              "the flags the join kernels write");
static_assert(sizeof(cvs_join_cfg) == 16 && sizeof(cvs_chain) == 16, "the structs of the join call");

int cvs_chain_joins(cvs_handle h, const int32_t* points, int n_points, const cvs_chain* chains, int n_chains, const float* xy,
                    const cvs_join_cfg* cfg, cvs_chain_join* table, int mem)
{
    if (!h) return CVS_E_BADARG;
    if (!cfg) return fail(h, CVS_E_BADARG, "cfg missing");
    if (cfg->radius < 1 || cfg->radius > kJoinMaxRadius) return fail(h, CVS_E_BADARG, "radius is 1 .. 64");
    if (cfg->min_arm < 1 || cfg->min_arm > cfg->radius) return fail(h, CVS_E_BADARG, "min_arm is 1 .. radius");
    if (!(cfg->min_cos >= -1.0f && cfg->min_cos <= 1.0f)) return fail(h, CVS_E_BADARG, "min_cos is -1 .. 1");   // (false for NaN)
    if (cfg->reserved != 0) return fail(h, CVS_E_BADARG, "cfg.reserved is 0");
    if (n_points < 0 || n_chains < 0) return fail(h, CVS_E_BADARG, "n_points and n_chains are >= 0");
    if ((n_points > 0 && !points) || (n_chains > 0 && (!chains || !table))) return fail(h, CVS_E_BADARG, "points / chains / table missing");
    if (mem != CVS_MEM_HOST && mem != CVS_MEM_DEVICE) return fail(h, CVS_E_BADARG, "mem");
    if (misaligned(points) || misaligned(chains) || misaligned(xy) || misaligned(table)) return fail(h, CVS_E_BADARG, "an array is not aligned to 4 bytes");
    if (n_points > (1 << 30)) return fail(h, CVS_E_SIZE, "more than 2^30 points");
    if (n_chains > kJoinMaxChains) return fail(h, CVS_E_SIZE, "more than 2^26 chains");
    if (n_points > 0 && n_chains == 0) return fail(h, CVS_E_BADARG, "points without a chain");
    const cvs_plane ins[3] = {array_plane(points, n_points, 2, mem), array_plane(chains, n_chains, 4, mem), array_plane(xy, xy ? n_points : 0, 2, mem)};
    const cvs_plane out = array_plane(table, 2ll * n_chains, kJoinWords, mem);
    int rc;
    if ((rc = check_disjoint(h, ins, 3, &out, 1))) return rc;
    const bool host = mem == CVS_MEM_HOST;
    if (host)
        if (const char* what = chain_table_not_running_sum(n_points, reinterpret_cast<const int32_t*>(chains), n_chains)) return fail(h, CVS_E_BADARG, what);
    if (host && (rc = refuse_capture(h, "cvs_chain_joins stages host memory and synchronises: not capturable"))) return rc;
    if (n_chains == 0) return CVS_OK;

    // the scratch: the node grouping first (a function of n_chains alone), then what a host call stages (no points: a null list)
    hipStream_t s = h->stream;
    JoinArgs a{};
    a.n_points = n_points;
    a.n_chains = n_chains;
    a.radius = cfg->radius;
    a.min_arm = cfg->min_arm;
    a.min_cos = cfg->min_cos;
    Staged st(h, "cvs_chain_joins", host);
    st.scratch(a.scratch, join_scratch_bytes(n_chains));
    st.in(a.points, host && !n_points ? nullptr : points, (size_t)n_points * 8);
    st.in(a.chains, chains, (size_t)n_chains * sizeof(cvs_chain));
    st.in(a.xy, xy, (size_t)n_points * 8);
    st.out(a.table, table, 2 * (size_t)n_chains * sizeof(cvs_chain_join));
    HIP_TRY(h, hipSetDevice(h->device));   // (this call allocates, DEVICE arrays or not)
    if ((rc = st.commit())) return rc;
    h->used = true;
    if ((rc = st.upload(s))) return rc;

    // three launches for any table: the launch sequence is a function of n_chains alone
    HIP_TRY(h, launch_join_arms(a, s));
    HIP_TRY(h, launch_join_insert(a, s));
    HIP_TRY(h, launch_join_resolve(a, s));
    return st.fetch(s);
}
