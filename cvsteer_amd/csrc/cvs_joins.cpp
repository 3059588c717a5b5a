// cvs_joins.cpp -- the C ABI of the contour joins (extension): cvs_chain_joins.  Argument checks, the check of a host chain table
// (joins_host_table_wrong, cvs_joins.h), the scratch of the node grouping and the staging of host arrays in the handle's scratch
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

namespace {

bool misaligned(const void* p) { return reinterpret_cast<uintptr_t>(p) % alignof(int32_t) != 0; }

// an array of `n` records of `words` 4-byte words as a plane, for the overlap rule of the contour tail (check_disjoint)
cvs_plane array_plane(const void* p, long long n, int words, int mem)
{
    cvs_plane q{};
    q.data = n > 0 ? const_cast<float*>(static_cast<const float*>(p)) : nullptr;
    q.rows = (int)n;
    q.cols = words;
    q.step = (size_t)words * 4;
    q.mem = mem;
    return q;
}

}  // namespace

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
        if (const char* what = joins_host_table_wrong(n_points, reinterpret_cast<const int32_t*>(chains), n_chains)) return fail(h, CVS_E_BADARG, what);
    if (host && (rc = refuse_capture(h, "cvs_chain_joins stages host memory and synchronises: not capturable"))) return rc;
    if (n_chains == 0) return CVS_OK;

    // the scratch: the node grouping first (a function of n_chains alone), then what a host call stages
    const size_t b_out = 2 * (size_t)n_chains * sizeof(cvs_chain_join), b_pts = (size_t)n_points * 8, b_tab = (size_t)n_chains * sizeof(cvs_chain);
    const size_t b_xy = xy ? b_pts : 0;
    Scratch sc;
    const size_t o_join = sc.reserve(join_scratch_bytes(n_chains));
    size_t o_out = 0, o_pts = 0, o_chn = 0, o_xy = 0;
    if (host) o_out = sc.reserve(b_out), o_pts = sc.reserve(b_pts), o_chn = sc.reserve(b_tab), o_xy = sc.reserve(b_xy);
    if (sc.need > h->ch_scr_bytes) {
        bool cap = false;
        if ((rc = capturing(h, cap))) return rc;
        if (cap) return fail(h, CVS_E_UNSUPPORTED, "cvs_chain_joins would have to grow the handle's scratch during capture: call once eagerly first");
    }
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = grow_scratch(h, "hipMalloc(&h->ch_scr, need)", h->ch_scr, h->ch_scr_bytes, sc.need, 1))) return rc;
    h->used = true;

    hipStream_t s = h->stream;
    JoinArgs a{};
    a.points = points;
    a.n_points = n_points;
    a.chains = reinterpret_cast<const int32_t*>(chains);
    a.n_chains = n_chains;
    a.xy = xy;
    a.radius = cfg->radius;
    a.min_arm = cfg->min_arm;
    a.min_cos = cfg->min_cos;
    a.table = reinterpret_cast<uint32_t*>(table);
    a.scratch = h->ch_scr + o_join;
    if (host) {
        const struct {
            const void* src;
            size_t off, bytes;
        } up[3] = {{points, o_pts, b_pts}, {chains, o_chn, b_tab}, {xy, o_xy, b_xy}};
        for (const auto& u : up)
            if (u.bytes) HIP_TRY(h, hipMemcpyAsync(h->ch_scr + u.off, u.src, u.bytes, hipMemcpyHostToDevice, s));
        a.points = n_points ? reinterpret_cast<const int32_t*>(h->ch_scr + o_pts) : nullptr;
        a.chains = reinterpret_cast<const int32_t*>(h->ch_scr + o_chn);
        a.xy = xy ? reinterpret_cast<const float*>(h->ch_scr + o_xy) : nullptr;
        a.table = reinterpret_cast<uint32_t*>(h->ch_scr + o_out);
    }
    // three launches for any table: the launch sequence is a function of n_chains alone
    HIP_TRY(h, launch_join_arms(a, s));
    HIP_TRY(h, launch_join_insert(a, s));
    HIP_TRY(h, launch_join_resolve(a, s));
    if (host) {
        HIP_TRY(h, hipMemcpyAsync(table, a.table, b_out, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
    }
    return CVS_OK;
}
