// cvs_bridges.cpp -- the C ABI of the contour bridges (extension): cvs_chain_bridges.  Argument checks, the check of a host chain table
// (chain_table_not_running_sum, cvs_chain_table.h), the scratch of the cell grouping and the staging of host arrays in the handle's scratch
// (cvs_context::ch_scr) and the launch sequence of cvs_kernels_bridges.hip.  A DEVICE call reads nothing back; a HOST call reads the counts
// and the two written totals and then copies out the records, entries and points that were written, no more.  No arithmetic on
// coordinates happens here.
#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "cvs_bridges.h"
#include "cvs_contour_host.h"

using namespace cvs;

static_assert(sizeof(cvs_chain_bridge) == kBridgeWords * 4 && offsetof(cvs_chain_bridge, flags) == 4 && offsetof(cvs_chain_bridge, n) == 8 &&
                  offsetof(cvs_chain_bridge, steps) == 12 && offsetof(cvs_chain_bridge, bridge) == 16 && offsetof(cvs_chain_bridge, start) == 20 &&
                  offsetof(cvs_chain_bridge, cos) == 24 && offsetof(cvs_chain_bridge, cos_partner) == 28,
              "cvs_chain_bridge: the eight words k_bridge_records writes");
static_assert(CVS_BRIDGE_MUTUAL == kBridgeMutual && CVS_BRIDGE_NONE == kBridgeNone && CVS_BRIDGE_JUNCTION == kBridgeJunction &&
                  CVS_BRIDGE_SHORT == kBridgeShort && CVS_BRIDGE_DEGENERATE == kBridgeDegenerate && CVS_BRIDGE_NO_CHAIN == kBridgeNoChain &&
                  CVS_BRIDGE_CROWDED == kBridgeCrowded,
              "the flags the bridge kernels write");
static_assert(sizeof(cvs_bridge_cfg) == 16 && sizeof(cvs_chain) == 16, "the structs of the bridge call");
static_assert(CVS_BRIDGE_SCRATCH_PER_CHAIN == kBridgeChainBytes && CVS_BRIDGE_MAX_GAP == kBridgeMaxGap && CVS_BRIDGE_MAX_CELL == kBridgeMaxCell,
              "the constants the header names");

int cvs_chain_bridges(cvs_handle h, const int32_t* points, int n_points, const cvs_chain* chains, int n_chains, const float* xy,
                      const cvs_bridge_cfg* cfg, cvs_chain_bridge* table, int32_t* out_points, int cap_points, cvs_chain* out_chains, int cap_chains,
                      float* out_xy, int32_t* counts, int mem)
{
    if (!h) return CVS_E_BADARG;
    if (!cfg) return fail(h, CVS_E_BADARG, "cfg missing");
    if (cfg->radius < 1 || cfg->radius > kJoinMaxRadius) return fail(h, CVS_E_BADARG, "radius is 1 .. 64");
    if (cfg->min_arm < 1 || cfg->min_arm > cfg->radius) return fail(h, CVS_E_BADARG, "min_arm is 1 .. radius");
    if (cfg->max_gap < 2 || cfg->max_gap > kBridgeMaxGap) return fail(h, CVS_E_BADARG, "max_gap is 2 .. 32");
    if (!(cfg->min_cos >= -1.0f && cfg->min_cos <= 1.0f)) return fail(h, CVS_E_BADARG, "min_cos is -1 .. 1");   // (false for NaN)
    if (n_points < 0 || n_chains < 0) return fail(h, CVS_E_BADARG, "n_points and n_chains are >= 0");
    if (!counts) return fail(h, CVS_E_BADARG, "counts missing");
    if ((n_points > 0 && !points) || (n_chains > 0 && (!chains || !table))) return fail(h, CVS_E_BADARG, "points / chains / table missing");
    const bool emit = out_points || out_chains;
    if (emit && (!out_points || !out_chains)) return fail(h, CVS_E_BADARG, "out_points and out_chains: both or neither");
    if (!emit && (cap_points != 0 || cap_chains != 0)) return fail(h, CVS_E_BADARG, "a capacity without its array");
    if (emit && (cap_points < n_points || cap_chains < n_chains)) return fail(h, CVS_E_BADARG, "the capacities hold the inputs at least");
    if ((out_xy != nullptr) != (emit && xy != nullptr)) return fail(h, CVS_E_BADARG, "out_xy: with xy and out_points, and only then");
    if (mem != CVS_MEM_HOST && mem != CVS_MEM_DEVICE) return fail(h, CVS_E_BADARG, "mem");
    if (misaligned(points) || misaligned(chains) || misaligned(xy) || misaligned(table) || misaligned(out_points) || misaligned(out_chains) ||
        misaligned(out_xy) || misaligned(counts))
        return fail(h, CVS_E_BADARG, "an array is not aligned to 4 bytes");
    if (n_points > (1 << 30)) return fail(h, CVS_E_SIZE, "more than 2^30 points");
    if (n_chains > kBridgeMaxChains) return fail(h, CVS_E_SIZE, "more than 2^26 chains");
    if (n_points > 0 && n_chains == 0) return fail(h, CVS_E_BADARG, "points without a chain");
    const cvs_plane ins[3] = {array_plane(points, n_points, 2, mem), array_plane(chains, n_chains, 4, mem), array_plane(xy, xy ? n_points : 0, 2, mem)};
    const cvs_plane outs[5] = {array_plane(table, 2ll * n_chains, kBridgeWords, mem), array_plane(out_points, emit ? cap_points : 0, 2, mem),
                               array_plane(out_chains, emit ? cap_chains : 0, 4, mem), array_plane(out_xy, out_xy ? cap_points : 0, 2, mem),
                               array_plane(counts, 1, 3, mem)};
    int rc;
    if ((rc = check_disjoint(h, ins, 3, outs, 5))) return rc;
    const bool host = mem == CVS_MEM_HOST;
    if (host)
        if (const char* what = chain_table_not_running_sum(n_points, reinterpret_cast<const int32_t*>(chains), n_chains)) return fail(h, CVS_E_BADARG, what);
    if (host && (rc = refuse_capture(h, "cvs_chain_bridges stages host memory and synchronises: not capturable"))) return rc;
    hipStream_t s = h->stream;
    if (n_chains == 0) {
        if (host) {
            counts[0] = counts[1] = counts[2] = 0;
            return CVS_OK;
        }
        HIP_TRY(h, hipSetDevice(h->device));
        h->used = true;
        HIP_TRY(h, hipMemsetAsync(counts, 0, 3 * sizeof(int32_t), s));
        return CVS_OK;
    }

    // the scratch: the grouping first (a function of n_chains alone), then what a host call stages (no points: a null list)
    BridgeArgs a{};
    a.n_points = n_points;
    a.n_chains = n_chains;
    a.radius = cfg->radius;
    a.min_arm = cfg->min_arm;
    a.max_gap = cfg->max_gap;
    a.min_cos = cfg->min_cos;
    a.cap_points = cap_points;
    a.cap_chains = cap_chains;
    Staged st(h, "cvs_chain_bridges", host);
    st.scratch(a.scratch, bridge_scratch_bytes(n_chains));
    st.in(a.points, host && !n_points ? nullptr : points, (size_t)n_points * 8);
    st.in(a.chains, chains, (size_t)n_chains * sizeof(cvs_chain));
    st.in(a.xy, xy, (size_t)n_points * 8);
    st.out(a.table, table, 2 * (size_t)n_chains * sizeof(cvs_chain_bridge));
    st.out(a.out_points, out_points, (size_t)cap_points * 8);
    st.out(a.out_chains, out_chains, (size_t)cap_chains * sizeof(cvs_chain));
    st.out(a.out_xy, out_xy, (size_t)cap_points * 8);
    st.out(a.counts, counts, 3 * sizeof(int32_t));
    HIP_TRY(h, hipSetDevice(h->device));   // (this call allocates, DEVICE arrays or not)
    if ((rc = st.commit())) return rc;
    h->used = true;
    if ((rc = st.upload(s))) return rc;

    // 8 launches for any table, 9 with outputs: the launch sequence is a function of n_chains alone
    HIP_TRY(h, launch_bridges(a, s));
    if (!host) return CVS_OK;

    // HOST: the counts and the written totals first, then what they count -- entries and points past them are not written
    int32_t got[3] = {0, 0, 0}, written[2] = {0, 0};
    HIP_TRY(h, hipMemcpyAsync(got, a.counts, sizeof(got), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(written, a.scratch + bridge_written_offset(n_chains), sizeof(written), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    if (written[0] < n_chains || written[1] < n_points || (emit && (written[0] > cap_chains || written[1] > cap_points)))
        return fail(h, CVS_E_HIP, "cvs_chain_bridges: totals outside the arrays");
    const size_t wc = (size_t)written[0], wp = (size_t)written[1];
    HIP_TRY(h, hipMemcpyAsync(table, a.table, 2 * (size_t)n_chains * sizeof(cvs_chain_bridge), hipMemcpyDeviceToHost, s));
    if (emit && wp) HIP_TRY(h, hipMemcpyAsync(out_points, a.out_points, wp * 8, hipMemcpyDeviceToHost, s));
    if (emit) HIP_TRY(h, hipMemcpyAsync(out_chains, a.out_chains, wc * sizeof(cvs_chain), hipMemcpyDeviceToHost, s));
    if (out_xy && wp) HIP_TRY(h, hipMemcpyAsync(out_xy, a.out_xy, wp * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    counts[0] = got[0], counts[1] = got[1], counts[2] = got[2];
    return CVS_OK;
}
