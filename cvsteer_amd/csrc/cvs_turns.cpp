// cvs_turns.cpp -- the C ABI of the contour turns (extension): cvs_chain_turns.  Argument checks, the check of a host chain table
// (chain_table_not_running_sum, cvs_chain_table.h), staging of host arrays in the handle's scratch (cvs_context::ch_scr) and the two or three launches
// of cvs_kernels_turns.hip.  Nothing is read back; no arithmetic on coordinates happens here.
#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "cvs_contour_host.h"
#include "cvs_turns.h"

using namespace cvs;

static_assert(sizeof(cvs_chain_turn) == kTurnWords * 4 && offsetof(cvs_chain_turn, flags) == 4 && offsetof(cvs_chain_turn, nb) == 8 &&
                  offsetof(cvs_chain_turn, sin) == 16 && offsetof(cvs_chain_turn, cos) == 20 && offsetof(cvs_chain_turn, lb) == 24,
              "cvs_chain_turn: the eight words tn_store writes");
static_assert(sizeof(cvs_turn_summary) == kTurnSummaryWords * 4 && offsetof(cvs_turn_summary, sharpest) == 8 &&
                  offsetof(cvs_turn_summary, min_cos) == 12,
              "cvs_turn_summary: the four words tn_store_summary writes");
static_assert(CVS_TURN_CORNER == kTurnCorner && CVS_TURN_END == kTurnEnd && CVS_TURN_DEGENERATE == kTurnDegenerate &&
                  CVS_TURN_SHORT == kTurnShort && CVS_TURN_NO_CHAIN == kTurnNoChain,
              "the flags the turn kernels write");
static_assert(sizeof(cvs_turn_cfg) == 16 && sizeof(cvs_chain) == 16, "the structs of the turn call");

int cvs_chain_turns(cvs_handle h, const int32_t* points, int n_points, const cvs_chain* chains, int n_chains, const float* xy,
                    const cvs_turn_cfg* cfg, cvs_chain_turn* table, cvs_turn_summary* summary, int mem)
{
    if (!h) return CVS_E_BADARG;
    if (!cfg) return fail(h, CVS_E_BADARG, "cfg missing");
    if (cfg->radius < 1 || cfg->radius > kTurnMaxRadius) return fail(h, CVS_E_BADARG, "radius is 1 .. 64");
    if (cfg->min_arm < 1 || cfg->min_arm > cfg->radius) return fail(h, CVS_E_BADARG, "min_arm is 1 .. radius");
    if (cfg->nms < 0 || cfg->nms > kTurnMaxNms) return fail(h, CVS_E_BADARG, "nms is 0 .. 64");
    if (!(cfg->max_cos >= -1.0f && cfg->max_cos <= 1.0f)) return fail(h, CVS_E_BADARG, "max_cos is -1 .. 1");   // (false for NaN)
    if (n_points < 0 || n_chains < 0) return fail(h, CVS_E_BADARG, "n_points and n_chains are >= 0");
    if ((n_points > 0 && (!points || !table)) || (n_chains > 0 && !chains)) return fail(h, CVS_E_BADARG, "points / chains / table missing");
    if (mem != CVS_MEM_HOST && mem != CVS_MEM_DEVICE) return fail(h, CVS_E_BADARG, "mem");
    if (misaligned(points) || misaligned(chains) || misaligned(xy) || misaligned(table) || misaligned(summary))
        return fail(h, CVS_E_BADARG, "an array is not aligned to 4 bytes");
    if (n_points > (1 << 30)) return fail(h, CVS_E_SIZE, "more than 2^30 points");
    if (n_points > 0 && n_chains == 0) return fail(h, CVS_E_BADARG, "points without a chain");
    const cvs_plane ins[3] = {array_plane(points, n_points, 2, mem), array_plane(chains, n_chains, 4, mem),
                              array_plane(xy, xy ? n_points : 0, 2, mem)};
    const cvs_plane outs[2] = {array_plane(table, n_points, kTurnWords, mem), array_plane(summary, summary ? n_chains : 0, kTurnSummaryWords, mem)};
    int rc;
    if ((rc = check_disjoint(h, ins, 3, outs, 2))) return rc;
    const bool host = mem == CVS_MEM_HOST;
    if (host)
        if (const char* what = chain_table_not_running_sum(n_points, reinterpret_cast<const int32_t*>(chains), n_chains)) return fail(h, CVS_E_BADARG, what);
    if (host && (rc = refuse_capture(h, "cvs_chain_turns stages host memory and synchronises: not capturable"))) return rc;
    if (n_points == 0) return CVS_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    h->used = true;

    hipStream_t s = h->stream;
    TurnArgs a{};
    a.n_points = n_points;
    a.n_chains = n_chains;
    a.radius = cfg->radius;
    a.min_arm = cfg->min_arm;
    a.nms = cfg->nms;
    a.max_cos = cfg->max_cos;
    Staged st(h, "cvs_chain_turns", host);
    st.in(a.points, points, (size_t)n_points * 8);
    st.in(a.chains, chains, (size_t)n_chains * sizeof(cvs_chain));
    st.in(a.xy, xy, (size_t)n_points * 8);
    st.out(a.table, table, (size_t)n_points * sizeof(cvs_chain_turn));
    st.out(a.summary, summary, (size_t)n_chains * sizeof(cvs_turn_summary));
    if ((rc = st.commit()) || (rc = st.upload(s))) return rc;
    // two launches for any table, three with a summary: the launch sequence is a function of (n_points, n_chains, summary != NULL) alone
    HIP_TRY(h, launch_turns(a, s));
    HIP_TRY(h, launch_turn_nms(a, s));
    if (a.summary) HIP_TRY(h, launch_turn_summary(a, s));
    return st.fetch(s);
}
