// cvs_paths.h -- launch descriptor of the contour-path kernels (cvs_kernels_paths.hip), shared with their C-ABI layer (cvs_paths.cpp).
// The chain table and kChainClosed are those of cvs_chains.h, the join record (kJoinWords, kJoinMutual) that of cvs_joins.h; the scan over
// the partial sums goes through launch_scan_partials of cvs_components.h.
#pragma once
#include "cvs_chains.h"
#include "cvs_components.h"
#include "cvs_joins.h"

namespace cvs {
// ---- contour paths (cvs_chain_paths, extension) ----
constexpr int kMemberReversed = 1;   // CVS_MEMBER_REVERSED
constexpr int kPathMaxChains = kJoinMaxChains;

// Scratch of one call: kPathEndBytes per END -- its links (16), the two buffers of the walk's last end and smallest end (2 x 8), the two
// buffers of the ranking (2 x 16), what the scan leaves at the first end of a path (16) -- then the three arrays of partial sums, one int
// per kPathScanBlock ends and one for the total.
constexpr size_t kPathEndBytes = 80;
constexpr int kPathScanBlock = 1024;   // ends per workgroup of the scan: 256 lanes x 4
constexpr int path_scan_blocks(int n_chains) { return (int)((2ll * n_chains + kPathScanBlock - 1) / kPathScanBlock); }
constexpr size_t path_partials_bytes(int n_chains) { return (((size_t)path_scan_blocks(n_chains) + 1) * 4 + 255) / 256 * 256; }
constexpr size_t path_scratch_bytes(int n_chains) { return 2 * (size_t)n_chains * kPathEndBytes + 3 * path_partials_bytes(n_chains); }
// rounds of pointer jumping: the smallest r with 2^r >= n_chains.  A walk holds a chain once (its twin holds the other direction), so no
// walk and no cycle has more than n_chains entry ends, and 2^r steps reach round every one of them.
constexpr int path_rounds(int n_chains)
{
    int r = 0;
    while ((1ll << r) < n_chains) ++r;
    return r;
}
// launches of one call: links, r rounds for the last and the smallest end, the cut, r rounds of ranking, count, three scans of partial
// sums, apply, emit
constexpr int path_launches(int n_chains) { return 2 * path_rounds(n_chains) + 8; }

struct PathArgs {
    const int32_t* points;   // n_points (x, y) pairs
    int n_points;
    const int32_t* chains;   // n_chains entries (start, length, flags, plane)
    int n_chains;
    const int32_t* joins;    // 2 * n_chains records of kJoinWords words
    const float* xy;         // nullptr, or n_points pairs
    int32_t* path_points;    // n_points pairs
    int32_t* paths;          // n_chains entries
    int32_t* info;           // n_chains records of 4 words
    int32_t* members;        // n_chains records of 4 words
    int32_t* index;          // nullptr, or n_points
    float* path_xy;          // nullptr iff xy is
    int32_t* counts;         // 2
    unsigned char* scratch;  // path_scratch_bytes(n_chains), aligned to 16 bytes
};
// the whole sequence, path_launches(n_chains) launches on s: nothing is read back
hipError_t launch_paths(const PathArgs& a, hipStream_t s);

}  // namespace cvs
