// cvs_bridges.h -- launch descriptor of the contour-bridge kernels (cvs_kernels_bridges.hip), shared with their C-ABI layer
// (cvs_bridges.cpp).  The chain table and its flags are those of cvs_chains.h, the arm and the size of the hash table (join_slots) those of
// the joins (cvs_joins.h, cvs_chain_table.h); the scan over the partial sums goes through launch_scan_partials of cvs_components.h.
#pragma once
#include "cvs_chain_table.h"
#include "cvs_chains.h"
#include "cvs_components.h"
#include "cvs_joins.h"

namespace cvs {
// ---- contour bridges (cvs_chain_bridges, extension) ----
// One record per chain END: kBridgeWords 4-byte words (struct cvs_chain_bridge; cvs_bridges.cpp asserts the layout): partner, flags, n,
// steps, bridge, start, then the floats cos, cos_partner.  Record 2c is the head of chain c, 2c + 1 its tail.
constexpr int kBridgeWords = 8;
constexpr int kBridgeMutual = 1, kBridgeNone = 2, kBridgeJunction = 4, kBridgeShort = 8, kBridgeDegenerate = 16, kBridgeNoChain = 32,
              kBridgeCrowded = 64;   // CVS_BRIDGE_*
constexpr int kBridgeNotInCell = kBridgeNone | kBridgeJunction | kBridgeShort | kBridgeDegenerate | kBridgeNoChain;   // never counted into a cell
constexpr int kBridgeNotCandidate = kBridgeNotInCell | kBridgeCrowded;
constexpr int kBridgeMaxGap = 32, kBridgeMaxCell = 32;
constexpr int kBridgeMaxChains = kJoinMaxChains;

// Scratch of one call: kBridgeEndBytes per END (its arm, key, cell, the nine slots around it, its partner and what the scan leaves) and one
// int per CHAIN (the smaller end of bridge k: there are never more bridges than chains) -- kBridgeChainBytes per chain --, then the hash
// table of the cells (join_slots(n_chains) slots of kBridgeSlotBytes: at most half of them are ever claimed), the two arrays of partial
// sums (one int per kBridgeScanBlock ends and one for the total) and the block of the two written totals.
constexpr size_t kBridgeEndBytes = 120, kBridgeSlotBytes = 16;
constexpr size_t kBridgeChainBytes = 2 * kBridgeEndBytes + 4;
constexpr int kBridgeScanBlock = 1024;   // ends per workgroup of the scan: 256 lanes x 4
constexpr int bridge_scan_blocks(int n_chains) { return (int)((2ll * n_chains + kBridgeScanBlock - 1) / kBridgeScanBlock); }
constexpr size_t bridge_round(size_t bytes) { return (bytes + 255) / 256 * 256; }
constexpr size_t bridge_partials_bytes(int n_chains) { return bridge_round(((size_t)bridge_scan_blocks(n_chains) + 1) * 4); }
constexpr size_t bridge_ends_bytes(int n_chains) { return bridge_round(2 * (size_t)n_chains * kBridgeEndBytes); }
constexpr size_t bridge_los_bytes(int n_chains) { return bridge_round((size_t)n_chains * 4); }
constexpr size_t bridge_scratch_bytes(int n_chains)
{
    return bridge_ends_bytes(n_chains) + bridge_los_bytes(n_chains) + join_slots(n_chains) * kBridgeSlotBytes + 2 * bridge_partials_bytes(n_chains) + 256;
}
// launches of one call: arms, insert, crowd, best, resolve (with the partial sums), two scans of partial sums, records; emit with outputs
constexpr int kBridgeLaunchesTable = 8, kBridgeLaunchesEmit = 9;

struct BridgeArgs {
    const int32_t* points;   // n_points (x, y) pairs
    int n_points;
    const int32_t* chains;   // n_chains entries (start, length, flags, plane)
    int n_chains;
    const float* xy;         // nullptr: the integer points
    int radius, min_arm, max_gap;
    float min_cos;
    uint32_t* table;         // 2 * n_chains records
    int32_t* out_points;     // nullptr (table and counts only), or cap_points pairs
    int cap_points;
    int32_t* out_chains;     // nullptr iff out_points is, or cap_chains entries
    int cap_chains;
    float* out_xy;           // non-null iff xy and out_points are
    int32_t* counts;         // 3: n_bridges, n_out_chains, n_out_points
    unsigned char* scratch;  // bridge_scratch_bytes(n_chains), aligned to 16 bytes
};
// where the two written totals (chain entries, points: what a HOST call copies out) lie in the scratch
constexpr size_t bridge_written_offset(int n_chains) { return bridge_scratch_bytes(n_chains) - 256; }
// the whole sequence on s: nothing is read back
hipError_t launch_bridges(const BridgeArgs& a, hipStream_t s);

}  // namespace cvs
