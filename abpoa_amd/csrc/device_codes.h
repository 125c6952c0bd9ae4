// Codes that device and host code share, defined once: the status a DP kernel leaves in AlnOut.status and the reason a read-set left a pass of the
// device-resident driver (PoaState.reason).  No HIP include: the host-side decisions (msa_passes.cpp) and their CPU tests read them too.
#pragma once

#define ABPOA_HIP_STATUS_OVERFLOW 1   // arena too small: host retries with a full-width arena
#define ABPOA_HIP_STATUS_NEED_SCORES 2   // direction-plane arenas (dir_plane.h): the backtrack met the one case the plane cannot decide -> redo with score records

namespace abpoa_hip {

// PoaState.reason of a set whose status is POA_ST_FALLBACK (msa_device.h host_reason_of maps them to the reasons the host reports)
constexpr int POA_WHY_NONE = 0;
constexpr int POA_WHY_NODES_AT_INIT = 1;      // the first read alone has more nodes than the set has node slots
constexpr int POA_WHY_PRED_SLOTS = 2;         // prepare: predecessor-list slots
constexpr int POA_WHY_CIGAR_SLOTS = 3;        // prepare: cigar slots
constexpr int POA_WHY_NODES_IN_FUSE = 4;      // fuse: node slots
constexpr int POA_WHY_EDGE_SLOTS = 5;         // an edge / aligned list of a node is full: more node slots would not help, the last pass does
constexpr int POA_WHY_GROWTH = 6;             // prepare: the projected node growth does not fit this pass (early exit)
constexpr int POA_WHY_ORDER_WALK = 7;         // the row-order walk did not finish
constexpr int POA_WHY_RANK_WALK = 8;          // the MSA rank walk did not finish
constexpr int POA_WHY_DP_STATUS = 1000;       // + the DP kernel's status (ABPOA_HIP_STATUS_*)

}  // namespace abpoa_hip
