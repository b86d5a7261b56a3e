// explain_args.hpp — arguments of the explain and shortfall kernels (explain.hip, explain_plan.hip).
//
// HIP-free: the kernels take these by value, explain_stage.cpp fills them over the two staged buffers and
// tools/shortfall_check.cpp follows them on the host.  The launches are declared in explain_dev.hpp.
#pragma once

#include <cstdint>

#include "explain.hpp"
#include "explain_plan.hpp"

namespace sr {

constexpr int kExplainSums = 16;  // words per queried pod: counts[SR_WHY_COUNT], feasible, first, 2 spare
constexpr int kExplainFeasible = SR_WHY_COUNT, kExplainFirst = SR_WHY_COUNT + 1;

// Everything the kernel reads sits in one buffer the explain call uploads
// (the atom rows and node free values of ITS encode: the resident workload's
// node section may be stale after a K0-less tick and is not read).
struct ExplainArgs {
  int32_t n_spot, n_pad, Wp;
  int32_t n_pods;              // queried (active) pods
  int32_t pod0;                // first pod of this launch (blockIdx.y + pod0)
  const uint64_t* atoms;       // [n_atoms][Wp]
  const int64_t* node_free;    // [3][n_pad]
  const int32_t* xoff;         // [n_classes + 1]
  const int32_t* xops;
  const ExplainPod* pods;      // [n_pods]
  int32_t* sums;               // [n_pods][kExplainSums], zeroed on the stream before the launch; first as
                               //   n_pad - position (0: none), so the largest value is the first position
  uint16_t* node_mask;         // [n_pods][n_spot], nullptr: not wanted
};

// sr_explain_plan (explain_plan.hip): the same, a query being a candidate's
// stop pod with the plain context of its earlier pods, from the same buffer.
struct ExplainPlanArgs {
  ExplainArgs x;
  const int32_t* ctx_off;       // [n_pods + 1] CSR query -> entries
  const PlanCtxEntry* ctx;      // per query sorted by node, nodes < n_spot
  const int32_t* node_slack;    // [n_pad] allowed pods - pods, pads 0
};

// sr_shortfall_pods / sr_shortfall_plan: sibling kernels of the two above (k_shortfall in explain.hip,
// k_shortfall_plan in explain_plan.hip) that take these beside the explain arguments, so the explain kernels'
// own arguments, registers and LDS stay what they were.  A block leaves its minimum per dimension as a partial
// and k_shortfall_close takes the partials of a query in block order: no result depends on the order in which
// blocks or atomics ran.
constexpr int kShortSums = 8;  // words per queried pod: near, only_nodes[SR_SHORT_COUNT], 3 spare
constexpr uint64_t kShortNone = ~uint64_t(0);  // no only-d node (a shortfall is at most INT64_MAX)

struct ShortfallArgs {
  const int64_t* node_left;  // [n_pad] allowed pods - pods (explain_plan.hpp node_left), pads 0
  int32_t* sums;             // [n_pods][kShortSums], zeroed on the stream before the launch
  uint64_t* part_min;        // [n_pods][blocks][SR_SHORT_COUNT] a block's smallest only-d shortfall, kShortNone: none
  int32_t* part_at;          // [n_pods][blocks][SR_SHORT_COUNT] the lowest position attaining it
  int32_t blocks;            // gridDim.x of the launch
  int64_t* only_min;         // [n_pods][SR_SHORT_COUNT] written by k_shortfall_close
  int32_t* only_at;          // [n_pods][SR_SHORT_COUNT]
  int64_t* node_short;       // [n_pods][n_spot][SR_SHORT_COUNT], nullptr: not wanted
};

inline int32_t shortfall_blocks(int32_t Wp) { return (Wp + 3) / 4; }  // (kXWaves row words a block)

}  // namespace sr
