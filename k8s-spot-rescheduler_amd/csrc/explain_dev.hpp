// explain_dev.hpp — arguments of the explain kernel (explain.hip), shared with planner.cpp.
#pragma once

#include <hip/hip_runtime.h>

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

hipError_t launch_explain(const ExplainArgs& a, hipStream_t s);

// sr_explain_plan (explain_plan.hip): the same, a query being a candidate's
// stop pod with the plain context of its earlier pods, from the same buffer.
struct ExplainPlanArgs {
  ExplainArgs x;
  const int32_t* ctx_off;       // [n_pods + 1] CSR query -> entries
  const PlanCtxEntry* ctx;      // per query sorted by node, nodes < n_spot
  const int32_t* node_slack;    // [n_pad] allowed pods - pods, pads 0
};

hipError_t launch_explain_plan(const ExplainPlanArgs& a, hipStream_t s);

}  // namespace sr
