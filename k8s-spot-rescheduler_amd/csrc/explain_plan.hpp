// explain_plan.hpp — the stop pods of a tick's candidates in the context of their own earlier pods
// (sr_explain_plan), host side.
//
// HIP-free.  Candidate c stopped at pod k because pods 0..k-1 of its node were
// placed first (rescheduler.go:366).  What those pods change for pod k on a
// node is what AddPod changes there.  The context of (c, k) is PLAIN when that
// is nothing but arithmetic on the touched nodes: the pod count and the three
// requested values.  plan_queries decides it from the sr_cluster tables alone
// (the rule is syntactic and conservative) and writes a plain
// context as a list sorted by node; explain_node_ctx is explain_node with such
// a list applied, the statement the kernel of explain_plan.hip follows.
#pragma once

#include <cstdint>
#include <vector>

#include "explain.hpp"

struct sr_snapshot;

namespace sr {

// One touched node of a plain context: the earlier pods placed there and the
// sum of what AddPod adds to Requested for them (acc_*, req_* without those
// tables): the accounting, not the fit request.
struct PlanCtxEntry {
  int32_t node;
  int32_t pods;
  int64_t acc[3];
};
static_assert(sizeof(PlanCtxEntry) == 32, "read by the kernel as it stands");

// What of a pod can meet the same thing of another pod on one node.
struct PodTraits {
  bool ports;    // a host port or an inline disk
  bool scalars;  // a scalar name or an attachable volume
  bool anti;     // required anti-affinity (terms or the flag)
  bool terms;    // ... or required affinity terms
  bool spread;   // a DoNotSchedule spread constraint
};
PodTraits pod_traits(const sr_cluster* c, int32_t pod);

constexpr int64_t kQuantityEnd = int64_t(1) << 62;  // the encoder takes node quantities in [0, 2^62)

struct PlanQueries {
  std::vector<uint8_t> how;           // [n_cand] SR_EXPLAIN_NONE / BATCHED / SINGLE
  std::vector<int32_t> batched;       // the candidates going the batched way, ascending
  std::vector<int32_t> pods;          // ... their stop pods (cluster pod indices)
  std::vector<int32_t> off;           // [batched + 1] into entries
  std::vector<PlanCtxEntry> entries;  // per query sorted by node, one entry per distinct node
};

// Checks at_pod / node_of_pod against the candidates (SR_ERR_INVALID_ARG:
// at_pod[c] >= pods of c, a pod index out of range, a position below at_pod[c]
// that is -1 or >= n_spot) and sorts every asked candidate into its way.
// Nothing is modified.
sr_status plan_queries(const sr_snapshot* snap, const sr_cluster* c, const sr_candidates* cands, const int32_t* at_pod,
                       const int32_t* node_of_pod, PlanQueries* out);

// Allowed pods minus pods of every spot node ([n_pad], pads 0), clamped to
// int32: slack >= 1 is the atom-0 row.
void node_slack(const sr_snapshot* snap, int32_t n_pad, std::vector<int32_t>* out);

// explain_node in a plain context: on a touched node (e != nullptr) PODS is
// slack - pods < 1 wherever the program judges the pod count, and CPU / MEMORY
// / EPHEMERAL compare the request with free - acc; every other bit as
// explain_node leaves it.
uint32_t explain_node_ctx(const ExplainPrograms& x, const ExplainPod& p, const uint64_t* atoms, int32_t Wp,
                          const int64_t* node_free, int32_t n_pad, int32_t node, int32_t slack, const PlanCtxEntry* e);

// sr_shortfall_pods / sr_shortfall_plan: what the node is short of, given the
// mask explain_node / explain_node_ctx gave it (the statement the shortfall
// kernels follow).  out[SR_SHORT_*] is 0 where the mask lacks the bit.  cpu /
// memory / ephemeral: request - (free - acc), which the encoder's ranges keep
// below 2^63 (requests and node quantities lie in [0, 2^62)).  pods:
// 1 - (left - earlier pods there), `left` being node_left's value; allowed
// pods are any int64, so this one saturates at INT64_MAX.
void shortfall_node(uint32_t mask, const ExplainPod& p, const int64_t* node_free, int32_t n_pad, int32_t node,
                    int64_t left, const PlanCtxEntry* e, int64_t out[SR_SHORT_COUNT]);

// Allowed pods minus pods of every spot node in 64 bits ([n_pad], pads 0),
// INT64_MIN where the difference does not fit.  node_slack is this clamped to
// +-2^30.
void node_left(const sr_snapshot* snap, int32_t n_pad, std::vector<int64_t>* out);

// The entry of `node` in a sorted list [lo, hi), nullptr: untouched.
const PlanCtxEntry* find_ctx(const PlanCtxEntry* lo, const PlanCtxEntry* hi, int32_t node);

}  // namespace sr
