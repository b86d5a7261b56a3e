// blockers.hpp — every pod that keeps a stuck candidate from draining (sr_blockers_plan), host side.
//
// HIP-free.  canDrainNode's loop with the `return err` at the first unplaceable pod replaced by "note the pod
// and go on" (sr_planner.h).  A candidate is PLAIN AS A WHOLE when no pod of it changes anything for a later
// one but its node's pod count and requested cpu / memory / ephemeral: plan_queries' rule (explain_plan.hpp)
// lifted from one stop pod to every pod, decided from the sr_cluster tables alone.  Such a candidate needs no
// Fork: its own placements are a list of {node, pods, acc[3]} sorted by node (PlanCtxEntry) that grows as the
// loop goes, and every pod is judged by explain_node_ctx against the snapshot as it is plus that list.
// blockers_candidate is that loop on the host, the statement the kernel of blockers.hip follows, one
// candidate per wave.  BlockersStage lays out, packs and unpacks the two buffers of the batched pass, which
// query.cpp owns; what it shares with sr_evacuate_plan's stage -- groups of pods (candidates here, scenarios
// there) planned one after the other by one kernel -- is GroupStage.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "stage_base.hpp"

struct sr_snapshot;

namespace sr {

// The distinct nodes a candidate's own placements can touch in the kernel's list (one LDS entry each), hence
// the pods a batched candidate may have: the host rule and the kernel share it.
constexpr int kBlockersCtx = SR_BLOCKERS_BATCH_PODS;
constexpr int kBlockersThreads = 256, kBlockersWaves = kBlockersThreads / 64;  // a wave is a candidate

// A pod of a batched candidate as the kernel reads it: what explain judges it by (the fit request) and what
// AddPod accounts for it (acc; differs from req with init containers or overhead).
struct BlockerPod {
  ExplainPod p;
  int64_t acc[3];
};
static_assert(sizeof(BlockerPod) == 56, "read by the kernel as it stands");

// The ways of a call: how[c] SR_EXPLAIN_NONE (not asked) / BATCHED / SINGLE, `batched` ascending.
struct BlockerWays {
  std::vector<uint8_t> how;
  std::vector<int32_t> batched;
};

// Checks the candidates (SR_ERR_INVALID_ARG: a negative pod count or a pod index out of range in an asked
// candidate) and sorts every asked one into its way.  BATCHED needs all of:
//   at most kBlockersCtx pods;
//   no pod with required anti-affinity; no pod but the first with affinity terms or a spread constraint;
//   at most one pod with host ports (or inline disks), at most one with scalars (or attachable volumes);
//   every pod_acc non-negative;
//   the largest requested value of any spot node plus the candidate's total acc stays below 2^62 per
//   dimension, so Requested stays a quantity the encoder takes wherever the pods land.
// Nothing is modified.
sr_status blockers_ways(const sr_snapshot* snap, const sr_cluster* c, const sr_candidates* cands, const int32_t* ask,
                        BlockerWays* out);

// The pods of the batched candidates in `batched` order, flattened: what the batched pass encodes as
// single-pod candidates.
void blockers_flat(const sr_candidates* cands, const BlockerWays& ways, std::vector<int32_t>* pods);

// The loop for one plain candidate.  node_of_pod [n]; counts [n][SR_WHY_COUNT] or nullptr: a blocker's row
// is written, every other row left as it is.  slack: node_slack's values.  Returns the blockers, *first the
// first one's index (-1: none).
int32_t blockers_candidate(const ExplainPrograms& x, const BlockerPod* pods, int32_t n, const uint64_t* atoms, int32_t Wp,
                           const int64_t* node_free, int32_t n_pad, int32_t n_spot, const int32_t* slack,
                           int32_t* node_of_pod, int32_t* counts, int32_t* first);

// What k_blockers takes (by value).  x.pods, x.sums, x.node_mask and x.pod0 are not used.
struct BlockersArgs {
  ExplainArgs x;
  const BlockerPod* pods;    // [x.n_pods] candidate after candidate
  const int32_t* cand_off;   // [n_cand + 1] into pods; no candidate has more than kBlockersCtx
  const int64_t* node_left;  // [n_pad] allowed pods - pods (node_left), pads 0
  int32_t n_cand;
  int32_t* counts;           // [x.n_pods][SR_WHY_COUNT], zeroed on the stream before the launch; nullptr: not wanted
  int32_t* node_of_pod;      // [x.n_pods]
  int32_t* blockers;         // [n_cand]
  int32_t* first;            // [n_cand]
};

// The two buffers of a pass over groups of pods, as part tables (stage_base.hpp).  Input: the common parts
// (IN_PODS: BlockerPod), GIN_OFF, the unit's own parts, and the nodes' pod slack last.  Output: GOUT_*.
constexpr int GIN_OFF = IN_COMMON;  // int32 [groups + 1] into the pods
constexpr int kGroupInMax = IN_COMMON + 4;
enum GroupOut {
  GOUT_COUNTS,       // int32 [n_pods][SR_WHY_COUNT]; absent when not wanted; the zeroed prefix
  GOUT_NODE_OF_POD,  // int32 [n_pods]
  GOUT_COUNT,        // int32 [groups]: blockers / stranded
  GOUT_FIRST,        // int32 [groups]
  GOUT_PARTS
};
struct GroupLayout {
  StagePart in[kGroupInMax], out[GOUT_PARTS];
  int n_in = 0;  // parts of `in` in use
  size_t in_bytes = 0, zero_bytes = 0, out_bytes = 0;
};
// sr_blockers_plan's input: the common parts, cand_off, node_left
enum BlockersIn { BIN_COFF = GIN_OFF, BIN_LEFT, BIN_PARTS };
using BlockersLayout = GroupLayout;

// The caller's arrays a pass over groups fills, by the caller's group and pod indices.
struct GroupResults {
  int32_t *count, *first, *node_of_pod, *counts;
  uint8_t* mark;  // [groups] or nullptr: set to `marked` for every group the kernel planned
  uint8_t marked;
};

// What BlockersStage and EvacuateStage share.  Valid while the workload, node_free and the groups given to
// plan_groups() stand.
class GroupStage {
 public:
  const GroupLayout& at() const { return at_; }
  int32_t n_pods() const { return static_cast<int32_t>(pods_.size()); }
  const ExplainPrograms& programs() const { return prog_; }
  void pack(char* in) const;  // at().in_bytes

 protected:
  // plan() in three steps.  check(): stage_workload over `w`, the errors starting with `who`.
  sr_status check(const char* who, const Workload& w, const std::vector<int64_t>& node_free, bool more_ok, std::string* err);
  // plan_groups(): check()'s `w` is the encode (tags on) of the pods of the groups `ids` of `groups`, flattened in that
  // order, as single-pod candidates (`what_pods` names them in an error).  Keeps every group of at most
  // `pod_cap` pods none of whose pods the encode handed back as fallback or left inactive: its BlockerPods, its
  // id in kept_, its end in goff_.  The others are appended to *dropped.
  sr_status plan_groups(const std::string& who, const char* what_pods, const sr_cluster* c, const sr_candidates* groups,
                        const std::vector<int32_t>& ids, size_t pod_cap, std::vector<int32_t>* dropped, std::string* err);
  // After plan_groups() and the unit's own parts in at_.in[GIN_OFF + 1 ..]: node_left as part n_in - 1, both
  // buffers laid out.
  void lay_out(const sr_snapshot* snap, int n_in, bool want_counts);
  int32_t n_groups() const { return static_cast<int32_t>(kept_.size()); }
  // The arguments every such kernel takes: the ExplainArgs prefix, the pods, the group offsets, node_left.
  void in_args(const char* in, ExplainArgs* x, const BlockerPod** pods, const int32_t** off, const int64_t** left) const;
  // ... and its four outputs (counts nullptr when not wanted)
  void out_args(char* out, int32_t** counts, int32_t** node_of_pod, int32_t** count, int32_t** first) const;
  // The first at().out_bytes of the output buffer into the caller's arrays.
  void unpack_groups(const char* image, const sr_candidates* groups, const GroupResults& r) const;

  ExplainPrograms prog_;
  std::vector<BlockerPod> pods_;
  std::vector<int32_t> goff_, kept_;  // the kernel's groups: their pods, the caller's indices
  std::vector<int64_t> left_;
  const Workload* w_ = nullptr;
  const void* src_[kGroupInMax] = {};
  GroupLayout at_;
  bool counts_ = false;
};

// Every output of candidate c as "not judged": blockers / first -1, its pods -1, zero rows, fallback as given.
void blockers_clear(const sr_candidates* cands, int32_t c, uint8_t fallback, sr_blockers_out* out);

// The staging of the batched pass.
class BlockersStage : public GroupStage {
 public:
  // `w`: the encode (tags on) of blockers_flat's pods as single-pod candidates.  A candidate one of whose
  // pods that encode handed back as fallback (or left inactive) leaves the batch: ways->how[c] becomes
  // SR_EXPLAIN_SINGLE (ways->batched is left as it was encoded).  SR_ERR_STATE with *err set when the workload
  // holds something the kernel would index out of bounds with.
  sr_status plan(const Workload& w, const std::vector<int64_t>& node_free, const sr_snapshot* snap, const sr_cluster* c,
                 const sr_candidates* cands, BlockerWays* ways, bool want_counts, std::string* err);
  int32_t n_cand() const { return n_groups(); }  // candidates the kernel plans
  void args(const char* in, char* out, BlockersArgs* a) const;
  // the first at().out_bytes of the output buffer into the caller's arrays
  void unpack(const char* image, const sr_candidates* cands, sr_blockers_out* out) const;
};

}  // namespace sr
