// explain_stage.hpp — the two staged buffers of an explain / shortfall call (sr_explain_pods,
// sr_explain_plan, sr_shortfall_pods, sr_shortfall_plan): what goes up in one copy, what comes back in one,
// and where each part lies.
//
// HIP-free.  query.cpp's explain() owns the buffers, the stream and the launches; this unit validates
// what the kernels index with, lays the buffers out (plan), writes the input image (pack), points the kernel
// arguments into the buffers (args) and reads the downloaded image into the caller's arrays (unpack).  The
// part tables and the checks it shares with the blockers and evacuate stages are stage_base.hpp's.
// tools/shortfall_check.cpp runs all four on the host over exact-size heap blocks, under the sanitizers.
#pragma once

#include <string>
#include <vector>

#include "node_view.hpp"
#include "stage_base.hpp"

struct sr_snapshot;

namespace sr {

struct Workload;

// The input parts in buffer order: stage_base.hpp's common ones (IN_PODS: ExplainPod), then
enum StageIn {
  IN_CTX = IN_COMMON,  // PlanCtxEntry, lists only
  IN_COFF,             // int32 [n_pods + 1], lists only
  IN_SLACK,  // shortfall / node view: node_left, int64 [n_pad]; else with lists: node_slack, int32 [n_pad]; else absent
  IN_PARTS
};
enum StageOut {
  OUT_SUMS,    // int32 [n_pods][kExplainSums]
  OUT_SSUMS,   // int32 [n_pods][kShortSums], shortfall only (as the next two)
  OUT_OMIN,    // int64 [n_pods][SR_SHORT_COUNT]
  OUT_OAT,     // int32 [n_pods][SR_SHORT_COUNT]
  OUT_NSHORT,  // int64 [n_pods][n_spot][SR_SHORT_COUNT], when wanted
  OUT_MASKS,   // uint16 [n_pods][n_spot], when wanted; the download ends with it
  OUT_PMIN,    // uint64 [n_pods][blocks][SR_SHORT_COUNT]: the blocks' partials stay on the device (shortfall only)
  OUT_PAT,     // int32 [n_pods][blocks][SR_SHORT_COUNT]
  OUT_PARTS
};

struct StageLayout {
  StagePart in[IN_PARTS], out[OUT_PARTS];
  size_t in_bytes = 0;       // the upload
  size_t zero_bytes = 0;     // prefix of the output buffer zeroed before the launch (the sums the blocks add into)
  size_t out_bytes = 0;      // the downloaded prefix
  size_t dev_out_bytes = 0;  // ... and the partials behind it
  // the node-view switch (absent without it): behind the parts above in their buffers, inside in_bytes /
  // dev_out_bytes
  StagePart view_slot;  // input: int32 [n_pods] the slot of every active pod
  StagePart view_part;  // output, device only: the chunks' partial rows, node_view_layout(n_pad, chunks)
};

// The context lists of `pq` in active-pod order: list q is the one of asked pod w.pod_src[q] - w.pod_base.
void active_lists(const Workload& w, const PlanQueries& pq, std::vector<PlanCtxEntry>* entries,
                  std::vector<int32_t>* off);

// "Nothing evaluated" in result slot `o`: a fallback pod (fallback = 1) or a candidate not asked (0).
void clear_slot(sr_explain_out* out, sr_shortfall_out* sh, size_t o, size_t n_spot, uint8_t fallback);

// The node-view switch of plan(): the per-node reduction of sr_node_view_pods / sr_node_view_plan in place of
// every per-query output.  The call's totals are no part of the two buffers: they live through the several
// passes of one call (the batched pass and every SINGLE candidate), between which the output buffer may be
// allocated anew, so query.cpp keeps them in a buffer of their own, node_view_layout(node_view_stride(n_spot), 1)
// long.  `judged` needs no device word: it is the number of active pods, which the host knows.
struct NodeViewAsk {
  const int32_t* slot = nullptr;  // asked index -> slot, nullptr: the asked index (as unpack's `slot`)
  int32_t per = 0;                // SR_NODE_VIEW_CHUNK, 0: node_view_chunks decides
};

// One call's staging.  The vectors keep their capacity from call to call; everything else is of the last plan()
// and valid while the workload and node_free it was given stand.  Read-only from outside: what plan() decided
// cannot be changed between it and pack / args / unpack.
class ExplainStage {
 public:
  // Checks the encoded explain workload (`node_free`: EncoderCache::node_free of its encode), builds what
  // the kernel reads and lays both buffers out.  pq != nullptr: context lists (sr_explain_plan); `shortfall`:
  // the sibling kernels; node_mask / node_short: the optional outputs.  SR_ERR_STATE with *err set when the
  // workload holds something a kernel would index out of bounds with.  w has at least one active pod.
  sr_status plan(const Workload& w, const std::vector<int64_t>& node_free, const sr_snapshot* snap,
                 const PlanQueries* pq, bool shortfall, bool node_mask, bool node_short, std::string* err,
                 const NodeViewAsk* view = nullptr);
  // (`view`: shortfall is implied, node_mask / node_short are not wanted, no per-query output is laid out and
  // nothing comes down from the output buffer: at().out_bytes and zero_bytes are 0)

  const StageLayout& at() const { return at_; }
  int32_t n_pods() const { return n_pods_; }  // queried (active) pods
  const ExplainPrograms& programs() const { return prog_; }
  const std::vector<PlanCtxEntry>& entries() const { return centries_; }  // the lists in active-pod order

  // The input image, at().in_bytes long.
  void pack(char* in) const;

  // The kernel arguments over the two buffers (device addresses, or host ones for the CPU check).  pa->x is
  // the ExplainArgs of the calls without lists; without lists / shortfall the rest of *pa / *sa is zero.
  void args(const char* in, char* out, ExplainPlanArgs* pa, ShortfallArgs* sa) const;
  // After plan() with `view`: the kernel arguments of node_view.hip over the two buffers and the call's totals.
  void view_args(const char* in, char* out, char* totals, ExplainPlanArgs* pa, NodeViewArgs* na) const;
  NodeViewChunks chunks() const { return chunks_; }

  // The first at().out_bytes of the output buffer into the caller's arrays: active pod q to slot[its asked
  // index] (nullptr: the asked index).  `sh` as given to plan() by `shortfall`.
  void unpack(const char* out_image, const int32_t* slot, sr_explain_out* out, sr_shortfall_out* sh) const;

 private:
  ExplainPrograms prog_;
  std::vector<ExplainPod> pods_;
  std::vector<PlanCtxEntry> centries_;  // the context lists, their offsets and the nodes' pod slack as the
  std::vector<int32_t> coff_, slack_;   //   kernel reads them
  std::vector<int64_t> left_;           // sr_shortfall_*: the nodes' pod slack in 64 bits
  std::vector<int32_t> slots_;          // node view: the slot of every active pod
  NodeViewChunks chunks_;
  bool view_ = false;
  StageLayout at_;
  int32_t n_pods_ = 0, blocks_ = 0;
  bool lists_ = false, shortfall_ = false, want_mask_ = false, want_short_ = false;
  const Workload* w_ = nullptr;
  const void* src_[IN_PARTS] = {};
};

}  // namespace sr
