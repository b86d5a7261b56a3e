// query.hpp — the state of the read-only query calls (sr_explain_*, sr_shortfall_*, sr_node_view_*,
// sr_blockers_plan, sr_evacuate_plan; query.cpp), which a planning context holds as one member.
//
// The query side shares nothing with the planning tick but the device, the stream and the error string: an
// encoder, a workload and buffers of its own, outside the slots, the workload arenas and the residency model,
// so a plan before and after a query call encodes and uploads exactly the same.
#pragma once

#include <string>

#include "dev_buf.hpp"
#include "evacuate.hpp"
#include "explain_stage.hpp"
#include "host.hpp"

struct sr_ctx;

namespace sr {

struct QueryCtx {
  // the planning context's, set by sr_create
  int device = 0;
  hipStream_t stream = nullptr;
  std::string* err = nullptr;
  // the explain encoder (tags on) and the workload of the last single-pod encode
  EncoderCache x_enc;
  Workload x_wl;
  // what a pass uploads and where each part of its two buffers lies: the explain / shortfall / node-view passes
  // (explain_stage.hpp), sr_blockers_plan's batched pass (blockers.hpp), sr_evacuate_plan's passes (evacuate.hpp)
  ExplainStage x_stage;
  BlockersStage b_stage;
  EvacuateStage e_stage;
  // the one pair of staged buffers every pass goes through, and their pinned images
  DevBuf x_in, x_out;
  HostBuf hx_in, hx_out;
  // sr_node_view_*: the call's per-node totals, which every pass of one call accumulates into (x_out may be
  // allocated anew between the passes)
  DevBuf x_view;
  HostBuf hx_view;
  // sr_evacuate_plan: the blocks' dense per-node deltas.  The scratch is zero between launches -- every block
  // restores its slice -- so it is zeroed on the stream only when it was allocated anew, or when a call ended
  // before its launch was known to have finished
  DevBuf e_scratch;
  bool e_scratch_zero = false;
};

// The query state of a planning context (planner.cpp, where sr_ctx is defined; sr_destroy frees the buffers).
QueryCtx* query_ctx(sr_ctx* ctx);

}  // namespace sr
