// query.cpp — the read-only query calls next to the planning tick: sr_explain_*, sr_shortfall_*,
// sr_node_view_*, sr_blockers_plan and sr_evacuate_plan.
//
// Every call is made of the same two steps.  encode_singles: the asked pods as single-pod candidates through
// the explain encoder (tags on), so a pod has no earlier pod of its candidate and every filter is a static atom.
// staged_pass: what the kernel reads -- the atom rows, the node free values of this encode, the explain
// programs, the pods -- up in one buffer, one launch, the results down in one copy.  Nothing of the planning
// side is read, written or re-encoded.  What a pass uploads and how its results are read
// is the stage units' business (explain_stage.hpp, blockers.hpp, evacuate.hpp); the buffers, the stream and the
// launches are this unit's.
#include "query.hpp"

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "blockers_dev.hpp"
#include "evacuate_dev.hpp"
#include "explain_dev.hpp"

namespace {

using sr::QueryCtx;

std::string& err_string(QueryCtx* q) { return *q->err; }

// `n` pods as candidates of their own into q->x_wl.
sr_status encode_singles(QueryCtx* q, const sr_snapshot* snap, const sr_cluster* cluster, const int32_t* pods, int32_t n) {
  std::vector<int32_t> off(static_cast<size_t>(n) + 1);
  for (int32_t i = 0; i <= n; ++i) off[i] = i;
  const sr_candidates singles{n, off.data(), pods, nullptr};
  q->x_enc.want_why = true;
  q->x_wl.reuse.drop();  // always a full encode: the tags belong to it
  std::string err;
  const sr_status st = sr::encode_workload(&q->x_enc, snap, cluster, &singles, &q->x_wl, &err);
  if (st != SR_OK) *q->err = err;
  return st;
}

struct PassSizes {
  size_t in_bytes;       // the upload
  size_t out_bytes;      // the downloaded prefix of the output buffer; 0: nothing comes down
  size_t dev_out_bytes;  // the output buffer on the device
  size_t zero_bytes;     // its prefix zeroed before the launch
};

// One pass through x_in / x_out.  pack(image) fills the input image; it runs once the buffers are there and
// before the upload, so a caller with a buffer of its own (sr_evacuate_plan's scratch) readies it there.
// launch(in, out) gets the device buffers.  unpack(image) reads the downloaded prefix after the stream has
// been synchronised; a pass that brings nothing down (node view) returns with its launch in the stream.
// The synchronise at the start waits for the staging buffers of the call before; it does not touch the
// planner's in_flight (a query call leaves the tick's own bookkeeping alone).
template <class Pack, class Launch, class Unpack>
sr_status staged_pass(QueryCtx* q, const PassSizes& z, Pack&& pack, Launch&& launch, Unpack&& unpack) {
  HIP_TRY(q, hipSetDevice(q->device));
  HIP_TRY(q, hipStreamSynchronize(q->stream));
  HIP_TRY(q, host_reserve(q->hx_in, z.in_bytes));
  HIP_TRY(q, host_reserve(q->hx_out, z.out_bytes));
  HIP_TRY(q, dev_reserve(q->x_in, z.in_bytes));
  HIP_TRY(q, dev_reserve(q->x_out, z.dev_out_bytes));
  sr_status st = pack(static_cast<char*>(q->hx_in.p));
  if (st != SR_OK) return st;
  HIP_TRY(q, hipMemcpyAsync(q->x_in.p, q->hx_in.p, z.in_bytes, hipMemcpyHostToDevice, q->stream));
  if (z.zero_bytes) HIP_TRY(q, hipMemsetAsync(q->x_out.p, 0, z.zero_bytes, q->stream));
  st = launch(static_cast<const char*>(q->x_in.p), static_cast<char*>(q->x_out.p));
  if (st != SR_OK || z.out_bytes == 0) return st;
  HIP_TRY(q, hipMemcpyAsync(q->hx_out.p, q->x_out.p, z.out_bytes, hipMemcpyDeviceToHost, q->stream));
  HIP_TRY(q, hipStreamSynchronize(q->stream));
  unpack(static_cast<const char*>(q->hx_out.p));
  return SR_OK;
}

// A node-view call: every pass of it adds its active pods into the call's totals (view_begin, view_end).
struct NodeViewCall {
  sr_node_view_out* out;
  int32_t per = 0;      // SR_NODE_VIEW_CHUNK
  int32_t judged = 0;   // active pods of the passes so far
};

// What an explain pass computes and where it goes.  kWhy: the explain kernels into `out`.  kShortfall: the
// sibling kernels (k_shortfall, k_shortfall_plan), which read the nodes' pod slack in 64 bits (node_left, in the
// place of node_slack) and leave per-block partials that k_shortfall_close closes on the same stream, into
// `out` and `sh`.  kNodeView: the kernels of node_view.hip; no per-query output is staged and nothing comes
// down, the pass adds into the totals of `view`.
struct ExplainTo {
  enum Kind { kWhy, kShortfall, kNodeView } kind;
  sr_explain_out* out;
  sr_shortfall_out* sh;
  NodeViewCall* view;
  static ExplainTo why(sr_explain_out* out) { return {kWhy, out, nullptr, nullptr}; }
  static ExplainTo shortfall(sr_explain_out* out, sr_shortfall_out* sh) { return {kShortfall, out, sh, nullptr}; }
  static ExplainTo node_view(NodeViewCall* view) { return {kNodeView, nullptr, nullptr, view}; }
};

// One explain pass over `pods`, each a candidate of its own.  With `pq` (sr_explain_plan's batched pass) the
// pods are its stop pods, pod i carries the context list pq->off[i] and the kernels are the ones that read the
// lists and the nodes' pod slack from the same buffer.  `slot` (nullptr: i) is where pod i's results go.
sr_status explain(QueryCtx* q, const sr_snapshot* snap, const sr_cluster* cluster, const int32_t* pods, int32_t n,
                  const ExplainTo& to, const sr::PlanQueries* pq = nullptr, const int32_t* slot = nullptr) {
  if (n == 0) return SR_OK;
  sr_status st = encode_singles(q, snap, cluster, pods, n);
  if (st != SR_OK) return st;
  const sr::Workload& w = q->x_wl;
  const bool view = to.kind == ExplainTo::kNodeView, shortfall = to.kind == ExplainTo::kShortfall;
  for (int32_t i = 0; i < n; ++i) {  // a fallback pod: nothing evaluated
    const uint8_t fb = w.status_host[i] == SR_CAND_FALLBACK ? 1 : 0;
    if (!view) sr::clear_slot(to.out, to.sh, static_cast<size_t>(slot ? slot[i] : i), static_cast<size_t>(w.n_spot), fb);
    else if (to.view->out->fallback) to.view->out->fallback[slot ? slot[i] : i] = fb;
  }
  if (w.pod_src.empty()) return SR_OK;
  sr::ExplainStage& x = q->x_stage;
  if (view) {
    const sr::NodeViewAsk ask{slot, to.view->per};
    st = x.plan(w, q->x_enc.node_free, snap, pq, true, false, false, q->err, &ask);
  } else {
    st = x.plan(w, q->x_enc.node_free, snap, pq, shortfall, to.out->node_mask != nullptr,
                shortfall && to.sh->node_short, q->err);
  }
  if (st != SR_OK) return st;
  const sr::StageLayout& at = x.at();
  return staged_pass(
      q, PassSizes{at.in_bytes, at.out_bytes, at.dev_out_bytes, at.zero_bytes},
      [&](char* image) {
        x.pack(image);
        return SR_OK;
      },
      [&](const char* in, char* out) -> sr_status {
        sr::ExplainPlanArgs pa;
        if (view) {  // (the totals were zeroed by view_begin and stay on the device until view_end)
          if (static_cast<size_t>(w.n_spot) != snap->nodes.size()) {
            *q->err = "node view: the encode's spot nodes are not the snapshot's";
            return SR_ERR_STATE;
          }
          sr::NodeViewArgs na;
          x.view_args(in, out, static_cast<char*>(q->x_view.p), &pa, &na);
          HIP_TRY(q, sr::launch_node_view(pa, na, q->stream));
          to.view->judged += x.n_pods();
          return SR_OK;
        }
        sr::ShortfallArgs sa;
        x.args(in, out, &pa, &sa);
        if (pq && shortfall) HIP_TRY(q, sr::launch_shortfall_plan(pa, sa, q->stream));
        else if (pq) HIP_TRY(q, sr::launch_explain_plan(pa, q->stream));
        else if (shortfall) HIP_TRY(q, sr::launch_shortfall(pa.x, sa, q->stream));
        else HIP_TRY(q, sr::launch_explain(pa.x, q->stream));
        if (shortfall) HIP_TRY(q, sr::launch_shortfall_close(x.n_pods(), sa, q->stream));
        return SR_OK;
      },
      [&](const char* image) { x.unpack(image, slot, to.out, to.sh); });
}

bool explain_out_ok(const sr_explain_out* out) { return out && out->feasible && out->first && out->counts; }

bool view_out_ok(const sr_node_view_out* o) {
  return o && o->judged && o->admits && o->near && o->refuses && o->sole && o->sole_min && o->sole_at;
}

bool shortfall_out_ok(const sr_shortfall_out* sh) {
  return sh && sh->near && sh->only_nodes && sh->only_min && sh->only_at;
}

// The caller's arrays as of no judged query, and the call's totals zeroed on the stream (once a call).
sr_status view_begin(QueryCtx* q, const sr_snapshot* snap, NodeViewCall* view, bool device) {
  const size_t ns = snap->nodes.size();
  sr::node_view_clear(view->out, ns);
  if (const char* b = std::getenv("SR_NODE_VIEW_CHUNK")) view->per = std::max(0, std::atoi(b));
  if (!device || ns == 0) return SR_OK;
  const size_t bytes = sr::node_view_layout(static_cast<size_t>(sr::node_view_stride(static_cast<int32_t>(ns))), 1).bytes;
  HIP_TRY(q, hipSetDevice(q->device));
  HIP_TRY(q, hipStreamSynchronize(q->stream));  // (the totals of the call before)
  HIP_TRY(q, dev_reserve(q->x_view, bytes));
  HIP_TRY(q, host_reserve(q->hx_view, bytes));
  HIP_TRY(q, hipMemsetAsync(q->x_view.p, 0, bytes, q->stream));
  return SR_OK;
}

// The totals down in one copy and into the caller's arrays.
sr_status view_end(QueryCtx* q, const sr_snapshot* snap, NodeViewCall* view) {
  const size_t ns = snap->nodes.size();
  *view->out->judged = view->judged;
  if (view->judged == 0 || ns == 0) return SR_OK;
  const size_t stride = static_cast<size_t>(sr::node_view_stride(static_cast<int32_t>(ns)));
  const size_t bytes = sr::node_view_layout(stride, 1).bytes;
  HIP_TRY(q, hipMemcpyAsync(q->hx_view.p, q->x_view.p, bytes, hipMemcpyDeviceToHost, q->stream));
  HIP_TRY(q, hipStreamSynchronize(q->stream));
  sr::node_view_unpack(static_cast<const char*>(q->hx_view.p), stride, ns, view->out);
  return SR_OK;
}

// An sr_explain_out of the call's own where the caller of sr_shortfall_* wants none.
struct OwnExplainOut {
  std::vector<int32_t> feasible, first, counts;
  sr_explain_out out{};
  explicit OwnExplainOut(int32_t n) : feasible(std::max(n, 1)), first(std::max(n, 1)), counts(size_t(std::max(n, 1)) * SR_WHY_COUNT) {
    out.feasible = feasible.data();
    out.first = first.data();
    out.counts = counts.data();
  }
};

// sr_explain_plan, sr_shortfall_plan and sr_node_view_plan by `to`.  The plain contexts (explain_plan.hpp) go
// through one encode of their stop pods against the base snapshot, one upload, one launch and one download;
// every other asked candidate through Fork / AddPod / explain / Revert, as sr_explain_candidate does it.  A
// stop pod the batched encode hands back as fallback is asked again on its own when the batch held other pods:
// candidates of one encode share the state word's host-port bits, so only an encode of its own tells "outside
// the encoded set" for certain.  (Node view: the batched pass and every SINGLE candidate add into the same
// totals.)
sr_status explain_plan(QueryCtx* q, sr_snapshot* snap, const sr_cluster* cluster, const sr_candidates* cands,
                       const int32_t* at_pod, const int32_t* node_of_pod, const ExplainTo& to, uint8_t* out_how) {
  const int32_t nc = cands->n_cand;
  if (nc > 0 && (!cands->cand_pod_off || !cands->cand_pods || !at_pod)) return SR_ERR_INVALID_ARG;
  if (snap->forked) return SR_ERR_STATE;
  // (the queries are built apart from the context: an argument error returns before the context is looked at)
  sr::PlanQueries pq;
  sr_status st = sr::plan_queries(snap, cluster, cands, at_pod, node_of_pod, &pq);
  if (st != SR_OK) return st;
  const size_t ns = snap->nodes.size();
  const int32_t nb = static_cast<int32_t>(pq.batched.size());
  NodeViewCall* view = to.view;
  if (view) {
    bool asked = false;
    for (int32_t c = 0; c < nc; ++c) asked = asked || pq.how[c] != SR_EXPLAIN_NONE;
    st = view_begin(q, snap, view, asked);
    if (st != SR_OK) return st;
    if (view->out->fallback) std::fill_n(view->out->fallback, nc, uint8_t(0));
  } else {
    for (int32_t c = 0; c < nc; ++c)  // not asked: as a fallback pod, but fallback = 0
      if (pq.how[c] == SR_EXPLAIN_NONE) sr::clear_slot(to.out, to.sh, static_cast<size_t>(c), ns, 0);
  }
  st = explain(q, snap, cluster, pq.pods.data(), nb, to, &pq, pq.batched.data());
  if (st != SR_OK) return st;
  if (nb > 1)
    for (int32_t i = 0; i < nb; ++i)
      if (q->x_wl.status_host[i] == SR_CAND_FALLBACK) pq.how[pq.batched[i]] = SR_EXPLAIN_SINGLE;
  const int32_t* off = cands->cand_pod_off;
  for (int32_t c = 0; c < nc; ++c) {
    if (pq.how[c] != SR_EXPLAIN_SINGLE) continue;
    st = sr_snapshot_fork(snap);
    if (st != SR_OK) return st;
    const int32_t* pods = cands->cand_pods + off[c];
    // (node_of_pod may be NULL when no asked candidate has an earlier pod)
    const int32_t* map = node_of_pod ? node_of_pod + (off[c] - off[0]) : nullptr;
    for (int32_t k = 0; k < at_pod[c]; ++k) sr::snapshot_add_pod(snap, cluster, pods[k], map[k]);
    st = explain(q, snap, cluster, pods + at_pod[c], 1, to, nullptr, &c);
    const sr_status rv = sr_snapshot_revert(snap);
    if (st != SR_OK || rv != SR_OK) return st != SR_OK ? st : rv;
  }
  if (view) {
    st = view_end(q, snap, view);
    if (st != SR_OK) return st;
  }
  if (out_how) std::copy(pq.how.begin(), pq.how.end(), out_how);
  return SR_OK;
}

// sr_blockers_plan's batched pass: the pods of every candidate that is plain as a whole (blockers.hpp), encoded
// as single-pod candidates against the snapshot as it is; one launch of k_blockers (a wave a candidate).  A
// candidate the encode hands a fallback pod back for leaves the batch (ways->how becomes SINGLE), for the
// reason given above explain_plan.
sr_status blockers_batched(QueryCtx* q, const sr_snapshot* snap, const sr_cluster* cluster, const sr_candidates* cands,
                           sr::BlockerWays* ways, sr_blockers_out* out) {
  std::vector<int32_t> flat;
  sr::blockers_flat(cands, *ways, &flat);
  if (flat.empty()) {  // (asked candidates without pods)
    for (int32_t c : ways->batched) out->blockers[c] = 0;
    return SR_OK;
  }
  sr_status st = encode_singles(q, snap, cluster, flat.data(), static_cast<int32_t>(flat.size()));
  if (st != SR_OK) return st;
  sr::BlockersStage& x = q->b_stage;
  st = x.plan(q->x_wl, q->x_enc.node_free, snap, cluster, cands, ways, out->counts != nullptr, q->err);
  if (st != SR_OK || x.n_cand() == 0) return st;
  return staged_pass(
      q, PassSizes{x.at().in_bytes, x.at().out_bytes, x.at().out_bytes, x.at().zero_bytes},
      [&](char* image) {
        x.pack(image);
        return SR_OK;
      },
      [&](const char* in, char* dev_out) -> sr_status {
        sr::BlockersArgs ba;
        x.args(in, dev_out, &ba);
        HIP_TRY(q, sr::launch_blockers(ba, q->stream));
        return SR_OK;
      },
      [&](const char* image) { x.unpack(image, cands, out); });
}

// ... and one SINGLE candidate: the loop of the contract itself, every pod explained alone against the forked
// snapshot that holds the pods placed before it.
sr_status blockers_single(QueryCtx* q, sr_snapshot* snap, const sr_cluster* cluster, const sr_candidates* cands, int32_t c,
                          sr_blockers_out* out) {
  const int32_t* off = cands->cand_pod_off;
  const int32_t* pods = cands->cand_pods + off[c];
  const int32_t np = off[c + 1] - off[c];
  const size_t p0 = static_cast<size_t>(off[c] - off[0]);
  sr_status st = sr_snapshot_fork(snap);
  if (st != SR_OK) return st;
  OwnExplainOut own(1);
  uint8_t fb = 0;
  own.out.fallback = &fb;
  int32_t blockers = 0, first = -1;
  for (int32_t k = 0; k < np && st == SR_OK && !fb; ++k) {
    st = explain(q, snap, cluster, pods + k, 1, ExplainTo::why(&own.out));
    if (st != SR_OK || fb) break;
    out->node_of_pod[p0 + k] = own.first[0];
    if (own.first[0] >= 0) {
      sr::snapshot_add_pod(snap, cluster, pods[k], own.first[0]);
      continue;
    }
    ++blockers;
    if (first < 0) first = k;
    if (out->counts) std::copy_n(own.counts.data(), SR_WHY_COUNT, out->counts + (p0 + k) * SR_WHY_COUNT);
  }
  const sr_status rv = sr_snapshot_revert(snap);
  if (st != SR_OK || rv != SR_OK) return st != SR_OK ? st : rv;
  if (fb) {
    sr::blockers_clear(cands, c, 1, out);
  } else {
    out->blockers[c] = blockers;
    out->first[c] = first;
  }
  return SR_OK;
}

// One pass of sr_evacuate_plan over the scenarios `ids` (all JUDGED by the rule): their pods encoded as
// single-pod candidates against the standing snapshot; one launch of k_evacuate (a block of waves a scenario,
// grid-stride).  A scenario the encode hands a fallback pod back for is not planned and appended to *fell.
sr_status evacuate_pass(QueryCtx* q, const sr_snapshot* snap, const sr_cluster* cluster, const sr_candidates* scen,
                        const int32_t* lost_off, const int32_t* lost_pos, const std::vector<int32_t>& ids,
                        std::vector<int32_t>* fell, sr_evacuate_out* out) {
  std::vector<int32_t> flat;
  sr::evacuate_flat(scen, ids, &flat);
  if (flat.empty()) {  // (scenarios without pods)
    for (int32_t s : ids) {
      out->stranded[s] = 0;
      if (out->how) out->how[s] = SR_EVAC_JUDGED;
    }
    return SR_OK;
  }
  sr_status st = encode_singles(q, snap, cluster, flat.data(), static_cast<int32_t>(flat.size()));
  if (st != SR_OK) return st;
  sr::EvacuateStage& x = q->e_stage;
  st = x.plan(q->x_wl, q->x_enc.node_free, snap, cluster, scen, lost_off, lost_pos, ids, out->counts != nullptr, fell,
              q->err);
  if (st != SR_OK || x.n_scen() == 0) return st;
  int32_t blocks = 0, waves = 0;
  sr::evacuate_shape(x.n_scen(), std::getenv("SR_EVAC_GRID"), std::getenv("SR_EVAC_WAVES"), &blocks, &waves);
  const sr::EvacuateScratch sc = sr::evacuate_scratch(x.n_pad(), blocks);
  return staged_pass(
      q, PassSizes{x.at().in_bytes, x.at().out_bytes, x.at().out_bytes, x.at().zero_bytes},
      [&](char* image) -> sr_status {
        if (sc.bytes > q->e_scratch.cap) q->e_scratch_zero = false;
        HIP_TRY(q, dev_reserve(q->e_scratch, sc.bytes));
        if (!q->e_scratch_zero && q->e_scratch.p)
          HIP_TRY(q, hipMemsetAsync(q->e_scratch.p, 0, q->e_scratch.cap, q->stream));
        q->e_scratch_zero = false;  // until the launch is known to have finished
        x.pack(image);
        return SR_OK;
      },
      [&](const char* in, char* dev_out) -> sr_status {
        sr::EvacuateArgs ea;
        x.args(in, dev_out, static_cast<char*>(q->e_scratch.p), blocks, waves, &ea);
        HIP_TRY(q, sr::launch_evacuate(ea, blocks, q->stream));
        return SR_OK;
      },
      [&](const char* image) {
        q->e_scratch_zero = true;  // (the stream was synchronised behind the launch)
        x.unpack(image, scen, out);
      });
}

}  // namespace

extern "C" {

sr_status sr_explain_pods(sr_ctx* ctx, const sr_snapshot* snap, const sr_cluster* cluster, const int32_t* pods, int32_t n,
                          sr_explain_out* out) {
  if (!ctx || !snap || !cluster || n < 0 || !explain_out_ok(out) || (n > 0 && !pods)) return SR_ERR_INVALID_ARG;
  return explain(sr::query_ctx(ctx), snap, cluster, pods, n, ExplainTo::why(out));
}

sr_status sr_explain_candidate(sr_ctx* ctx, sr_snapshot* snap, const sr_cluster* cluster, const int32_t* pods, int32_t n,
                               const int32_t* node_of_pod, int32_t at_pod, sr_explain_out* out) {
  if (!ctx || !snap || !cluster || n < 0 || !explain_out_ok(out) || !pods || !node_of_pod) return SR_ERR_INVALID_ARG;
  if (snap->forked) return SR_ERR_STATE;
  if (at_pod < 0 || at_pod >= n) return SR_ERR_INVALID_ARG;
  const int32_t n_spot = static_cast<int32_t>(snap->nodes.size());
  for (int32_t k = 0; k <= at_pod; ++k)
    if (pods[k] < 0 || pods[k] >= cluster->pods.n || (k < at_pod && (node_of_pod[k] < 0 || node_of_pod[k] >= n_spot)))
      return SR_ERR_INVALID_ARG;
  // Fork; the earlier pods where the plan put them (rescheduler.go:366): base
  // pods now, so what they do to pods[at_pod] is static atoms; Revert
  sr_status st = sr_snapshot_fork(snap);
  if (st != SR_OK) return st;
  for (int32_t k = 0; k < at_pod; ++k) sr::snapshot_add_pod(snap, cluster, pods[k], node_of_pod[k]);
  st = explain(sr::query_ctx(ctx), snap, cluster, pods + at_pod, 1, ExplainTo::why(out));
  const sr_status rv = sr_snapshot_revert(snap);
  return st != SR_OK ? st : rv;
}

sr_status sr_explain_plan(sr_ctx* ctx, sr_snapshot* snap, const sr_cluster* cluster, const sr_candidates* cands,
                          const int32_t* at_pod, const int32_t* node_of_pod, sr_explain_out* out, uint8_t* out_how) {
  if (!ctx || !snap || !cluster || !cands || cands->n_cand < 0 || !explain_out_ok(out)) return SR_ERR_INVALID_ARG;
  return explain_plan(sr::query_ctx(ctx), snap, cluster, cands, at_pod, node_of_pod, ExplainTo::why(out), out_how);
}

sr_status sr_shortfall_pods(sr_ctx* ctx, const sr_snapshot* snap, const sr_cluster* cluster, const int32_t* pods, int32_t n,
                            sr_explain_out* why, sr_shortfall_out* out) {
  if (!ctx || !snap || !cluster || n < 0 || !shortfall_out_ok(out) || (why && !explain_out_ok(why)) || (n > 0 && !pods))
    return SR_ERR_INVALID_ARG;
  OwnExplainOut own(why ? 0 : n);
  return explain(sr::query_ctx(ctx), snap, cluster, pods, n, ExplainTo::shortfall(why ? why : &own.out, out));
}

sr_status sr_shortfall_plan(sr_ctx* ctx, sr_snapshot* snap, const sr_cluster* cluster, const sr_candidates* cands,
                            const int32_t* at_pod, const int32_t* node_of_pod, sr_explain_out* why, sr_shortfall_out* out,
                            uint8_t* out_how) {
  if (!ctx || !snap || !cluster || !cands || cands->n_cand < 0 || !shortfall_out_ok(out) || (why && !explain_out_ok(why)))
    return SR_ERR_INVALID_ARG;
  OwnExplainOut own(why ? 0 : cands->n_cand);
  return explain_plan(sr::query_ctx(ctx), snap, cluster, cands, at_pod, node_of_pod,
                      ExplainTo::shortfall(why ? why : &own.out, out), out_how);
}

sr_status sr_node_view_pods(sr_ctx* ctx, const sr_snapshot* snap, const sr_cluster* cluster, const int32_t* pods, int32_t n,
                            sr_node_view_out* out) {
  if (!ctx || !snap || !cluster || n < 0 || !view_out_ok(out) || (n > 0 && !pods)) return SR_ERR_INVALID_ARG;
  QueryCtx* q = sr::query_ctx(ctx);
  NodeViewCall view{out};
  sr_status st = view_begin(q, snap, &view, n > 0);
  if (st != SR_OK) return st;
  st = explain(q, snap, cluster, pods, n, ExplainTo::node_view(&view));
  return st != SR_OK ? st : view_end(q, snap, &view);
}

sr_status sr_node_view_plan(sr_ctx* ctx, sr_snapshot* snap, const sr_cluster* cluster, const sr_candidates* cands,
                            const int32_t* at_pod, const int32_t* node_of_pod, sr_node_view_out* out, uint8_t* out_how) {
  if (!ctx || !snap || !cluster || !cands || cands->n_cand < 0 || !view_out_ok(out)) return SR_ERR_INVALID_ARG;
  NodeViewCall view{out};
  return explain_plan(sr::query_ctx(ctx), snap, cluster, cands, at_pod, node_of_pod, ExplainTo::node_view(&view), out_how);
}

sr_status sr_blockers_plan(sr_ctx* ctx, sr_snapshot* snap, const sr_cluster* cluster, const sr_candidates* cands,
                           const int32_t* ask, sr_blockers_out* out, uint8_t* out_how) {
  if (!ctx || !snap || !cluster || !cands || cands->n_cand < 0 || !out || !out->blockers || !out->first)
    return SR_ERR_INVALID_ARG;
  const int32_t nc = cands->n_cand;
  if (nc == 0) return SR_OK;
  if (!cands->cand_pod_off || !ask) return SR_ERR_INVALID_ARG;
  const int32_t* off = cands->cand_pod_off;
  if (off[nc] < off[0] || (off[nc] > off[0] && (!cands->cand_pods || !out->node_of_pod))) return SR_ERR_INVALID_ARG;
  if (snap->forked) return SR_ERR_STATE;
  // (the ways are decided apart from the context: an argument error returns before the context is looked at)
  sr::BlockerWays ways;
  sr_status st = sr::blockers_ways(snap, cluster, cands, ask, &ways);
  if (st != SR_OK) return st;
  for (int32_t c = 0; c < nc; ++c) sr::blockers_clear(cands, c, 0, out);
  QueryCtx* q = sr::query_ctx(ctx);
  st = blockers_batched(q, snap, cluster, cands, &ways, out);
  if (st != SR_OK) return st;
  for (int32_t c = 0; c < nc; ++c) {
    if (ways.how[c] != SR_EXPLAIN_SINGLE) continue;
    st = blockers_single(q, snap, cluster, cands, c, out);
    if (st != SR_OK) return st;
  }
  if (out_how) std::copy(ways.how.begin(), ways.how.end(), out_how);
  return SR_OK;
}

sr_status sr_evacuate_plan(sr_ctx* ctx, const sr_snapshot* snap, const sr_cluster* cluster, const sr_candidates* scen,
                           const int32_t* lost_off, const int32_t* lost_pos, sr_evacuate_out* out) {
  if (!ctx || !snap || !cluster || !scen || scen->n_cand < 0 || !out || !out->stranded || !out->first)
    return SR_ERR_INVALID_ARG;
  const int32_t nc = scen->n_cand;
  if (nc == 0) return SR_OK;
  if (!scen->cand_pod_off || !lost_off) return SR_ERR_INVALID_ARG;
  const int32_t* off = scen->cand_pod_off;
  if (off[nc] < off[0] || (off[nc] > off[0] && (!scen->cand_pods || !out->node_of_pod))) return SR_ERR_INVALID_ARG;
  if (lost_off[nc] < lost_off[0] || (lost_off[nc] > lost_off[0] && !lost_pos)) return SR_ERR_INVALID_ARG;
  if (snap->forked) return SR_ERR_STATE;
  // (the rule is decided apart from the context: an argument error returns before the context is looked at)
  sr::EvacuateWays ways;
  sr_status st = sr::evacuate_ways(snap, cluster, scen, lost_off, lost_pos, &ways);
  if (st != SR_OK) return st;
  for (int32_t s = 0; s < nc; ++s) sr::evacuate_clear(scen, s, ways.how[s], out);
  QueryCtx* q = sr::query_ctx(ctx);
  std::vector<int32_t> fell;
  st = evacuate_pass(q, snap, cluster, scen, lost_off, lost_pos, ways.judged, &fell, out);
  if (st != SR_OK) return st;
  // candidates of one encode share the state word's host-port bits (see explain_plan): a scenario the shared
  // encode handed a fallback pod back for is asked again alone before SR_EVAC_FALLBACK stands
  for (int32_t s : fell) {
    std::vector<int32_t> again;
    if (ways.judged.size() > 1) {
      st = evacuate_pass(q, snap, cluster, scen, lost_off, lost_pos, std::vector<int32_t>{s}, &again, out);
      if (st != SR_OK) return st;
    } else {
      again.push_back(s);
    }
    if (!again.empty()) sr::evacuate_clear(scen, s, SR_EVAC_FALLBACK, out);
  }
  return SR_OK;
}

}  // extern "C"
