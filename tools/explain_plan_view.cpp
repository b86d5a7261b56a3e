// Host-only view of sr_explain_plan's batched pass (csrc/explain_plan.cpp):
// built to lib/libsrexplainview.so together with the HIP-free encoder objects,
// so tests/test_explain_plan_reference.py can prove everything but the kernel
// without a GPU: which way every asked candidate goes, the context lists and
// the nodes' pod slack as the kernel reads them, and every batched query's
// per-node masks, evaluated by explain_node_ctx -- the statement the kernel
// follows.  Not part of libsrplanner.so or the ABI: the library carries its
// own copy of sr_snapshot_create / sr_snapshot_add_pod / sr_snapshot_destroy,
// and the snapshot passed in must come from it.
//   make -C k8s-spot-rescheduler_amd tools
#include <algorithm>
#include <string>
#include <vector>

#include "../k8s-spot-rescheduler_amd/csrc/blockers.hpp"
#include "../k8s-spot-rescheduler_amd/csrc/explain_stage.hpp"
#include "../k8s-spot-rescheduler_amd/csrc/host.hpp"

extern "C" {

// how[n_cand]; ctx_off[n_cand + 1] into ctx_node / ctx_pods / ctx_acc[.][3]
// (cap_entries entries each; a candidate that is not batched has an empty
// list); node_slack[n_spot]; atom0[n_spot] the encode's atom-0 row, bit by bit
// (255 everywhere when nothing is batched: no encode); node_mask[n_cand][n_spot]
// and fallback[n_cand] for the batched candidates (others: zeros).  As in the
// planner, a stop pod the batched encode hands back as fallback while other
// pods were in the batch goes the SINGLE way (the view does not evaluate it:
// zeros); alone in its batch it stays BATCHED with fallback = 1.
sr_status sr_explain_plan_view(const sr_cluster* cluster, const sr_snapshot* snap, const sr_candidates* cands,
                               const int32_t* at_pod, const int32_t* node_of_pod, uint8_t* how, int32_t* ctx_off,
                               int32_t* ctx_node, int32_t* ctx_pods, int64_t* ctx_acc, int32_t cap_entries,
                               int32_t* node_slack, uint8_t* atom0, uint16_t* node_mask, uint8_t* fallback) {
  if (!cluster || !snap || !cands || !at_pod || !how || !ctx_off || !node_slack || !atom0 || !node_mask || !fallback)
    return SR_ERR_INVALID_ARG;
  sr::PlanQueries pq;
  sr_status st = sr::plan_queries(snap, cluster, cands, at_pod, node_of_pod, &pq);
  if (st != SR_OK) return st;
  const int32_t nc = cands->n_cand, nb = static_cast<int32_t>(pq.batched.size());
  const size_t ns = snap->nodes.size();
  if (static_cast<int32_t>(pq.entries.size()) > cap_entries) return SR_ERR_INVALID_ARG;
  std::copy(pq.how.begin(), pq.how.end(), how);
  std::fill_n(node_mask, static_cast<size_t>(nc) * ns, uint16_t(0));
  std::fill_n(fallback, nc, uint8_t(0));
  std::fill_n(atom0, ns, uint8_t(255));
  ctx_off[0] = 0;
  for (int32_t c = 0, b = 0; c < nc; ++c) {
    ctx_off[c + 1] = ctx_off[c];
    if (b < nb && pq.batched[b] == c) {
      for (int32_t j = pq.off[b]; j < pq.off[b + 1]; ++j) {
        const int32_t o = ctx_off[c + 1]++;
        ctx_node[o] = pq.entries[j].node;
        ctx_pods[o] = pq.entries[j].pods;
        for (int d = 0; d < 3; ++d) ctx_acc[o * 3 + d] = pq.entries[j].acc[d];
      }
      ++b;
    }
  }
  if (nb == 0) {
    std::vector<int32_t> slack;
    sr::node_slack(snap, static_cast<int32_t>(ns), &slack);
    std::copy(slack.begin(), slack.end(), node_slack);
    return SR_OK;
  }
  // the stop pods as candidates of their own against the base snapshot, tags on
  std::vector<int32_t> off(static_cast<size_t>(nb) + 1);
  for (int32_t i = 0; i <= nb; ++i) off[i] = i;
  const sr_candidates stops{nb, off.data(), pq.pods.data(), nullptr};
  sr::EncoderCache cache;
  cache.want_why = true;
  sr::Workload w;
  std::string err;
  st = sr::encode_workload(&cache, snap, cluster, &stops, &w, &err);
  if (st != SR_OK) return st;
  for (int32_t i = 0; i < nb; ++i) {
    if (w.status_host[i] != SR_CAND_FALLBACK) continue;
    if (nb > 1) how[pq.batched[i]] = SR_EXPLAIN_SINGLE;
    else fallback[pq.batched[i]] = 1;
  }
  std::vector<int32_t> slack;
  sr::node_slack(snap, std::max(w.n_pad, static_cast<int32_t>(ns)), &slack);
  std::copy_n(slack.begin(), ns, node_slack);
  if (w.n_atoms > 0 && w.atoms.size() >= static_cast<size_t>(w.Wp) && static_cast<size_t>(w.Wp) * 64 >= ns)
    for (size_t j = 0; j < ns; ++j) atom0[j] = static_cast<uint8_t>(w.atoms[j >> 6] >> (j & 63) & 1);
  const int32_t na = static_cast<int32_t>(w.pod_src.size());
  if (na == 0) return SR_OK;
  sr::ExplainPrograms x;
  std::vector<sr::ExplainPod> xp;
  if (!sr::build_explain(w, &x) || w.pod_cls.size() != static_cast<size_t>(na)) return SR_ERR_STATE;
  sr::explain_pods(w, &xp);
  std::vector<sr::PlanCtxEntry> entries;  // the lists in active-pod order
  std::vector<int32_t> eoff;
  sr::active_lists(w, pq, &entries, &eoff);
  for (int32_t q = 0; q < na; ++q) {
    const sr::PlanCtxEntry *lo = entries.data() + eoff[q], *hi = entries.data() + eoff[q + 1];
    uint16_t* row = node_mask + static_cast<size_t>(pq.batched[w.pod_src[q] - w.pod_base]) * ns;
    for (int32_t node = 0; node < static_cast<int32_t>(ns); ++node)
      row[node] = static_cast<uint16_t>(sr::explain_node_ctx(x, xp[q], w.atoms.data(), w.Wp, cache.node_free.data(),
                                                             w.n_pad, node, slack[node], sr::find_ctx(lo, hi, node)));
  }
  return SR_OK;
}

}  // extern "C"

namespace {

// `pods` as candidates of their own against `snap`, tags on; query i (into pods) with context list i of `pq`
// (nullptr: no contexts): every node's mask by explain_node_ctx and its shortfalls by shortfall_node, into row
// slot[i] (nullptr: i) of node_mask / node_short; status[i] the encode's.
sr_status shortfall_rows(const sr_cluster* cluster, const sr_snapshot* snap, const int32_t* pods, int32_t n,
                         const sr::PlanQueries* pq, const int32_t* slot, uint16_t* node_mask, int64_t* node_short,
                         std::vector<int32_t>* status) {
  status->assign(static_cast<size_t>(n), SR_CAND_OK);
  if (n == 0) return SR_OK;
  const size_t ns = snap->nodes.size();
  std::vector<int32_t> coff(static_cast<size_t>(n) + 1);
  for (int32_t i = 0; i <= n; ++i) coff[i] = i;
  const sr_candidates cands{n, coff.data(), pods, nullptr};
  sr::EncoderCache cache;
  cache.want_why = true;
  sr::Workload w;
  std::string err;
  sr_status st = sr::encode_workload(&cache, snap, cluster, &cands, &w, &err);
  if (st != SR_OK) return st;
  for (int32_t i = 0; i < n; ++i) (*status)[i] = w.status_host[i];
  const int32_t na = static_cast<int32_t>(w.pod_src.size());
  if (na == 0) return SR_OK;
  sr::ExplainPrograms x;
  std::vector<sr::ExplainPod> xp;
  if (!sr::build_explain(w, &x) || w.pod_cls.size() != static_cast<size_t>(na)) return SR_ERR_STATE;
  sr::explain_pods(w, &xp);
  std::vector<int32_t> slack;
  std::vector<int64_t> left;
  sr::node_slack(snap, std::max(w.n_pad, static_cast<int32_t>(ns)), &slack);
  sr::node_left(snap, std::max(w.n_pad, static_cast<int32_t>(ns)), &left);
  std::vector<sr::PlanCtxEntry> entries;  // the lists in active-pod order
  std::vector<int32_t> eoff;
  if (pq) sr::active_lists(w, *pq, &entries, &eoff);
  for (int32_t q = 0; q < na; ++q) {
    const int32_t i = w.pod_src[q] - w.pod_base;
    const size_t row = static_cast<size_t>(slot ? slot[i] : i) * ns;
    for (int32_t node = 0; node < static_cast<int32_t>(ns); ++node) {
      const sr::PlanCtxEntry* e =
          pq ? sr::find_ctx(entries.data() + eoff[q], entries.data() + eoff[q + 1], node) : nullptr;
      const uint32_t m = sr::explain_node_ctx(x, xp[q], w.atoms.data(), w.Wp, cache.node_free.data(), w.n_pad, node,
                                              slack[node], e);
      node_mask[row + node] = static_cast<uint16_t>(m);
      sr::shortfall_node(m, xp[q], cache.node_free.data(), w.n_pad, node, left[node], e,
                         node_short + (row + node) * SR_SHORT_COUNT);
    }
  }
  return SR_OK;
}

}  // namespace

extern "C" {

// sr_shortfall_pods on the host: node_mask[n][n_spot], node_short[n][n_spot][SR_SHORT_COUNT] and fallback[n] of
// `pods` against the snapshot as it is (a fallback pod: zeros), by explain_node and shortfall_node.
sr_status sr_shortfall_pods_view(const sr_cluster* cluster, const sr_snapshot* snap, const int32_t* pods, int32_t n,
                                 uint16_t* node_mask, int64_t* node_short, uint8_t* fallback) {
  if (!cluster || !snap || n < 0 || (n > 0 && !pods) || !node_mask || !node_short || !fallback)
    return SR_ERR_INVALID_ARG;
  const size_t ns = snap->nodes.size();
  std::fill_n(node_mask, static_cast<size_t>(n) * ns, uint16_t(0));
  std::fill_n(node_short, static_cast<size_t>(n) * ns * SR_SHORT_COUNT, int64_t(0));
  std::vector<int32_t> status;
  const sr_status st = shortfall_rows(cluster, snap, pods, n, nullptr, nullptr, node_mask, node_short, &status);
  if (st != SR_OK) return st;
  for (int32_t i = 0; i < n; ++i) fallback[i] = status[i] == SR_CAND_FALLBACK ? 1 : 0;
  return SR_OK;
}

// sr_shortfall_plan's batched pass on the host: how[n_cand] as sr_explain_plan_view gives it, and for the batched
// candidates node_mask[n_cand][n_spot], node_short[n_cand][n_spot][SR_SHORT_COUNT] and fallback[n_cand] in the
// context of their earlier pods (others: zeros).
sr_status sr_shortfall_plan_view(const sr_cluster* cluster, const sr_snapshot* snap, const sr_candidates* cands,
                                 const int32_t* at_pod, const int32_t* node_of_pod, uint8_t* how, uint16_t* node_mask,
                                 int64_t* node_short, uint8_t* fallback) {
  if (!cluster || !snap || !cands || !at_pod || !how || !node_mask || !node_short || !fallback) return SR_ERR_INVALID_ARG;
  sr::PlanQueries pq;
  sr_status st = sr::plan_queries(snap, cluster, cands, at_pod, node_of_pod, &pq);
  if (st != SR_OK) return st;
  const int32_t nc = cands->n_cand, nb = static_cast<int32_t>(pq.batched.size());
  const size_t ns = snap->nodes.size();
  std::copy(pq.how.begin(), pq.how.end(), how);
  std::fill_n(node_mask, static_cast<size_t>(nc) * ns, uint16_t(0));
  std::fill_n(node_short, static_cast<size_t>(nc) * ns * SR_SHORT_COUNT, int64_t(0));
  std::fill_n(fallback, nc, uint8_t(0));
  std::vector<int32_t> status;
  st = shortfall_rows(cluster, snap, pq.pods.data(), nb, &pq, pq.batched.data(), node_mask, node_short, &status);
  if (st != SR_OK) return st;
  for (int32_t i = 0; i < nb; ++i) {
    if (status[i] != SR_CAND_FALLBACK) continue;
    if (nb > 1) how[pq.batched[i]] = SR_EXPLAIN_SINGLE;
    else fallback[pq.batched[i]] = 1;
  }
  return SR_OK;
}

}  // extern "C"

namespace {

// `pods` as shortfall_rows takes them: every judged query folded into every node's row by node_view_fold (the
// statement the kernels of csrc/node_view.hip follow), the rows through the device's column-major layout
// (node_view_store) and back into `out` by node_view_unpack, as the planner unpacks the downloaded totals.
sr_status node_view_rows(const sr_cluster* cluster, const sr_snapshot* snap, const int32_t* pods, int32_t n,
                         const sr::PlanQueries* pq, const int32_t* slot, sr_node_view_out* out,
                         std::vector<int32_t>* status) {
  const size_t ns = snap->nodes.size();
  sr::node_view_clear(out, ns);
  std::vector<uint16_t> masks(static_cast<size_t>(n) * ns);
  std::vector<int64_t> shorts(static_cast<size_t>(n) * ns * SR_SHORT_COUNT);
  const sr_status st = shortfall_rows(cluster, snap, pods, n, pq, nullptr, masks.data(), shorts.data(), status);
  if (st != SR_OK) return st;
  std::vector<sr::NodeViewRow> rows(ns);
  int32_t judged = 0;
  for (int32_t i = 0; i < n; ++i) {
    if ((*status)[i] == SR_CAND_FALLBACK) continue;
    ++judged;
    for (size_t node = 0; node < ns; ++node)
      sr::node_view_fold(masks[i * ns + node], shorts.data() + (i * ns + node) * SR_SHORT_COUNT, slot ? slot[i] : i,
                         &rows[node]);
  }
  const size_t stride = static_cast<size_t>(sr::node_view_stride(static_cast<int32_t>(ns)));
  const sr::NodeViewLayout l = sr::node_view_layout(stride, 1);
  std::vector<uint64_t> image(l.bytes / 8);
  char* base = reinterpret_cast<char*>(image.data());
  for (size_t node = 0; node < ns; ++node)
    sr::node_view_store(rows[node], reinterpret_cast<uint64_t*>(base + l.min), reinterpret_cast<int32_t*>(base + l.cnt),
                        reinterpret_cast<int32_t*>(base + l.at), stride, node);
  sr::node_view_unpack(base, stride, ns, out);
  *out->judged = judged;
  return SR_OK;
}

bool node_view_out_ok(const sr_node_view_out* o) {
  return o && o->judged && o->admits && o->near && o->refuses && o->sole && o->sole_min && o->sole_at && o->fallback;
}

}  // namespace

extern "C" {

// sr_node_view_pods on the host: every array of `out` (fallback [n] included) for `pods` against the snapshot
// as it is.
sr_status sr_node_view_pods_view(const sr_cluster* cluster, const sr_snapshot* snap, const int32_t* pods, int32_t n,
                                 sr_node_view_out* out) {
  if (!cluster || !snap || n < 0 || (n > 0 && !pods) || !node_view_out_ok(out)) return SR_ERR_INVALID_ARG;
  std::vector<int32_t> status;
  const sr_status st = node_view_rows(cluster, snap, pods, n, nullptr, nullptr, out, &status);
  if (st != SR_OK) return st;
  for (int32_t i = 0; i < n; ++i) out->fallback[i] = status[i] == SR_CAND_FALLBACK ? 1 : 0;
  return SR_OK;
}

// sr_node_view_plan's batched pass on the host: how[n_cand] as sr_explain_plan_view gives it, and `out` over the
// batched candidates alone, each in the context of its earlier pods, its slot the candidate (a candidate that goes
// the SINGLE way is not evaluated by the view and counted nowhere).
sr_status sr_node_view_plan_view(const sr_cluster* cluster, const sr_snapshot* snap, const sr_candidates* cands,
                                 const int32_t* at_pod, const int32_t* node_of_pod, uint8_t* how, sr_node_view_out* out) {
  if (!cluster || !snap || !cands || !at_pod || !how || !node_view_out_ok(out)) return SR_ERR_INVALID_ARG;
  sr::PlanQueries pq;
  sr_status st = sr::plan_queries(snap, cluster, cands, at_pod, node_of_pod, &pq);
  if (st != SR_OK) return st;
  const int32_t nc = cands->n_cand, nb = static_cast<int32_t>(pq.batched.size());
  std::copy(pq.how.begin(), pq.how.end(), how);
  std::fill_n(out->fallback, nc, uint8_t(0));
  std::vector<int32_t> status;
  st = node_view_rows(cluster, snap, pq.pods.data(), nb, &pq, pq.batched.data(), out, &status);
  if (st != SR_OK) return st;
  for (int32_t i = 0; i < nb; ++i) {
    if (status[i] != SR_CAND_FALLBACK) continue;
    if (nb > 1) how[pq.batched[i]] = SR_EXPLAIN_SINGLE;
    else out->fallback[pq.batched[i]] = 1;
  }
  return SR_OK;
}

}  // extern "C"

namespace {

// One SINGLE candidate of sr_blockers_plan on the host: the contract's loop, every pod encoded alone against the
// forked snapshot and judged by explain_node on every node.
sr_status blockers_single_view(const sr_cluster* cluster, sr_snapshot* snap, const sr_candidates* cands, int32_t c,
                               sr_blockers_out* out) {
  const int32_t* off = cands->cand_pod_off;
  const int32_t* pods = cands->cand_pods + off[c];
  const int32_t np = off[c + 1] - off[c], ns = static_cast<int32_t>(snap->nodes.size());
  const size_t p0 = static_cast<size_t>(off[c] - off[0]);
  sr_status st = sr_snapshot_fork(snap);
  if (st != SR_OK) return st;
  int32_t blockers = 0, first = -1;
  bool fallback = false;
  for (int32_t k = 0; k < np && st == SR_OK && !fallback; ++k) {
    const int32_t one_off[2] = {0, 1};
    const sr_candidates one{1, one_off, pods + k, nullptr};
    sr::EncoderCache cache;
    cache.want_why = true;
    sr::Workload w;
    std::string err;
    sr::ExplainPrograms x;
    std::vector<sr::ExplainPod> xp;
    st = sr::encode_workload(&cache, snap, cluster, &one, &w, &err);
    if (st != SR_OK) break;
    if (w.status_host[0] == SR_CAND_FALLBACK) {
      fallback = true;
      break;
    }
    if (w.pod_src.size() != 1 || !sr::build_explain(w, &x)) {
      st = SR_ERR_STATE;
      break;
    }
    sr::explain_pods(w, &xp);
    int32_t at = -1, row[SR_WHY_COUNT] = {0};
    for (int32_t node = 0; node < ns; ++node) {
      const uint32_t m = sr::explain_node(x, xp[0], w.atoms.data(), w.Wp, cache.node_free.data(), w.n_pad, node);
      if (m == 0 && at < 0) at = node;
      for (int r = 0; r < SR_WHY_COUNT; ++r) row[r] += m >> r & 1;
    }
    out->node_of_pod[p0 + k] = at;
    if (at >= 0) {
      sr::snapshot_add_pod(snap, cluster, pods[k], at);
      continue;
    }
    ++blockers;
    if (first < 0) first = k;
    if (out->counts) std::copy_n(row, SR_WHY_COUNT, out->counts + (p0 + k) * SR_WHY_COUNT);
  }
  const sr_status rv = sr_snapshot_revert(snap);
  if (st != SR_OK || rv != SR_OK) return st != SR_OK ? st : rv;
  if (fallback) {
    sr::blockers_clear(cands, c, 1, out);
  } else {
    out->blockers[c] = blockers;
    out->first[c] = first;
  }
  return SR_OK;
}

}  // namespace

extern "C" {

// sr_blockers_plan on the host, every output as the planner writes it: the ways (blockers_ways), the batched
// pass through BlockersStage on heap blocks with blockers_candidate -- the statement the kernel follows -- in
// the kernel's place, and the SINGLE candidates by the loop above.  The snapshot is forked and reverted.
sr_status sr_blockers_plan_view(const sr_cluster* cluster, sr_snapshot* snap, const sr_candidates* cands,
                                const int32_t* ask, sr_blockers_out* out, uint8_t* how) {
  if (!cluster || !snap || !cands || cands->n_cand < 0 || !out || !out->blockers || !out->first || !how)
    return SR_ERR_INVALID_ARG;
  const int32_t nc = cands->n_cand;
  if (nc == 0) return SR_OK;
  if (!cands->cand_pod_off || !ask || !out->node_of_pod) return SR_ERR_INVALID_ARG;
  if (snap->forked) return SR_ERR_STATE;
  sr::BlockerWays ways;
  sr_status st = sr::blockers_ways(snap, cluster, cands, ask, &ways);
  if (st != SR_OK) return st;
  for (int32_t c = 0; c < nc; ++c) sr::blockers_clear(cands, c, 0, out);
  std::vector<int32_t> flat;
  sr::blockers_flat(cands, ways, &flat);
  if (flat.empty()) {
    for (int32_t c : ways.batched) out->blockers[c] = 0;
  } else {
    const int32_t n = static_cast<int32_t>(flat.size());
    std::vector<int32_t> off(static_cast<size_t>(n) + 1);
    for (int32_t i = 0; i <= n; ++i) off[i] = i;
    const sr_candidates singles{n, off.data(), flat.data(), nullptr};
    sr::EncoderCache cache;
    cache.want_why = true;
    sr::Workload w;
    std::string err;
    st = sr::encode_workload(&cache, snap, cluster, &singles, &w, &err);
    if (st != SR_OK) return st;
    sr::BlockersStage x;
    st = x.plan(w, cache.node_free, snap, cluster, cands, &ways, out->counts != nullptr, &err);
    if (st != SR_OK) return st;
    if (x.n_cand() > 0) {
      std::vector<uint64_t> in(x.at().in_bytes / 8 + 1), dev(x.at().out_bytes / 8 + 1, 0xA5A5A5A5A5A5A5A5ull);
      x.pack(reinterpret_cast<char*>(in.data()));
      std::fill_n(reinterpret_cast<char*>(dev.data()), x.at().zero_bytes, 0);
      sr::BlockersArgs b;
      x.args(reinterpret_cast<const char*>(in.data()), reinterpret_cast<char*>(dev.data()), &b);
      std::vector<int32_t> slack;
      sr::node_slack(snap, b.x.n_pad, &slack);
      for (int32_t c = 0; c < b.n_cand; ++c) {
        const int32_t p0 = b.cand_off[c];
        b.blockers[c] = sr::blockers_candidate(x.programs(), b.pods + p0, b.cand_off[c + 1] - p0, b.x.atoms, b.x.Wp,
                                               b.x.node_free, b.x.n_pad, b.x.n_spot, slack.data(), b.node_of_pod + p0,
                                               b.counts ? b.counts + static_cast<size_t>(p0) * SR_WHY_COUNT : nullptr,
                                               b.first + c);
      }
      x.unpack(reinterpret_cast<const char*>(dev.data()), cands, out);
    }
  }
  for (int32_t c = 0; c < nc; ++c) {
    if (ways.how[c] != SR_EXPLAIN_SINGLE) continue;
    st = blockers_single_view(cluster, snap, cands, c, out);
    if (st != SR_OK) return st;
  }
  std::copy(ways.how.begin(), ways.how.end(), how);
  return SR_OK;
}

}  // extern "C"
