// blockers.cpp — the ways, the host statement and the staging of sr_blockers_plan.
#include "blockers.hpp"

#include <algorithm>
#include "host.hpp"

namespace sr {

sr_status blockers_ways(const sr_snapshot* snap, const sr_cluster* c, const sr_candidates* cands, const int32_t* ask,
                        BlockerWays* out) {
  const int32_t nc = cands->n_cand;
  const int32_t* off = cands->cand_pod_off;
  for (int32_t i = 0; i < nc; ++i) {
    if (off[i + 1] < off[i]) return SR_ERR_INVALID_ARG;
    if (ask[i] < 0) continue;
    for (int32_t j = off[i]; j < off[i + 1]; ++j)
      if (cands->cand_pods[j] < 0 || cands->cand_pods[j] >= c->pods.n) return SR_ERR_INVALID_ARG;
  }
  // the largest requested value of any spot node: wherever the pods land, Requested stays below it plus
  // their total acc
  int64_t top[3] = {0, 0, 0};
  for (const NodeState& st : snap->state)
    for (int d = 0; d < 3; ++d) top[d] = std::max(top[d], st.requested[d]);
  out->how.assign(static_cast<size_t>(nc), SR_EXPLAIN_NONE);
  out->batched.clear();
  for (int32_t i = 0; i < nc; ++i) {
    if (ask[i] < 0) continue;
    const int32_t np = off[i + 1] - off[i];
    const int32_t* pods = cands->cand_pods + off[i];
    bool plain = np <= kBlockersCtx;
    int32_t ports = 0, scalars = 0;
    int64_t sum[3] = {top[0], top[1], top[2]};
    for (int32_t k = 0; k < np && plain; ++k) {
      const PodTraits t = pod_traits(c, pods[k]);
      ports += t.ports;
      scalars += t.scalars;
      if (t.anti || (k > 0 && (t.terms || t.spread)) || ports > 1 || scalars > 1) plain = false;
      for (int d = 0; d < 3 && plain; ++d) {
        const int64_t a = pod_acc(c, pods[k], d);
        if (a < 0 || __builtin_add_overflow(sum[d], a, &sum[d]) || sum[d] >= kQuantityEnd) plain = false;
      }
    }
    out->how[i] = plain ? SR_EXPLAIN_BATCHED : SR_EXPLAIN_SINGLE;
    if (plain) out->batched.push_back(i);
  }
  return SR_OK;
}

void blockers_flat(const sr_candidates* cands, const BlockerWays& ways, std::vector<int32_t>* pods) {
  pods->clear();
  const int32_t* off = cands->cand_pod_off;
  for (int32_t c : ways.batched) pods->insert(pods->end(), cands->cand_pods + off[c], cands->cand_pods + off[c + 1]);
}

int32_t blockers_candidate(const ExplainPrograms& x, const BlockerPod* pods, int32_t n, const uint64_t* atoms, int32_t Wp,
                           const int64_t* node_free, int32_t n_pad, int32_t n_spot, const int32_t* slack,
                           int32_t* node_of_pod, int32_t* counts, int32_t* first) {
  std::vector<PlanCtxEntry> list;  // the candidate's own placements, sorted by node
  std::vector<uint32_t> masks(static_cast<size_t>(n_spot));
  int32_t blockers = 0;
  *first = -1;
  for (int32_t k = 0; k < n; ++k) {
    int32_t at = -1;
    for (int32_t node = 0; node < n_spot && at < 0; ++node) {
      const PlanCtxEntry* e = find_ctx(list.data(), list.data() + list.size(), node);
      masks[node] = explain_node_ctx(x, pods[k].p, atoms, Wp, node_free, n_pad, node, slack[node], e);
      if (masks[node] == 0) at = node;
    }
    node_of_pod[k] = at;
    if (at < 0) {  // every node was judged: masks is the blocker's row
      ++blockers;
      if (*first < 0) *first = k;
      if (counts)
        for (int r = 0; r < SR_WHY_COUNT; ++r) {
          int32_t v = 0;
          for (uint32_t m : masks) v += m >> r & 1;
          counts[static_cast<size_t>(k) * SR_WHY_COUNT + r] = v;
        }
      continue;
    }
    auto it = std::lower_bound(list.begin(), list.end(), at, [](const PlanCtxEntry& e, int32_t v) { return e.node < v; });
    if (it == list.end() || it->node != at) it = list.insert(it, PlanCtxEntry{at, 0, {0, 0, 0}});
    it->pods += 1;
    for (int d = 0; d < 3; ++d) it->acc[d] += pods[k].acc[d];
  }
  return blockers;
}

void blockers_clear(const sr_candidates* cands, int32_t c, uint8_t fallback, sr_blockers_out* out) {
  const int32_t* off = cands->cand_pod_off;
  const size_t p0 = static_cast<size_t>(off[c] - off[0]), np = static_cast<size_t>(off[c + 1] - off[c]);
  out->blockers[c] = out->first[c] = -1;
  std::fill_n(out->node_of_pod + p0, np, -1);
  if (out->counts) std::fill_n(out->counts + p0 * SR_WHY_COUNT, np * SR_WHY_COUNT, 0);
  if (out->fallback) out->fallback[c] = fallback;
}

void GroupStage::pack(char* in) const { pack_parts(in, at_.in, src_, at_.n_in); }

sr_status GroupStage::check(const char* who, const Workload& w, const std::vector<int64_t>& node_free, bool more_ok,
                            std::string* err) {
  at_ = GroupLayout{};
  w_ = &w;
  return stage_workload(who, w, node_free, more_ok, &prog_, at_.in, src_, err);
}

sr_status GroupStage::plan_groups(const std::string& who, const char* what_pods, const sr_cluster* c,
                                  const sr_candidates* groups, const std::vector<int32_t>& ids, size_t pod_cap,
                                  std::vector<int32_t>* dropped, std::string* err) {
  const Workload& w = *w_;
  const size_t na = w.pod_src.size();
  std::vector<ExplainPod> xp;
  explain_pods(w, &xp);
  const int32_t* off = groups->cand_pod_off;
  size_t flat = 0;
  for (int32_t g : ids) flat += static_cast<size_t>(off[g + 1] - off[g]);
  if (w.status_host.size() != flat) {
    *err = who + ": the encode is not of " + what_pods;
    return SR_ERR_STATE;
  }
  std::vector<int32_t> active(flat, -1);  // flat pod -> active pod
  for (size_t q = 0; q < na; ++q) {
    const int32_t i = w.pod_src[q] - w.pod_base;
    if (i < 0 || static_cast<size_t>(i) >= flat || xp[q].cls < 0 || xp[q].cls >= w.n_classes) {
      *err = who + ": pod source or class out of range";
      return SR_ERR_STATE;
    }
    active[i] = static_cast<int32_t>(q);
  }
  pods_.clear();
  kept_.clear();
  goff_.assign(1, 0);
  size_t f0 = 0;
  for (int32_t g : ids) {
    const size_t np = static_cast<size_t>(off[g + 1] - off[g]);
    bool keep = np <= pod_cap;
    for (size_t k = 0; k < np; ++k) keep = keep && active[f0 + k] >= 0 && w.status_host[f0 + k] != SR_CAND_FALLBACK;
    if (keep) {
      for (size_t k = 0; k < np; ++k) {
        BlockerPod bp;
        bp.p = xp[active[f0 + k]];
        for (int d = 0; d < 3; ++d) bp.acc[d] = pod_acc(c, groups->cand_pods[off[g] + k], d);
        pods_.push_back(bp);
      }
      kept_.push_back(g);
      goff_.push_back(static_cast<int32_t>(pods_.size()));
    } else {
      dropped->push_back(g);
    }
    f0 += np;
  }
  part_of(&at_.in[IN_PODS], &src_[IN_PODS], pods_.data(), pods_.size());
  part_of(&at_.in[GIN_OFF], &src_[GIN_OFF], goff_.data(), goff_.size());
  return SR_OK;
}

void GroupStage::lay_out(const sr_snapshot* snap, int n_in, bool want_counts) {
  node_left(snap, w_->n_pad, &left_);
  counts_ = want_counts;
  at_.n_in = n_in;
  part_of(&at_.in[n_in - 1], &src_[n_in - 1], left_.data(), left_.size());
  at_.in_bytes = up8(place(at_.in, n_in));
  const size_t np = pods_.size(), nk = kept_.size();
  part_of<int32_t>(&at_.out[GOUT_COUNTS], nullptr, nullptr, counts_ ? np * SR_WHY_COUNT : 0);
  part_of<int32_t>(&at_.out[GOUT_NODE_OF_POD], nullptr, nullptr, np);
  part_of<int32_t>(&at_.out[GOUT_COUNT], nullptr, nullptr, nk);
  part_of<int32_t>(&at_.out[GOUT_FIRST], nullptr, nullptr, nk);
  at_.out_bytes = up8(place(at_.out, GOUT_PARTS));
  at_.zero_bytes = at_.out[GOUT_COUNTS].bytes;
}

void GroupStage::in_args(const char* in, ExplainArgs* x, const BlockerPod** pods, const int32_t** off,
                         const int64_t** left) const {
  stage_args(*w_, n_pods(), in, at_.in, x);
  *pods = at_part<BlockerPod>(in, at_.in[IN_PODS]);
  *off = at_part<int32_t>(in, at_.in[GIN_OFF]);
  *left = at_part<int64_t>(in, at_.in[at_.n_in - 1]);
}

void GroupStage::out_args(char* out, int32_t** counts, int32_t** node_of_pod, int32_t** count, int32_t** first) const {
  *counts = counts_ ? at_part<int32_t>(out, at_.out[GOUT_COUNTS]) : nullptr;
  *node_of_pod = at_part<int32_t>(out, at_.out[GOUT_NODE_OF_POD]);
  *count = at_part<int32_t>(out, at_.out[GOUT_COUNT]);
  *first = at_part<int32_t>(out, at_.out[GOUT_FIRST]);
}

void GroupStage::unpack_groups(const char* image, const sr_candidates* groups, const GroupResults& r) const {
  const int32_t* counts = at_part<int32_t>(image, at_.out[GOUT_COUNTS]);
  const int32_t* map = at_part<int32_t>(image, at_.out[GOUT_NODE_OF_POD]);
  const int32_t* count = at_part<int32_t>(image, at_.out[GOUT_COUNT]);
  const int32_t* first = at_part<int32_t>(image, at_.out[GOUT_FIRST]);
  const int32_t* off = groups->cand_pod_off;
  for (size_t j = 0; j < kept_.size(); ++j) {
    const int32_t g = kept_[j];
    const size_t p0 = static_cast<size_t>(off[g] - off[0]), k0 = static_cast<size_t>(goff_[j]);
    const size_t np = static_cast<size_t>(goff_[j + 1] - goff_[j]);
    r.count[g] = count[j];
    r.first[g] = first[j];
    if (np) std::copy_n(map + k0, np, r.node_of_pod + p0);
    if (counts_ && r.counts && np) std::copy_n(counts + k0 * SR_WHY_COUNT, np * SR_WHY_COUNT, r.counts + p0 * SR_WHY_COUNT);
    if (r.mark) r.mark[g] = r.marked;
  }
}

sr_status BlockersStage::plan(const Workload& w, const std::vector<int64_t>& node_free, const sr_snapshot* snap,
                              const sr_cluster* c, const sr_candidates* cands, BlockerWays* ways, bool want_counts,
                              std::string* err) {
  sr_status st = check("blockers", w, node_free, true, err);
  if (st != SR_OK) return st;
  std::vector<int32_t> left;  // the candidates that leave the batch
  st = plan_groups("blockers", "the batched candidates' pods", c, cands, ways->batched, kBlockersCtx, &left, err);
  if (st != SR_OK) return st;
  for (int32_t b : left) ways->how[b] = SR_EXPLAIN_SINGLE;
  lay_out(snap, BIN_PARTS, want_counts);
  return SR_OK;
}

void BlockersStage::args(const char* in, char* out, BlockersArgs* a) const {
  *a = BlockersArgs{};
  in_args(in, &a->x, &a->pods, &a->cand_off, &a->node_left);
  a->n_cand = n_cand();
  out_args(out, &a->counts, &a->node_of_pod, &a->blockers, &a->first);
}

void BlockersStage::unpack(const char* image, const sr_candidates* cands, sr_blockers_out* out) const {
  unpack_groups(image, cands, GroupResults{out->blockers, out->first, out->node_of_pod, out->counts, out->fallback, 0});
}

}  // namespace sr
