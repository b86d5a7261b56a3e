// blockers.cpp — the ways, the host statement and the staging of sr_blockers_plan.
#include "blockers.hpp"

#include <algorithm>
#include <cstring>

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

namespace {

size_t up8(size_t b) { return (b + 7) & ~size_t(7); }

}  // namespace

sr_status BlockersStage::plan(const Workload& w, const std::vector<int64_t>& node_free, const sr_snapshot* snap,
                              const sr_cluster* c, const sr_candidates* cands, BlockerWays* ways, bool want_counts,
                              std::string* err) {
  const size_t na = w.pod_src.size(), n_pad = static_cast<size_t>(w.n_pad);
  if (!build_explain(w, &prog_) || w.pod_cls.size() != na || w.n_pad != w.Wp * 64 || node_free.size() < 3 * n_pad) {
    *err = "blockers: the encoder left no reasons";
    return SR_ERR_STATE;
  }
  for (int32_t op : prog_.ops)  // what the kernel indexes with
    if ((op >> 8) < 0 || (op >> 8) >= w.n_atoms || (op >> 3 & 31) >= SR_WHY_COUNT || (op & 7) > X_ALL) {
      *err = "blockers: malformed program";
      return SR_ERR_STATE;
    }
  std::vector<ExplainPod> xp;
  explain_pods(w, &xp);
  const int32_t* off = cands->cand_pod_off;
  size_t flat = 0;
  for (int32_t b : ways->batched) flat += static_cast<size_t>(off[b + 1] - off[b]);
  if (w.status_host.size() != flat) {
    *err = "blockers: the encode is not of the batched candidates' pods";
    return SR_ERR_STATE;
  }
  std::vector<int32_t> active(flat, -1);  // flat pod -> active pod
  for (size_t q = 0; q < na; ++q) {
    const int32_t i = w.pod_src[q] - w.pod_base;
    if (i < 0 || static_cast<size_t>(i) >= flat || xp[q].cls < 0 || xp[q].cls >= w.n_classes) {
      *err = "blockers: pod source or class out of range";
      return SR_ERR_STATE;
    }
    active[i] = static_cast<int32_t>(q);
  }
  pods_.clear();
  kept_.clear();
  coff_.assign(1, 0);
  size_t f0 = 0;
  for (int32_t b : ways->batched) {
    const size_t np = static_cast<size_t>(off[b + 1] - off[b]);
    bool keep = np <= static_cast<size_t>(kBlockersCtx);
    for (size_t k = 0; k < np; ++k) keep = keep && active[f0 + k] >= 0 && w.status_host[f0 + k] != SR_CAND_FALLBACK;
    if (keep) {
      for (size_t k = 0; k < np; ++k) {
        BlockerPod bp;
        bp.p = xp[active[f0 + k]];
        for (int d = 0; d < 3; ++d) bp.acc[d] = pod_acc(c, cands->cand_pods[off[b] + k], d);
        pods_.push_back(bp);
      }
      kept_.push_back(b);
      coff_.push_back(static_cast<int32_t>(pods_.size()));
    } else {
      ways->how[b] = SR_EXPLAIN_SINGLE;
    }
    f0 += np;
  }
  node_left(snap, w.n_pad, &left_);
  w_ = &w;
  free_ = node_free.data();
  counts_ = want_counts;
  const size_t np = pods_.size(), nk = kept_.size();
  at_ = BlockersLayout{};
  at_.atoms = 0;
  at_.free = up8(at_.atoms + w.atoms.size() * 8);
  at_.xoff = up8(at_.free + 3 * n_pad * 8);
  at_.xops = up8(at_.xoff + prog_.off.size() * 4);
  at_.pods = up8(at_.xops + prog_.ops.size() * 4);
  at_.coff = up8(at_.pods + np * sizeof(BlockerPod));
  at_.left = up8(at_.coff + coff_.size() * 4);
  at_.in_bytes = up8(at_.left + left_.size() * 8);
  at_.counts = 0;
  at_.zero_bytes = counts_ ? np * SR_WHY_COUNT * 4 : 0;
  at_.node_of_pod = up8(at_.zero_bytes);
  at_.blockers = up8(at_.node_of_pod + np * 4);
  at_.first = up8(at_.blockers + nk * 4);
  at_.out_bytes = up8(at_.first + nk * 4);
  return SR_OK;
}

void BlockersStage::pack(char* in) const {
  auto put = [&](size_t at, const void* src, size_t bytes) {
    if (bytes) std::memcpy(in + at, src, bytes);
  };
  put(at_.atoms, w_->atoms.data(), w_->atoms.size() * 8);
  put(at_.free, free_, 3 * static_cast<size_t>(w_->n_pad) * 8);
  put(at_.xoff, prog_.off.data(), prog_.off.size() * 4);
  put(at_.xops, prog_.ops.data(), prog_.ops.size() * 4);
  put(at_.pods, pods_.data(), pods_.size() * sizeof(BlockerPod));
  put(at_.coff, coff_.data(), coff_.size() * 4);
  put(at_.left, left_.data(), left_.size() * 8);
}

void BlockersStage::args(const char* in, char* out, BlockersArgs* a) const {
  *a = BlockersArgs{};
  a->x.n_spot = w_->n_spot;
  a->x.n_pad = w_->n_pad;
  a->x.Wp = w_->Wp;
  a->x.n_pods = n_pods();
  a->x.atoms = reinterpret_cast<const uint64_t*>(in + at_.atoms);
  a->x.node_free = reinterpret_cast<const int64_t*>(in + at_.free);
  a->x.xoff = reinterpret_cast<const int32_t*>(in + at_.xoff);
  a->x.xops = reinterpret_cast<const int32_t*>(in + at_.xops);
  a->pods = reinterpret_cast<const BlockerPod*>(in + at_.pods);
  a->cand_off = reinterpret_cast<const int32_t*>(in + at_.coff);
  a->node_left = reinterpret_cast<const int64_t*>(in + at_.left);
  a->n_cand = n_cand();
  a->counts = counts_ ? reinterpret_cast<int32_t*>(out + at_.counts) : nullptr;
  a->node_of_pod = reinterpret_cast<int32_t*>(out + at_.node_of_pod);
  a->blockers = reinterpret_cast<int32_t*>(out + at_.blockers);
  a->first = reinterpret_cast<int32_t*>(out + at_.first);
}

void BlockersStage::unpack(const char* image, const sr_candidates* cands, sr_blockers_out* out) const {
  const int32_t* counts = reinterpret_cast<const int32_t*>(image + at_.counts);
  const int32_t* map = reinterpret_cast<const int32_t*>(image + at_.node_of_pod);
  const int32_t* blockers = reinterpret_cast<const int32_t*>(image + at_.blockers);
  const int32_t* first = reinterpret_cast<const int32_t*>(image + at_.first);
  const int32_t* off = cands->cand_pod_off;
  for (size_t j = 0; j < kept_.size(); ++j) {
    const int32_t c = kept_[j];
    const size_t p0 = static_cast<size_t>(off[c] - off[0]), k0 = static_cast<size_t>(coff_[j]);
    const size_t np = static_cast<size_t>(coff_[j + 1] - coff_[j]);
    out->blockers[c] = blockers[j];
    out->first[c] = first[j];
    std::copy_n(map + k0, np, out->node_of_pod + p0);
    if (counts_ && out->counts) std::copy_n(counts + k0 * SR_WHY_COUNT, np * SR_WHY_COUNT, out->counts + p0 * SR_WHY_COUNT);
    if (out->fallback) out->fallback[c] = 0;
  }
}

}  // namespace sr
