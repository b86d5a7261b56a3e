// explain_plan.cpp — plain contexts of sr_explain_plan and their host evaluation.
#include "explain_plan.hpp"

#include <algorithm>

#include "host.hpp"

namespace sr {

PodTraits pod_traits(const sr_cluster* c, int32_t pod) {
  PodTraits t;
  t.ports = has_ports(c, pod);
  t.scalars = has_scalars(c, pod) || att_count(c, pod) > 0;
  t.anti = has_anti_terms(c, pod);
  const sr_pod_affinity* A = c->pod_affinity;
  t.terms = t.anti || (A && A->aff_off && A->aff_off[pod + 1] > A->aff_off[pod]);
  t.spread = has_spread(c, pod);
  return t;
}

sr_status plan_queries(const sr_snapshot* snap, const sr_cluster* c, const sr_candidates* cands, const int32_t* at_pod,
                       const int32_t* node_of_pod, PlanQueries* out) {
  const int32_t nc = cands->n_cand, n_spot = static_cast<int32_t>(snap->nodes.size());
  const int32_t* off = cands->cand_pod_off;
  for (int32_t i = 0; i < nc; ++i) {
    const int32_t k = at_pod[i], np = off[i + 1] - off[i];
    if (k < 0) continue;
    if (np < 0 || k >= np || (k > 0 && !node_of_pod)) return SR_ERR_INVALID_ARG;
    for (int32_t q = 0; q <= k; ++q) {
      const int32_t pod = cands->cand_pods[off[i] + q];
      if (pod < 0 || pod >= c->pods.n) return SR_ERR_INVALID_ARG;
      if (q < k) {
        const int32_t pos = node_of_pod[off[i] - off[0] + q];
        if (pos < 0 || pos >= n_spot) return SR_ERR_INVALID_ARG;
      }
    }
  }
  out->how.assign(static_cast<size_t>(nc), SR_EXPLAIN_NONE);
  out->batched.clear();
  out->pods.clear();
  out->off.assign(1, 0);
  out->entries.clear();
  std::vector<PlanCtxEntry> list;
  for (int32_t i = 0; i < nc; ++i) {
    const int32_t k = at_pod[i];
    if (k < 0) continue;
    const int32_t* pods = cands->cand_pods + off[i];
    const int32_t* map = node_of_pod ? node_of_pod + (off[i] - off[0]) : nullptr;
    const PodTraits stop = pod_traits(c, pods[k]);
    // with no earlier pod the context is empty whatever the stop pod carries
    bool plain = k == 0 || !(stop.terms || stop.spread);
    list.clear();
    for (int32_t q = 0; q < k && plain; ++q) {
      const PodTraits e = pod_traits(c, pods[q]);
      if ((stop.ports && e.ports) || (stop.scalars && e.scalars) || e.anti) plain = false;
      PlanCtxEntry en{map[q], 1, {0, 0, 0}};
      for (int d = 0; d < 3 && plain; ++d) {
        en.acc[d] = pod_acc(c, pods[q], d);
        if (en.acc[d] < 0) plain = false;
      }
      list.push_back(en);
    }
    if (plain && !list.empty()) {  // one entry per distinct node
      std::stable_sort(list.begin(), list.end(),
                       [](const PlanCtxEntry& a, const PlanCtxEntry& b) { return a.node < b.node; });
      size_t n = 0;
      for (size_t j = 0; j < list.size() && plain; ++j) {
        if (n > 0 && list[n - 1].node == list[j].node) {
          PlanCtxEntry& m = list[n - 1];
          m.pods += 1;
          for (int d = 0; d < 3; ++d)
            if (__builtin_add_overflow(m.acc[d], list[j].acc[d], &m.acc[d])) plain = false;
        } else {
          list[n++] = list[j];
        }
      }
      list.resize(n);
      // Requested after the fill must stay a quantity the encoder takes
      // (free - acc is then allocatable - it, which cannot overflow)
      for (size_t j = 0; j < list.size() && plain; ++j) {
        const NodeState& st = snap->state[list[j].node];
        for (int d = 0; d < 3; ++d) {
          int64_t r;
          if (__builtin_add_overflow(st.requested[d], list[j].acc[d], &r) || r < 0 || r >= kQuantityEnd) plain = false;
        }
      }
    }
    if (!plain) {
      out->how[i] = SR_EXPLAIN_SINGLE;
      continue;
    }
    out->how[i] = SR_EXPLAIN_BATCHED;
    out->batched.push_back(i);
    out->pods.push_back(pods[k]);
    out->entries.insert(out->entries.end(), list.begin(), list.end());
    out->off.push_back(static_cast<int32_t>(out->entries.size()));
  }
  return SR_OK;
}

void node_slack(const sr_snapshot* snap, int32_t n_pad, std::vector<int32_t>* out) {
  out->assign(static_cast<size_t>(n_pad), 0);
  const size_t n = std::min(snap->nodes.size(), static_cast<size_t>(n_pad));
  for (size_t i = 0; i < n; ++i) {
    const int64_t left = snap->nodes[i].alloc_pods - snap->state[i].npods;
    (*out)[i] = static_cast<int32_t>(std::max<int64_t>(-(1 << 30), std::min<int64_t>(left, 1 << 30)));
  }
}

void node_left(const sr_snapshot* snap, int32_t n_pad, std::vector<int64_t>* out) {
  out->assign(static_cast<size_t>(n_pad), 0);
  const size_t n = std::min(snap->nodes.size(), static_cast<size_t>(n_pad));
  for (size_t i = 0; i < n; ++i) {
    int64_t left;
    if (__builtin_sub_overflow(snap->nodes[i].alloc_pods, snap->state[i].npods, &left))
      left = snap->nodes[i].alloc_pods < 0 ? INT64_MIN : INT64_MAX;
    (*out)[i] = left;
  }
}

void shortfall_node(uint32_t mask, const ExplainPod& p, const int64_t* node_free, int32_t n_pad, int32_t node,
                    int64_t left, const PlanCtxEntry* e, int64_t out[SR_SHORT_COUNT]) {
  for (int d = 0; d < 3; ++d) {
    const int64_t free = node_free[static_cast<size_t>(d) * n_pad + node] - (e ? e->acc[d] : 0);
    out[SR_SHORT_CPU + d] = (mask >> (WHY_CPU + d) & 1) ? p.req[d] - free : 0;
  }
  // the bit says left - earlier < 1, so 1 + earlier - left lies in [1, 2^63 + 2^31]: exact in 64 unsigned bits
  const uint64_t u = uint64_t(1) + static_cast<uint64_t>(e ? e->pods : 0) - static_cast<uint64_t>(left);
  out[SR_SHORT_PODS] = (mask >> WHY_PODS & 1) ? static_cast<int64_t>(std::min<uint64_t>(u, INT64_MAX)) : 0;
}

const PlanCtxEntry* find_ctx(const PlanCtxEntry* lo, const PlanCtxEntry* hi, int32_t node) {
  const PlanCtxEntry* it =
      std::lower_bound(lo, hi, node, [](const PlanCtxEntry& e, int32_t v) { return e.node < v; });
  return it != hi && it->node == node ? it : nullptr;
}

uint32_t explain_node_ctx(const ExplainPrograms& x, const ExplainPod& p, const uint64_t* atoms, int32_t Wp,
                          const int64_t* node_free, int32_t n_pad, int32_t node, int32_t slack, const PlanCtxEntry* e) {
  uint32_t mask = explain_node(x, p, atoms, Wp, node_free, n_pad, node);
  if (!e) return mask;
  bool pods_judged = false;
  for (int32_t i = x.off[p.cls]; i < x.off[p.cls + 1]; ++i)
    pods_judged = pods_judged || x.ops[i] == x_op(0, WHY_PODS, X_AND);
  if (pods_judged) mask = (mask & ~(1u << WHY_PODS)) | (slack - e->pods < 1 ? 1u << WHY_PODS : 0u);
  if (p.resources)
    for (int d = 0; d < 3; ++d) {
      const uint32_t bit = 1u << (WHY_CPU + d);
      mask = (mask & ~bit) | (p.req[d] > node_free[static_cast<size_t>(d) * n_pad + node] - e->acc[d] ? bit : 0u);
    }
  return mask;
}

}  // namespace sr
