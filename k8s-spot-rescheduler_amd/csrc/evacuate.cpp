// evacuate.cpp — the rule, the host statement and the staging of sr_evacuate_plan.
#include "evacuate.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "host.hpp"

namespace sr {

sr_status evacuate_ways(const sr_snapshot* snap, const sr_cluster* c, const sr_candidates* scen, const int32_t* lost_off,
                        const int32_t* lost_pos, EvacuateWays* out) {
  const int32_t nc = scen->n_cand, n_spot = static_cast<int32_t>(snap->nodes.size());
  const int32_t* off = scen->cand_pod_off;
  if (off[0] < 0 || lost_off[0] < 0) return SR_ERR_INVALID_ARG;
  for (int32_t i = 0; i < nc; ++i)
    if (off[i + 1] < off[i] || lost_off[i + 1] < lost_off[i]) return SR_ERR_INVALID_ARG;
  for (int32_t j = off[0]; j < off[nc]; ++j)
    if (scen->cand_pods[j] < 0 || scen->cand_pods[j] >= c->pods.n) return SR_ERR_INVALID_ARG;
  std::vector<int32_t> seen(static_cast<size_t>(n_spot), -1);  // the last scenario that lost the position
  for (int32_t i = 0; i < nc; ++i)
    for (int32_t j = lost_off[i]; j < lost_off[i + 1]; ++j) {
      const int32_t p = lost_pos[j];
      if (p < 0 || p >= n_spot || seen[p] == i) return SR_ERR_INVALID_ARG;
      seen[p] = i;
    }
  // the largest requested value of any spot node: wherever the pods land, Requested stays below it plus
  // their total acc (blockers_ways' bound)
  int64_t top[3] = {0, 0, 0};
  for (const NodeState& st : snap->state)
    for (int d = 0; d < 3; ++d) top[d] = std::max(top[d], st.requested[d]);
  out->how.assign(static_cast<size_t>(nc), SR_EVAC_NOT_PLAIN);
  out->judged.clear();
  for (int32_t i = 0; i < nc; ++i) {
    bool plain = true;
    // what a lost node's pods still say in the standing snapshot about SURVIVING nodes: their required
    // anti-affinity repels from their whole domain, and a pod whose scalar requests are unknown sends every pod
    // with scalars to the fallback
    for (int32_t j = lost_off[i]; j < lost_off[i + 1] && plain; ++j) {
      const NodeState& st = snap->state[lost_pos[j]];
      if (st.anti != 0 || st.scalar_unknown != 0) plain = false;
    }
    int32_t ports = 0, scalars = 0;
    int64_t sum[3] = {top[0], top[1], top[2]};
    for (int32_t k = off[i]; k < off[i + 1] && plain; ++k) {
      const int32_t pod = scen->cand_pods[k];
      const PodTraits t = pod_traits(c, pod);
      ports += t.ports;
      scalars += t.scalars;
      if (t.anti || t.terms || t.spread || ports > 1 || scalars > 1) plain = false;
      for (int d = 0; d < 3 && plain; ++d) {
        const int64_t a = pod_acc(c, pod, d);
        if (a < 0 || __builtin_add_overflow(sum[d], a, &sum[d]) || sum[d] >= kQuantityEnd) plain = false;
      }
    }
    if (plain) {
      out->how[i] = SR_EVAC_JUDGED;
      out->judged.push_back(i);
    }
  }
  return SR_OK;
}

void evacuate_flat(const sr_candidates* scen, const std::vector<int32_t>& ids, std::vector<int32_t>* pods) {
  pods->clear();
  const int32_t* off = scen->cand_pod_off;
  for (int32_t s : ids) pods->insert(pods->end(), scen->cand_pods + off[s], scen->cand_pods + off[s + 1]);
}

int32_t evacuate_scenario(const ExplainPrograms& x, const BlockerPod* pods, int32_t n, const uint64_t* atoms, int32_t Wp,
                          const int64_t* node_free, int32_t n_pad, int32_t n_spot, const int32_t* slack,
                          const uint64_t* lost, EvacuateDeltas* d, int32_t* node_of_pod, int32_t* counts, int32_t* first) {
  std::vector<uint32_t> masks(static_cast<size_t>(n_spot));
  const size_t np = static_cast<size_t>(n_pad);
  int32_t stranded = 0;
  *first = -1;
  for (int32_t k = 0; k < n; ++k) {
    int32_t at = -1;
    for (int32_t node = 0; node < n_spot && at < 0; ++node) {
      masks[node] = 0;
      if (lost[node >> 6] >> (node & 63) & 1) continue;  // never a target, in no row
      const PlanCtxEntry e{node, d->added[node], {d->used[node], d->used[np + node], d->used[2 * np + node]}};
      masks[node] = explain_node_ctx(x, pods[k].p, atoms, Wp, node_free, n_pad, node, slack[node],
                                     d->added[node] > 0 ? &e : nullptr);
      if (masks[node] == 0) at = node;
    }
    node_of_pod[k] = at;
    if (at < 0) {  // every surviving node was judged: masks is the stranded pod's row
      ++stranded;
      if (*first < 0) *first = k;
      if (counts)
        for (int r = 0; r < SR_WHY_COUNT; ++r) {
          int32_t v = 0;
          for (uint32_t m : masks) v += m >> r & 1;
          counts[static_cast<size_t>(k) * SR_WHY_COUNT + r] = v;
        }
      continue;
    }
    d->added[at] += 1;
    for (int dim = 0; dim < 3; ++dim) d->used[dim * np + at] += pods[k].acc[dim];
  }
  for (int32_t k = 0; k < n; ++k) {  // the undo log: the scenario's own mapping
    const int32_t at = node_of_pod[k];
    if (at < 0) continue;
    d->added[at] = 0;
    for (int dim = 0; dim < 3; ++dim) d->used[dim * np + at] = 0;
  }
  return stranded;
}

void evacuate_clear(const sr_candidates* scen, int32_t s, uint8_t how, sr_evacuate_out* out) {
  const int32_t* off = scen->cand_pod_off;
  const size_t p0 = static_cast<size_t>(off[s] - off[0]), np = static_cast<size_t>(off[s + 1] - off[s]);
  out->stranded[s] = out->first[s] = -1;
  if (np) std::fill_n(out->node_of_pod + p0, np, -1);
  if (out->counts && np) std::fill_n(out->counts + p0 * SR_WHY_COUNT, np * SR_WHY_COUNT, 0);
  if (out->how) out->how[s] = how;
}

EvacuateScratch evacuate_scratch(int32_t n_pad, int32_t blocks) {
  EvacuateScratch s;
  const size_t cells = static_cast<size_t>(std::max(blocks, 0)) * static_cast<size_t>(std::max(n_pad, 0));
  s.used = 0;
  s.added = 3 * cells * 8;
  s.bytes = up8(s.added + cells * 4);
  return s;
}

void evacuate_shape(int32_t n_scen, const char* grid_env, const char* waves_env, int32_t* blocks, int32_t* waves) {
  int32_t g = kEvacGrid, w = kEvacWaves;
  if (grid_env && std::atoi(grid_env) > 0) g = std::min(std::atoi(grid_env), kEvacMaxGrid);
  if (waves_env && std::atoi(waves_env) > 0) w = std::min(std::atoi(waves_env), kEvacMaxWaves);
  *blocks = std::max(1, std::min(g, n_scen));
  *waves = w;
}

sr_status EvacuateStage::plan(const Workload& w, const std::vector<int64_t>& node_free, const sr_snapshot* snap,
                              const sr_cluster* c, const sr_candidates* scen, const int32_t* lost_off,
                              const int32_t* lost_pos, const std::vector<int32_t>& ids, bool want_counts,
                              std::vector<int32_t>* fell, std::string* err) {
  const bool sizes_ok = static_cast<size_t>(w.n_spot) == snap->nodes.size() && w.n_spot <= w.n_pad;
  sr_status st = check("evacuate", w, node_free, sizes_ok, err);
  if (st != SR_OK) return st;
  if (w.Wp > kEvacMaxWp) {
    *err = "evacuate: more spot nodes than the lost set's bitmask holds";
    return SR_ERR_STATE;
  }
  st = plan_groups("evacuate", "the scenarios' pods", c, scen, ids, SIZE_MAX, fell, err);
  if (st != SR_OK) return st;
  lpos_.clear();
  loff_.assign(1, 0);
  for (int32_t s : kept_) {
    for (int32_t j = lost_off[s]; j < lost_off[s + 1]; ++j) {
      if (lost_pos[j] < 0 || lost_pos[j] >= w.n_spot) {  // (evacuate_ways checked it: the kernel sets an LDS bit with it)
        *err = "evacuate: lost position out of range";
        return SR_ERR_STATE;
      }
      lpos_.push_back(lost_pos[j]);
    }
    loff_.push_back(static_cast<int32_t>(lpos_.size()));
  }
  part_of(&at_.in[EIN_LOFF], &src_[EIN_LOFF], loff_.data(), loff_.size());
  part_of(&at_.in[EIN_LPOS], &src_[EIN_LPOS], lpos_.data(), lpos_.size());
  lay_out(snap, EIN_PARTS, want_counts);
  return SR_OK;
}

int32_t EvacuateStage::n_pad() const { return w_ ? w_->n_pad : 0; }

void EvacuateStage::args(const char* in, char* out, char* scratch, int32_t blocks, int32_t waves, EvacuateArgs* a) const {
  *a = EvacuateArgs{};
  in_args(in, &a->x, &a->pods, &a->scen_off, &a->node_left);
  a->lost_off = at_part<int32_t>(in, at_.in[EIN_LOFF]);
  a->lost_pos = at_part<int32_t>(in, at_.in[EIN_LPOS]);
  a->n_scen = n_scen();
  a->waves = waves;
  const EvacuateScratch sc = evacuate_scratch(w_->n_pad, blocks);
  a->used = reinterpret_cast<int64_t*>(scratch + sc.used);
  a->added = reinterpret_cast<int32_t*>(scratch + sc.added);
  out_args(out, &a->counts, &a->node_of_pod, &a->stranded, &a->first);
}

void EvacuateStage::unpack(const char* image, const sr_candidates* scen, sr_evacuate_out* out) const {
  unpack_groups(image, scen,
                GroupResults{out->stranded, out->first, out->node_of_pod, out->counts, out->how, SR_EVAC_JUDGED});
}

}  // namespace sr
