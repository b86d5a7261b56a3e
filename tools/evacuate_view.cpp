// Host-only view of sr_evacuate_plan (csrc/evacuate.cpp), linked into lib/libsrexplainview.so beside
// tools/explain_plan_view.cpp so tests/test_evacuate_reference.py can prove everything but the kernel without a
// GPU: the rule (evacuate_ways), the staging of a pass through EvacuateStage on heap blocks, and
// evacuate_scenario -- the statement the kernel follows -- in the kernel's place, every output as the planner
// writes it.  The snapshot must come from this library's own sr_snapshot_create.
//   make -C k8s-spot-rescheduler_amd tools
#include <algorithm>
#include <string>
#include <vector>

#include "../k8s-spot-rescheduler_amd/csrc/evacuate.hpp"
#include "../k8s-spot-rescheduler_amd/csrc/host.hpp"

namespace {

// One pass over the scenarios `ids`, as evacuate_pass of query.cpp runs it.
sr_status view_pass(const sr_cluster* cluster, const sr_snapshot* snap, const sr_candidates* scen, const int32_t* lost_off,
                    const int32_t* lost_pos, const std::vector<int32_t>& ids, std::vector<int32_t>* fell,
                    sr_evacuate_out* out) {
  std::vector<int32_t> flat;
  sr::evacuate_flat(scen, ids, &flat);
  if (flat.empty()) {
    for (int32_t s : ids) {
      out->stranded[s] = 0;
      if (out->how) out->how[s] = SR_EVAC_JUDGED;
    }
    return SR_OK;
  }
  const int32_t n = static_cast<int32_t>(flat.size());
  std::vector<int32_t> off(static_cast<size_t>(n) + 1);
  for (int32_t i = 0; i <= n; ++i) off[i] = i;
  const sr_candidates singles{n, off.data(), flat.data(), nullptr};
  sr::EncoderCache cache;
  cache.want_why = true;
  sr::Workload w;
  std::string err;
  sr_status st = sr::encode_workload(&cache, snap, cluster, &singles, &w, &err);
  if (st != SR_OK) return st;
  sr::EvacuateStage x;
  st = x.plan(w, cache.node_free, snap, cluster, scen, lost_off, lost_pos, ids, out->counts != nullptr, fell, &err);
  if (st != SR_OK || x.n_scen() == 0) return st;
  const sr::EvacuateScratch sc = sr::evacuate_scratch(x.n_pad(), 1);
  std::vector<uint64_t> in(x.at().in_bytes / 8 + 1), dev(x.at().out_bytes / 8 + 1, 0xA5A5A5A5A5A5A5A5ull);
  std::vector<uint64_t> scratch(sc.bytes / 8 + 1, 0);
  x.pack(reinterpret_cast<char*>(in.data()));
  std::fill_n(reinterpret_cast<char*>(dev.data()), x.at().zero_bytes, 0);
  sr::EvacuateArgs b;
  x.args(reinterpret_cast<const char*>(in.data()), reinterpret_cast<char*>(dev.data()), reinterpret_cast<char*>(scratch.data()),
         1, sr::kEvacWaves, &b);
  std::vector<int32_t> slack;
  sr::node_slack(snap, b.x.n_pad, &slack);
  sr::EvacuateDeltas d;
  d.size(b.x.n_pad);
  std::vector<uint64_t> lost(static_cast<size_t>(b.x.Wp));
  for (int32_t s = 0; s < b.n_scen; ++s) {
    std::fill(lost.begin(), lost.end(), 0);
    for (int32_t j = b.lost_off[s]; j < b.lost_off[s + 1]; ++j) lost[b.lost_pos[j] >> 6] |= uint64_t(1) << (b.lost_pos[j] & 63);
    const int32_t p0 = b.scen_off[s];
    b.stranded[s] = sr::evacuate_scenario(x.programs(), b.pods + p0, b.scen_off[s + 1] - p0, b.x.atoms, b.x.Wp, b.x.node_free,
                                          b.x.n_pad, b.x.n_spot, slack.data(), lost.data(), &d, b.node_of_pod + p0,
                                          b.counts ? b.counts + static_cast<size_t>(p0) * SR_WHY_COUNT : nullptr, b.first + s);
  }
  x.unpack(reinterpret_cast<const char*>(dev.data()), scen, out);
  return SR_OK;
}

}  // namespace

extern "C" {

// sr_evacuate_plan on the host, every output as the planner writes it.  The snapshot is not modified.
sr_status sr_evacuate_plan_view(const sr_cluster* cluster, const sr_snapshot* snap, const sr_candidates* scen,
                                const int32_t* lost_off, const int32_t* lost_pos, sr_evacuate_out* out) {
  if (!cluster || !snap || !scen || scen->n_cand < 0 || !out || !out->stranded || !out->first) return SR_ERR_INVALID_ARG;
  const int32_t nc = scen->n_cand;
  if (nc == 0) return SR_OK;
  if (!scen->cand_pod_off || !lost_off) return SR_ERR_INVALID_ARG;
  const int32_t* off = scen->cand_pod_off;
  if (off[nc] < off[0] || (off[nc] > off[0] && (!scen->cand_pods || !out->node_of_pod))) return SR_ERR_INVALID_ARG;
  if (lost_off[nc] < lost_off[0] || (lost_off[nc] > lost_off[0] && !lost_pos)) return SR_ERR_INVALID_ARG;
  if (snap->forked) return SR_ERR_STATE;
  sr::EvacuateWays ways;
  sr_status st = sr::evacuate_ways(snap, cluster, scen, lost_off, lost_pos, &ways);
  if (st != SR_OK) return st;
  for (int32_t s = 0; s < nc; ++s) sr::evacuate_clear(scen, s, ways.how[s], out);
  std::vector<int32_t> fell;
  st = view_pass(cluster, snap, scen, lost_off, lost_pos, ways.judged, &fell, out);
  if (st != SR_OK) return st;
  for (int32_t s : fell) {
    std::vector<int32_t> again;
    if (ways.judged.size() > 1) {
      st = view_pass(cluster, snap, scen, lost_off, lost_pos, std::vector<int32_t>{s}, &again, out);
      if (st != SR_OK) return st;
    } else {
      again.push_back(s);
    }
    if (!again.empty()) sr::evacuate_clear(scen, s, SR_EVAC_FALLBACK, out);
  }
  return SR_OK;
}

}  // extern "C"
