// Host-only check of sr_explain_pods' encoder side (csrc/explain.hpp): on a
// synthetic config, every candidate pod as a candidate of its own, encoded
// with the reason tags on.  For every pod and spot node the explain program
// and fitsRequest's compares are evaluated on the host; the nodes refused for
// no reason must be exactly S[class] & T & T & T, evaluated from the class
// programs (the pod's class after the dead check) and the T-row thresholds as
// the workload holds them.
//   make -C k8s-spot-rescheduler_amd tools && k8s-spot-rescheduler_amd/bin/explain_check <config> [on-demand nodes] [spot nodes]
//   (SR_SYNTH_REALISTIC / SR_SYNTH_AFFINITY: the bench variants, as bin/encode_stats)
// Prints the reasons seen as `reason <NAME> <pairs>` lines.  Exit status 1: a
// pair disagrees; 2: no pod shows two different reasons on one node (the run
// proves nothing about keeping the filters apart).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../k8s-spot-rescheduler_amd/csrc/explain.hpp"
#include "../k8s-spot-rescheduler_amd/csrc/host.hpp"
#include "../k8s-spot-rescheduler_amd/csrc/synth/sr_synth.h"

namespace {

const char* kNames[SR_WHY_COUNT] = {"UNSCHEDULABLE", "TAINT",  "NODE_AFFINITY", "PODS",   "CPU",    "MEMORY",
                                    "EPHEMERAL",     "SCALAR", "PORTS",         "INTER_POD", "SPREAD", "VOLUMES"};

// S[class] for one node, from the class program as K0 reads it.
bool class_admits(const sr::Workload& w, int32_t cls, int32_t node) {
  auto bit = [&](int32_t atom) {
    return (w.atoms[static_cast<size_t>(atom) * w.Wp + (node >> 6)] >> (node & 63) & 1) != 0;
  };
  bool acc = true, in_terms = false, any = false, term = false;
  for (int32_t i = w.cls_prog_off[cls]; i < w.cls_prog_off[cls + 1]; ++i) {
    const int32_t atom = w.cls_prog[i] >> 2, kind = w.cls_prog[i] & 3;
    if (kind == sr::PROG_AND) acc = acc && bit(atom);
    else if (kind == sr::PROG_ANDNOT) acc = acc && !bit(atom);
    else if (kind == sr::PROG_TERM_START) {
      any = any || (in_terms && term);
      in_terms = true;
      term = bit(atom);
    } else term = term && bit(atom);
  }
  return acc && (!in_terms || any || term);
}

}  // namespace

int main(int argc, char** argv) {
  sr_synth_params p{};
  p.config = argc > 1 ? atoi(argv[1]) : 3;
  p.n_on_demand = argc > 2 ? atoi(argv[2]) : 0;
  p.n_spot = argc > 3 ? atoi(argv[3]) : 0;
  p.pinned_fraction = -1;
  if (std::getenv("SR_SYNTH_REALISTIC")) {
    p.stateful_fraction = 0.15;
    p.init_fraction = 0.2;
    p.gpu_fraction = 0.3;
  }
  if (std::getenv("SR_SYNTH_AFFINITY")) {
    p.anti_fraction = 0.10;
    p.spread_fraction = 0.10;
  }
  sr_synth* s = sr_synth_generate(&p);
  sr_cluster c;
  sr_synth_view(s, &c);
  sr_node_label od, sp;
  sr_synth_labels(s, &od, &sp);
  const int nn = c.nodes.n, np = c.pods.n;
  std::vector<int32_t> spot(nn), odn(nn), off(nn + 1), idx(np > 0 ? np : 1);
  std::vector<int64_t> req(nn), fr(nn);
  int32_t ns = 0, nod = 0;
  sr_node_map m{spot.data(), &ns, odn.data(), &nod, off.data(), idx.data(), req.data(), fr.data()};
  sr_node_map_params prm{od, sp, 0};
  if (sr_new_node_map(&c, &prm, &m) != SR_OK) return 3;
  sr_snapshot* snap = nullptr;
  if (sr_snapshot_create(&c, spot.data(), ns, off.data(), idx.data(), &snap) != SR_OK) return 3;
  std::vector<int32_t> cp;  // every candidate pod, each a candidate of its own
  for (int i = 0; i < nod; ++i)
    for (int j = off[odn[i]]; j < off[odn[i] + 1]; ++j)
      if (!(c.pods.flags[idx[j]] & (SR_POD_MIRROR | SR_POD_DAEMONSET_CONTROLLER))) cp.push_back(idx[j]);
  std::vector<int32_t> coff(cp.size() + 1);
  for (size_t i = 0; i <= cp.size(); ++i) coff[i] = static_cast<int32_t>(i);
  sr_candidates cands{static_cast<int32_t>(cp.size()), coff.data(), cp.data(), nullptr};
  sr::EncoderCache cache;
  cache.want_why = true;
  sr::Workload w;
  std::string err;
  if (sr::encode_workload(&cache, snap, &c, &cands, &w, &err) != SR_OK) {
    printf("encode failed: %s\n", err.c_str());
    return 3;
  }
  sr::ExplainPrograms x;
  if (!sr::build_explain(w, &x)) {
    printf("the encoder left an untagged operation\n");
    return 1;
  }
  std::vector<sr::ExplainPod> pods;
  sr::explain_pods(w, &pods);
  const int32_t na = static_cast<int32_t>(pods.size());
  printf("config %d: spot %d candidate pods %zu explained %d fallback %zu classes %d atoms %d\n", p.config, ns,
         cp.size(), na, cp.size() - static_cast<size_t>(na), w.n_classes, w.n_atoms);
  long long seen[SR_WHY_COUNT] = {0}, pairs = 0, feasible = 0, bad = 0;
  int32_t pods_two = 0;
  const int64_t* nf = cache.node_free.data();
  for (int32_t q = 0; q < na; ++q) {
    const int32_t* rows = &w.pod_rows[static_cast<size_t>(q) * 4];
    bool two = false;
    for (int32_t n = 0; n < ns; ++n) {
      const uint32_t mask = sr::explain_node(x, pods[q], w.atoms.data(), w.Wp, nf, w.n_pad, n);
      bool fits = class_admits(w, rows[0], n);
      for (int d = 0; d < 3 && fits; ++d) {
        const int32_t t = rows[1 + d];  // row 0: every node
        if (t != 0) fits = nf[static_cast<size_t>(w.t_dim[t]) * w.n_pad + n] >= w.t_thr[t];
      }
      if (fits != (mask == 0)) {
        if (bad++ < 10) printf("pod %d node %d: mask %#x but S & T & T & T says %d\n", cp[w.pod_src[q]], n, mask, fits);
      }
      for (int r = 0; r < SR_WHY_COUNT; ++r) seen[r] += mask >> r & 1;
      two = two || (mask & (mask - 1)) != 0;
      feasible += mask == 0;
      ++pairs;
    }
    pods_two += two;
  }
  printf("pairs %lld feasible %lld\n", pairs, feasible);
  for (int r = 0; r < SR_WHY_COUNT; ++r)
    if (seen[r]) printf("reason %s %lld\n", kNames[r], seen[r]);
  printf("pods with two reasons on one node: %d\n", pods_two);
  sr_snapshot_destroy(snap);
  sr_synth_destroy(s);
  if (bad) {
    printf("FAILED: %lld pairs disagree\n", bad);
    return 1;
  }
  if (pods_two == 0) {
    printf("FAILED: no pod shows two different reasons on one node\n");
    return 2;
  }
  printf("ok\n");
  return 0;
}
