// Host-only check of the statements sr_shortfall_pods / sr_shortfall_plan follow (csrc/explain_plan.hpp:
// shortfall_node, node_left) together with the plan_queries path, on synthetic configs.  The candidates of a
// config are asked at their last pod, their earlier pods spread over the spot nodes by a fixed rule (several
// on one node, so entries merge); every batched query's stop pod is evaluated on every spot node by
// explain_node_ctx and shortfall_node, and every number is recomputed from the snapshot's own node state:
//   bit d set  <=>  shortfall_d >= 1, and then shortfall_d == request_d + requested_d + acc_d - allocatable_d;
//   PODS set   <=>  pods shortfall >= 1, and then == pods + earlier pods there + 1 - allowed pods.
// The same pods are asked without a context too.  Stand-alone (its own main), so it is the program to build with
// sanitizers:
//   make -C k8s-spot-rescheduler_amd bin/shortfall_check       && k8s-spot-rescheduler_amd/bin/shortfall_check
//   make -C k8s-spot-rescheduler_amd bin/shortfall_check_san   && k8s-spot-rescheduler_amd/bin/shortfall_check_san
// Exit status 1: a number disagrees; 2: no query showed a shortfall (the run proves nothing).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../k8s-spot-rescheduler_amd/csrc/explain_plan.hpp"
#include "../k8s-spot-rescheduler_amd/csrc/host.hpp"
#include "../k8s-spot-rescheduler_amd/csrc/synth/sr_synth.h"

namespace {

struct Tally {
  long long pairs = 0, with_short = 0, touched = 0, bad = 0, queries = 0;
};

// Every batched query of `pq` (stop pods `pq.pods`, contexts `pq.off` / `pq.entries`) on every spot node.
int check_queries(const sr_cluster& c, const sr_snapshot* snap, const sr::PlanQueries& pq, Tally* t) {
  const int32_t nb = static_cast<int32_t>(pq.pods.size()), ns = static_cast<int32_t>(snap->nodes.size());
  if (nb == 0) return 0;
  std::vector<int32_t> off(static_cast<size_t>(nb) + 1);
  for (int32_t i = 0; i <= nb; ++i) off[i] = i;
  const sr_candidates stops{nb, off.data(), pq.pods.data(), nullptr};
  sr::EncoderCache cache;
  cache.want_why = true;
  sr::Workload w;
  std::string err;
  if (sr::encode_workload(&cache, snap, &c, &stops, &w, &err) != SR_OK) {
    printf("encode failed: %s\n", err.c_str());
    return 3;
  }
  const int32_t na = static_cast<int32_t>(w.pod_src.size());
  if (na == 0) return 0;
  sr::ExplainPrograms x;
  std::vector<sr::ExplainPod> xp;
  if (!sr::build_explain(w, &x)) return 3;
  sr::explain_pods(w, &xp);
  std::vector<int32_t> slack;
  std::vector<int64_t> left;
  sr::node_slack(snap, w.n_pad, &slack);
  sr::node_left(snap, w.n_pad, &left);
  for (int32_t q = 0; q < na; ++q) {
    const int32_t i = w.pod_src[q] - w.pod_base;
    const sr::PlanCtxEntry *lo = pq.entries.data() + pq.off[i], *hi = pq.entries.data() + pq.off[i + 1];
    ++t->queries;
    for (int32_t n = 0; n < ns; ++n) {
      const sr::PlanCtxEntry* e = sr::find_ctx(lo, hi, n);
      const uint32_t m =
          sr::explain_node_ctx(x, xp[q], w.atoms.data(), w.Wp, cache.node_free.data(), w.n_pad, n, slack[n], e);
      int64_t sf[SR_SHORT_COUNT];
      sr::shortfall_node(m, xp[q], cache.node_free.data(), w.n_pad, n, left[n], e, sf);
      ++t->pairs;
      t->touched += e != nullptr;
      bool ok = true;
      for (int d = 0; d < 3; ++d) {
        const bool bit = (m >> (sr::WHY_CPU + d) & 1) != 0;
        const int64_t want =
            xp[q].req[d] + snap->state[n].requested[d] + (e ? e->acc[d] : 0) - snap->nodes[n].alloc[d];
        ok = ok && bit == (sf[d] >= 1) && (bit ? sf[d] == want : sf[d] == 0);
        if (xp[q].resources) ok = ok && bit == (want >= 1);
      }
      const bool pbit = (m >> sr::WHY_PODS & 1) != 0;
      const int64_t pwant = snap->state[n].npods + (e ? e->pods : 0) + 1 - snap->nodes[n].alloc_pods;
      ok = ok && pbit == (sf[SR_SHORT_PODS] >= 1) && (pbit ? sf[SR_SHORT_PODS] == pwant : sf[SR_SHORT_PODS] == 0);
      t->with_short += (sf[0] | sf[1] | sf[2] | sf[3]) != 0;
      if (!ok && t->bad++ < 10)
        printf("pod %d node %d: mask %#x shortfalls %lld %lld %lld %lld\n", pq.pods[i], n, m,
               static_cast<long long>(sf[0]), static_cast<long long>(sf[1]), static_cast<long long>(sf[2]),
               static_cast<long long>(sf[3]));
    }
  }
  return 0;
}

int run_config(int config, int n_od, int n_spot) {
  sr_synth_params p{};
  p.config = config;
  p.n_on_demand = n_od;
  p.n_spot = n_spot;
  p.pinned_fraction = -1;
  p.init_fraction = 0.2;
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
  // the candidates: the pods of every on-demand node; asked at the last pod, the earlier pod q of candidate i
  // on spot node (5 i + q / 2) % ns (two pods a node)
  std::vector<int32_t> cp, coff(1, 0), at, map;
  for (int i = 0; i < nod; ++i) {
    int32_t k = 0;
    for (int j = off[odn[i]]; j < off[odn[i] + 1]; ++j)
      if (!(c.pods.flags[idx[j]] & (SR_POD_MIRROR | SR_POD_DAEMONSET_CONTROLLER))) {
        cp.push_back(idx[j]);
        map.push_back(ns > 0 ? (5 * i + k / 2) % ns : 0);
        ++k;
      }
    coff.push_back(static_cast<int32_t>(cp.size()));
    at.push_back(k - 1);  // -1: an empty candidate is not asked
  }
  const sr_candidates cands{nod, coff.data(), cp.data(), nullptr};
  Tally t;
  sr::PlanQueries pq;
  int rc = 0;
  if (sr::plan_queries(snap, &c, &cands, at.data(), map.data(), &pq) != SR_OK) rc = 3;
  const size_t batched = pq.batched.size();
  if (rc == 0) rc = check_queries(c, snap, pq, &t);
  // the same stop pods against the snapshot as it is: empty lists
  sr::PlanQueries bare;
  bare.pods = pq.pods;
  bare.off.assign(pq.pods.size() + 1, 0);
  if (rc == 0) rc = check_queries(c, snap, bare, &t);
  printf("config %d: spot %d candidates %d batched %zu queries %lld pairs %lld touched %lld with a shortfall %lld\n",
         config, ns, nod, batched, t.queries, t.pairs, t.touched, t.with_short);
  sr_snapshot_destroy(snap);
  sr_synth_destroy(s);
  if (rc) return rc;
  if (t.bad) {
    printf("FAILED: %lld pairs disagree\n", t.bad);
    return 1;
  }
  return t.with_short > 0 && t.touched > 0 ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv) {
  // small pools by default (a sanitizer build runs them in seconds); `shortfall_check <config> [od] [spot]` for one
  if (argc > 1) return run_config(atoi(argv[1]), argc > 2 ? atoi(argv[2]) : 0, argc > 3 ? atoi(argv[3]) : 0);
  const int runs[][3] = {{1, 0, 0}, {2, 12, 70}, {3, 20, 130}};
  for (const auto& r : runs) {
    const int rc = run_config(r[0], r[1], r[2]);
    if (rc) {
      printf(rc == 2 ? "FAILED: no shortfall seen\n" : "FAILED\n");
      return rc;
    }
  }
  printf("ok\n");
  return 0;
}
