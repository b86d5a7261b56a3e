// Host-only check of sr_blockers_plan (csrc/blockers.hpp), on the synthetic configs of shortfall_check.  The
// candidates of a config are the pods of every on-demand node; every one is asked but the second.  The call is
// played as the planner plays it:
//   blockers_ways sorts the candidates; the pods of the batched ones are encoded as single-pod candidates with
//   one pod of one candidate put outside the encoded predicate set, so that candidate must leave the batch;
//   BlockersStage::plan / pack into a heap block of exactly in_bytes, args over it and a poisoned output block
//   of exactly out_bytes whose zeroed prefix is zero_bytes; the kernel of csrc/blockers.hip is followed on the
//   host through the argument pointers alone (blockers_candidate per candidate, the programs rebuilt from the
//   block); unpack into exact-size caller arrays; with and without counts.
// Every kept candidate's outputs are compared with a naive second implementation that really forks the
// snapshot, encodes each pod alone against the forked state, judges every node with explain_node, adds the pod
// where it fits first and reverts: no context list, no explain_node_ctx, no layout.
// Stand-alone (its own main), so it is the program to build with sanitizers:
//   make -C k8s-spot-rescheduler_amd bin/blockers_check       && k8s-spot-rescheduler_amd/bin/blockers_check
//   make -C k8s-spot-rescheduler_amd bin/blockers_check_san   && k8s-spot-rescheduler_amd/bin/blockers_check_san
// Exit status 1: an output disagrees or a layout is wrong; 2: the run proves nothing (no candidate with two
// blockers, none with a pod placed behind a blocker, no pod judged on a node its candidate had touched or no
// candidate that left the batch, in any of the configs).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../k8s-spot-rescheduler_amd/csrc/blockers.hpp"
#include "../k8s-spot-rescheduler_amd/csrc/host.hpp"
#include "../k8s-spot-rescheduler_amd/csrc/synth/sr_synth.h"

namespace {

constexpr unsigned char kPoison = 0xA5;

struct Tally {
  long long kept = 0, bad = 0, two = 0, behind = 0, shared = 0, left_batch = 0, single = 0, blockers = 0, fallback = 0;
};

struct Arrays {
  std::vector<int32_t> blockers, first, map, counts;
  std::vector<uint8_t> fallback;
  Arrays(size_t nc, size_t np)
      : blockers(nc, 0x5a5a5a5a), first(nc, 0x5a5a5a5a), map(np, 0x5a5a5a5a), counts(np * SR_WHY_COUNT, 0x5a5a5a5a),
        fallback(nc, 0x5a) {}
  sr_blockers_out out(bool with_counts) {
    return {blockers.data(), first.data(), map.data(), with_counts ? counts.data() : nullptr, fallback.data()};
  }
};

int32_t slack_of(int64_t left) {
  return static_cast<int32_t>(std::max<int64_t>(-(1 << 30), std::min<int64_t>(left, 1 << 30)));
}

size_t up8(size_t b) { return (b + 7) & ~size_t(7); }

// The two part tables against the documented layout, written out here: the input parts atoms, node_free, xoff,
// xops, pods, cand_off, node_left
// and the output parts counts (absent when not wanted), node_of_pod, one count per candidate, first, in that
// order; each of the size the pass gives it, at the 8-byte boundary after the part before it (so no two overlap)
// and a multiple of its element size; the byte counts the rounded ends; the zeroed prefix the counts.
bool layout_ok(const sr::BlockersLayout& at, const sr::Workload& w, const sr::BlockersStage& st, bool with_counts) {
  const size_t np = static_cast<size_t>(st.n_pods()), nk = static_cast<size_t>(st.n_cand()), n_pad = static_cast<size_t>(w.n_pad);
  const size_t in_want[sr::BIN_PARTS] = {w.atoms.size() * 8, 3 * n_pad * 8, st.programs().off.size() * 4,
                                       st.programs().ops.size() * 4, np * sizeof(sr::BlockerPod), (nk + 1) * 4, n_pad * 8};
  const size_t in_elem[sr::BIN_PARTS] = {8, 8, 4, 4, 8, 4, 8};
  const size_t out_want[sr::GOUT_PARTS] = {with_counts ? np * SR_WHY_COUNT * 4 : 0, np * 4, nk * 4, nk * 4};
  bool ok = at.n_in == sr::BIN_PARTS;
  size_t end = 0;
  for (int i = 0; i < sr::BIN_PARTS; ++i) {
    const sr::StagePart& p = at.in[i];
    ok = ok && p.off == up8(end) && p.bytes == in_want[i] && p.elem == in_elem[i] && p.off % in_elem[i] == 0;
    end = p.off + p.bytes;
  }
  ok = ok && at.in_bytes == up8(end);
  end = 0;
  for (int i = 0; i < sr::GOUT_PARTS; ++i) {
    const sr::StagePart& p = at.out[i];
    ok = ok && p.off == up8(end) && p.bytes == out_want[i] && p.elem == 4 && p.off % 4 == 0;
    end = p.off + p.bytes;
  }
  return ok && at.out_bytes == up8(end) && at.zero_bytes == out_want[sr::GOUT_COUNTS];
}

// k_blockers through the argument pointers.
void emulate(const sr::BlockersArgs& b) {
  const sr::ExplainArgs& a = b.x;
  int32_t n_cls = 0;
  for (int32_t q = 0; q < a.n_pods; ++q) n_cls = std::max(n_cls, b.pods[q].p.cls + 1);
  sr::ExplainPrograms x;
  x.off.assign(a.xoff, a.xoff + n_cls + 1);
  x.ops.assign(a.xops, a.xops + x.off[n_cls]);
  std::vector<int32_t> slack(static_cast<size_t>(a.n_pad));
  for (int32_t i = 0; i < a.n_pad; ++i) slack[i] = slack_of(b.node_left[i]);
  for (int32_t c = b.n_cand - 1; c >= 0; --c) {  // (no result may depend on the order of the waves)
    const int32_t p0 = b.cand_off[c], np = b.cand_off[c + 1] - p0;
    b.blockers[c] = sr::blockers_candidate(x, b.pods + p0, np, a.atoms, a.Wp, a.node_free, a.n_pad, a.n_spot,
                                           slack.data(), b.node_of_pod + p0,
                                           b.counts ? b.counts + static_cast<size_t>(p0) * SR_WHY_COUNT : nullptr,
                                           b.first + c);
  }
}

// The contract's loop, naively.  Returns false on an encoder error.
bool naive(const sr_cluster* c, sr_snapshot* snap, const int32_t* pods, int32_t np, int32_t* blockers, int32_t* first,
           int32_t* map, int32_t* counts, uint8_t* fallback, Tally* t) {
  const int32_t ns = static_cast<int32_t>(snap->nodes.size());
  if (sr_snapshot_fork(snap) != SR_OK) return false;
  *blockers = 0;
  *first = -1;
  *fallback = 0;
  std::fill_n(counts, static_cast<size_t>(np) * SR_WHY_COUNT, 0);
  std::vector<int32_t> used;
  bool ok = true, seen_blocker = false;
  for (int32_t k = 0; k < np && ok && !*fallback; ++k) {
    const int32_t off[2] = {0, 1};
    const sr_candidates one{1, off, pods + k, nullptr};
    sr::EncoderCache cache;
    cache.want_why = true;
    sr::Workload w;
    std::string err;
    sr::ExplainPrograms x;
    std::vector<sr::ExplainPod> xp;
    if (sr::encode_workload(&cache, snap, c, &one, &w, &err) != SR_OK) ok = false;
    if (ok && w.status_host[0] == SR_CAND_FALLBACK) {
      *fallback = 1;
      break;
    }
    if (!ok || w.pod_src.size() != 1 || !sr::build_explain(w, &x)) {
      ok = false;
      break;
    }
    sr::explain_pods(w, &xp);
    int32_t at = -1, row[SR_WHY_COUNT] = {0};
    for (int32_t node = 0; node < ns; ++node) {
      const uint32_t m = sr::explain_node(x, xp[0], w.atoms.data(), w.Wp, cache.node_free.data(), w.n_pad, node);
      if (m == 0 && at < 0) at = node;
      if (std::find(used.begin(), used.end(), node) != used.end()) ++t->shared;
      for (int r = 0; r < SR_WHY_COUNT; ++r) row[r] += m >> r & 1;
    }
    map[k] = at;
    if (at >= 0) {
      sr::snapshot_add_pod(snap, c, pods[k], at);
      used.push_back(at);
      t->behind += seen_blocker;
      continue;
    }
    seen_blocker = true;
    ++*blockers;
    if (*first < 0) *first = k;
    std::copy_n(row, SR_WHY_COUNT, counts + static_cast<size_t>(k) * SR_WHY_COUNT);
  }
  if (sr_snapshot_revert(snap) != SR_OK) return false;
  if (*fallback) {
    *blockers = *first = -1;
    std::fill_n(map, np, -1);
    std::fill_n(counts, static_cast<size_t>(np) * SR_WHY_COUNT, 0);
  }
  return ok;
}

int check_call(int config, const sr_cluster& c, sr_snapshot* snap, const sr_candidates& cands,
               const std::vector<int32_t>& ask, Tally* t) {
  const int32_t nc = cands.n_cand;
  const int32_t* off = cands.cand_pod_off;
  const size_t total = static_cast<size_t>(off[nc] - off[0]);
  sr::BlockerWays rule;
  if (sr::blockers_ways(snap, &c, &cands, ask.data(), &rule) != SR_OK) return 3;
  for (int32_t i = 0; i < nc; ++i) t->single += rule.how[i] == SR_EXPLAIN_SINGLE;
  std::vector<int32_t> flat;
  sr::blockers_flat(&cands, rule, &flat);
  if (flat.empty()) return 0;
  // one pod of the middle batched candidate outside the encoded set
  std::vector<uint32_t> flags(c.pods.flags, c.pods.flags + c.pods.n);
  const int32_t victim = rule.batched[rule.batched.size() / 2];
  if (rule.batched.size() >= 3 && off[victim + 1] > off[victim]) flags[cands.cand_pods[off[victim + 1] - 1]] |= SR_POD_FB_OTHER;
  sr_cluster cf = c;
  cf.pods.flags = flags.data();
  const int32_t n = static_cast<int32_t>(flat.size());
  std::vector<int32_t> soff(static_cast<size_t>(n) + 1);
  for (int32_t i = 0; i <= n; ++i) soff[i] = i;
  const sr_candidates singles{n, soff.data(), flat.data(), nullptr};
  sr::EncoderCache cache;
  cache.want_why = true;
  sr::Workload w;
  std::string err;
  if (sr::encode_workload(&cache, snap, &cf, &singles, &w, &err) != SR_OK) return 3;
  for (int with_counts = 1; with_counts >= 0; --with_counts) {
    sr::BlockerWays ways = rule;
    sr::BlockersStage st;
    if (st.plan(w, cache.node_free, snap, &cf, &cands, &ways, with_counts != 0, &err) != SR_OK) {
      printf("plan failed: %s\n", err.c_str());
      return 3;
    }
    const sr::BlockersLayout& at = st.at();
    long long left_batch = 0;
    for (int32_t i = 0; i < nc; ++i) left_batch += rule.how[i] == SR_EXPLAIN_BATCHED && ways.how[i] == SR_EXPLAIN_SINGLE;
    bool ok = at.zero_bytes == (with_counts ? static_cast<size_t>(st.n_pods()) * SR_WHY_COUNT * 4 : 0) &&
              at.out_bytes >= at.out[sr::GOUT_FIRST].off + static_cast<size_t>(st.n_cand()) * 4 && at.in_bytes % 8 == 0 &&
              static_cast<size_t>(st.n_cand()) + left_batch == rule.batched.size() &&
              layout_ok(at, w, st, with_counts != 0);
    char* in = static_cast<char*>(malloc(at.in_bytes));
    char* dev = static_cast<char*>(malloc(at.out_bytes));
    st.pack(in);
    std::memset(dev, kPoison, at.out_bytes);
    std::memset(dev, 0, at.zero_bytes);
    sr::BlockersArgs ba;
    st.args(in, dev, &ba);
    emulate(ba);
    Arrays got(static_cast<size_t>(nc), total);
    sr_blockers_out go = got.out(with_counts != 0);
    for (int32_t i = 0; i < nc; ++i) sr::blockers_clear(&cands, i, 0, &go);
    st.unpack(dev, &cands, &go);
    free(in), free(dev);
    long long bad = 0;
    for (int32_t i = 0; i < nc; ++i) {
      const size_t p0 = static_cast<size_t>(off[i] - off[0]);
      const int32_t np = off[i + 1] - off[i];
      if (ways.how[i] != SR_EXPLAIN_BATCHED) {  // not the kernel's: still "not judged"
        bool clear = got.blockers[i] == -1 && got.first[i] == -1 && got.fallback[i] == 0;
        for (int32_t k = 0; k < np; ++k) clear = clear && got.map[p0 + k] == -1;
        bad += !clear;
        continue;
      }
      int32_t wb, wf;
      uint8_t wfb;
      std::vector<int32_t> wmap(static_cast<size_t>(std::max(np, 1))), wcnt(static_cast<size_t>(std::max(np, 1)) * SR_WHY_COUNT);
      Tally scratch;
      if (!naive(&cf, snap, cands.cand_pods + off[i], np, &wb, &wf, wmap.data(), wcnt.data(), &wfb, with_counts ? t : &scratch))
        return 3;
      bool same = !wfb && got.blockers[i] == wb && got.first[i] == wf && got.fallback[i] == 0 &&
                  std::equal(wmap.begin(), wmap.begin() + np, got.map.begin() + p0);
      if (with_counts) same = same && std::equal(wcnt.begin(), wcnt.begin() + static_cast<size_t>(np) * SR_WHY_COUNT,
                                                 got.counts.begin() + p0 * SR_WHY_COUNT);
      if (!same) printf("config %d candidate %d: got %d blockers first %d, want %d first %d (fallback %d)\n", config, i,
                        got.blockers[i], got.first[i], wb, wf, wfb);
      bad += !same;
      if (with_counts) {
        ++t->kept;
        t->two += wb >= 2;
        t->blockers += wb;
      }
    }
    if (with_counts) t->left_batch += left_batch;
    printf("config %d %s counts: kernel candidates %d pods %d, left the batch %lld: %s%s\n", config,
           with_counts ? "with" : "without", st.n_cand(), st.n_pods(), left_batch, ok ? "layout ok" : "LAYOUT WRONG",
           bad ? ", RESULTS DIFFER" : ", results equal");
    t->bad += bad + !ok;
  }
  return 0;
}

// The candidate-level rule at the context capacity: pods of one spec, capacity and capacity + 1 of them.
bool capacity_ok(const sr_cluster& c, const sr_snapshot* snap, const std::vector<int32_t>& plain_pods) {
  if (plain_pods.empty()) return true;
  std::vector<int32_t> pods;
  for (int i = 0; i < 2 * sr::kBlockersCtx + 1; ++i) pods.push_back(plain_pods[static_cast<size_t>(i) % plain_pods.size()]);
  const int32_t off[3] = {0, sr::kBlockersCtx, 2 * sr::kBlockersCtx + 1}, ask[2] = {0, 0};
  const sr_candidates cands{2, off, pods.data(), nullptr};
  sr::BlockerWays ways;
  return sr::blockers_ways(snap, &c, &cands, ask, &ways) == SR_OK && ways.how[0] == SR_EXPLAIN_BATCHED &&
         ways.how[1] == SR_EXPLAIN_SINGLE;
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
  std::vector<int32_t> cp, coff(1, 0), ask;
  for (int i = 0; i < nod; ++i) {
    for (int j = off[odn[i]]; j < off[odn[i] + 1]; ++j)
      if (!(c.pods.flags[idx[j]] & (SR_POD_MIRROR | SR_POD_DAEMONSET_CONTROLLER))) cp.push_back(idx[j]);
    coff.push_back(static_cast<int32_t>(cp.size()));
    ask.push_back(i == 1 ? -1 : 0);
  }
  const sr_candidates cands{nod, coff.data(), cp.data(), nullptr};
  Tally t;
  int rc = check_call(config, c, snap, cands, ask, &t);
  // pods the rule takes in any number: those of the candidates it batched
  std::vector<int32_t> plain;
  sr::BlockerWays ways;
  if (rc == 0 && sr::blockers_ways(snap, &c, &cands, ask.data(), &ways) == SR_OK)
    for (int32_t b : ways.batched)
      for (int32_t j = coff[b]; j < coff[b + 1]; ++j) {
        const sr::PodTraits tr = sr::pod_traits(&c, cp[j]);
        if (!tr.ports && !tr.scalars && !tr.terms && !tr.spread) plain.push_back(cp[j]);
      }
  if (rc == 0 && !capacity_ok(c, snap, plain)) {
    printf("FAILED: the rule at the context capacity\n");
    rc = 1;
  }
  printf("config %d: spot %d candidates %d, kernel candidates %lld with %lld blockers; with two or more %lld, pods placed "
         "behind a blocker %lld, pairs judged on a touched node %lld, left the batch %lld, SINGLE by the rule %lld\n",
         config, ns, nod, t.kept, t.blockers, t.two, t.behind, t.shared, t.left_batch, t.single);
  sr_snapshot_destroy(snap);
  sr_synth_destroy(s);
  if (rc) return rc;
  if (t.bad) {
    printf("FAILED: %lld disagreements\n", t.bad);
    return 1;
  }
  return t.two > 0 && t.behind > 0 && t.shared > 0 && t.left_batch > 0 ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1) return run_config(atoi(argv[1]), argc > 2 ? atoi(argv[2]) : 0, argc > 3 ? atoi(argv[3]) : 0);
  const int runs[][3] = {{1, 0, 0}, {2, 12, 70}, {3, 20, 130}};
  int proved = 0;
  for (const auto& r : runs) {
    const int rc = run_config(r[0], r[1], r[2]);
    if (rc != 0 && rc != 2) {
      printf("FAILED\n");
      return rc;
    }
    proved += rc == 0;
  }
  if (proved == 0) {
    printf("FAILED: no run proves anything (see the header)\n");
    return 2;
  }
  printf("ok\n");
  return 0;
}
