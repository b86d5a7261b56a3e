// Host-only check of sr_node_view_pods / sr_node_view_plan (csrc/node_view.hpp, the node-view switch of
// csrc/explain_stage.hpp), on the synthetic configs of shortfall_check.  The candidates of a config are asked at
// their last pod, their earlier pods spread over the spot nodes by shortfall_check's rule; one stop pod is put
// outside the encoded predicate set, so the active order is not the asked order.  For several chunk sizes
// (node_view_chunks' own choice, 1, 3, 8 and more than the queries) a call of two launches is played:
//   launch 1  the stop pods with their context lists, slots shuffled;
//   launch 2  the same pods against the snapshot as it is, in slots above those of launch 1,
// both into the same totals.  Each launch goes plan / pack into a heap block of exactly in_bytes / view_args
// over it, a poisoned device block of exactly dev_out_bytes and a totals block of exactly
// node_view_layout(stride, 1).bytes; the kernels of csrc/node_view.hip are followed on the host through the
// argument pointers alone (the chunks in descending order: no result may depend on it), then the closing merge.
// The totals are unpacked into exact-size caller arrays and compared with a plain fold of explain_node_ctx /
// shortfall_node over all (query, node) pairs that uses neither NodeViewRow nor the layout.
// Stand-alone (its own main), so it is the program to build with sanitizers:
//   make -C k8s-spot-rescheduler_amd bin/node_view_check       && k8s-spot-rescheduler_amd/bin/node_view_check
//   make -C k8s-spot-rescheduler_amd bin/node_view_check_san   && k8s-spot-rescheduler_amd/bin/node_view_check_san
// Exit status 1: an array disagrees or a layout is wrong; 2: the run proves nothing (no sole query with a
// shortfall, no tie between the launches, no touched node, no fallback pod or a single chunk everywhere).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../k8s-spot-rescheduler_amd/csrc/explain_stage.hpp"
#include "../k8s-spot-rescheduler_amd/csrc/host.hpp"
#include "../k8s-spot-rescheduler_amd/csrc/synth/sr_synth.h"

namespace {

constexpr unsigned char kPoison = 0xA5;
constexpr size_t kDims = SR_SHORT_COUNT;
constexpr uint32_t kR = 1u << sr::WHY_PODS | 1u << sr::WHY_CPU | 1u << sr::WHY_MEMORY | 1u << sr::WHY_EPHEMERAL;
uint32_t dim_bit(size_t d) { return d < 3 ? 1u << (sr::WHY_CPU + d) : 1u << sr::WHY_PODS; }

struct Tally {
  long long calls = 0, bad = 0, sole_short = 0, ties = 0, touched = 0, fallback = 0, many_chunks = 0, ragged = 0;
};

// The caller's arrays, exact size.
struct Arrays {
  std::vector<int32_t> judged, admits, near, refuses, sole, sole_at;
  std::vector<int64_t> sole_min;
  explicit Arrays(size_t ns)
      : judged(1, 0x5a5a5a5a), admits(ns, 0x5a5a5a5a), near(ns, 0x5a5a5a5a), refuses(ns * SR_WHY_COUNT, 0x5a5a5a5a),
        sole(ns * SR_WHY_COUNT, 0x5a5a5a5a), sole_at(ns * kDims, 0x5a5a5a5a), sole_min(ns * kDims, 0x5a5a5a5a) {}
  sr_node_view_out out() {
    return {judged.data(), admits.data(), near.data(), refuses.data(), sole.data(), sole_min.data(), sole_at.data(), nullptr};
  }
  bool operator==(const Arrays& o) const {
    return judged == o.judged && admits == o.admits && near == o.near && refuses == o.refuses && sole == o.sole &&
           sole_at == o.sole_at && sole_min == o.sole_min;
  }
};

// The slack the kernels take on a touched node: node_left clamped (node_slack's clamp).
int32_t slack_of(int64_t left) {
  return static_cast<int32_t>(std::max<int64_t>(-(1 << 30), std::min<int64_t>(left, 1 << 30)));
}

// k_node_view and k_node_view_close through the argument pointers.
void emulate(const sr::ExplainPlanArgs& pa, const sr::NodeViewArgs& na) {
  const sr::ExplainArgs& a = pa.x;
  int32_t n_cls = 0;
  for (int32_t q = 0; q < a.n_pods; ++q) n_cls = std::max(n_cls, a.pods[q].cls + 1);
  sr::ExplainPrograms x;
  x.off.assign(a.xoff, a.xoff + n_cls + 1);
  x.ops.assign(a.xops, a.xops + x.off[n_cls]);
  const size_t stride = static_cast<size_t>(a.n_pad), ts = static_cast<size_t>(na.tot_stride);
  for (int32_t c = na.chunks - 1; c >= 0; --c) {
    const int32_t q0 = c * na.per, q1 = std::min(q0 + na.per, a.n_pods);
    uint64_t* pmin = na.part_min + static_cast<size_t>(c) * kDims * stride;
    int32_t* pcnt = na.part_cnt + static_cast<size_t>(c) * sr::kNodeViewCnt * stride;
    int32_t* pat = na.part_at + static_cast<size_t>(c) * kDims * stride;
    for (int32_t word = 0; word < a.Wp; ++word)
      for (int32_t node = word * 64; node < std::min(a.n_spot, word * 64 + 64); ++node) {  // (a pad writes nothing)
        sr::NodeViewRow row;
        for (int32_t q = q0; q < q1; ++q) {
          const sr::ExplainPod p = a.pods[q];
          const sr::PlanCtxEntry* e =
              na.lists ? sr::find_ctx(pa.ctx + pa.ctx_off[q], pa.ctx + pa.ctx_off[q + 1], node) : nullptr;
          const uint32_t m =
              sr::explain_node_ctx(x, p, a.atoms, a.Wp, a.node_free, a.n_pad, node, slack_of(na.node_left[node]), e);
          int64_t sf[kDims];
          sr::shortfall_node(m, p, a.node_free, a.n_pad, node, na.node_left[node], e, sf);
          sr::node_view_fold(m, sf, na.slot[q], &row);
        }
        sr::node_view_store(row, pmin, pcnt, pat, stride, static_cast<size_t>(node));
      }
  }
  for (int32_t node = 0; node < a.n_spot; ++node) {
    sr::NodeViewRow tot = sr::node_view_load(na.tot_min, na.tot_cnt, na.tot_at, ts, static_cast<size_t>(node));
    for (int32_t c = 0; c < na.chunks; ++c)
      sr::node_view_merge(&tot, sr::node_view_load(na.part_min + static_cast<size_t>(c) * kDims * stride,
                                                   na.part_cnt + static_cast<size_t>(c) * sr::kNodeViewCnt * stride,
                                                   na.part_at + static_cast<size_t>(c) * kDims * stride, stride,
                                                   static_cast<size_t>(node)));
    sr::node_view_store(tot, na.tot_min, na.tot_cnt, na.tot_at, ts, static_cast<size_t>(node));
  }
}

// The plain fold of one launch's queries into the expected arrays (started by node_view_clear's values).
bool direct(const sr::Workload& w, const sr::EncoderCache& cache, const sr_snapshot* snap, const sr::PlanQueries& pq,
            bool lists, const std::vector<int32_t>& slot, Arrays* r, Tally* t) {
  const size_t ns = snap->nodes.size();
  sr::ExplainPrograms x;
  std::vector<sr::ExplainPod> xp;
  if (!sr::build_explain(w, &x)) return false;
  sr::explain_pods(w, &xp);
  std::vector<int32_t> slack;
  std::vector<int64_t> left;
  sr::node_slack(snap, w.n_pad, &slack);
  sr::node_left(snap, w.n_pad, &left);
  for (size_t q = 0; q < w.pod_src.size(); ++q) {
    const size_t i = static_cast<size_t>(w.pod_src[q] - w.pod_base);
    const sr::PlanCtxEntry *lo = pq.entries.data() + pq.off[i], *hi = pq.entries.data() + pq.off[i + 1];
    ++r->judged[0];
    for (size_t node = 0; node < ns; ++node) {
      const sr::PlanCtxEntry* e = lists ? sr::find_ctx(lo, hi, static_cast<int32_t>(node)) : nullptr;
      t->touched += e != nullptr;
      const uint32_t m = sr::explain_node_ctx(x, xp[q], w.atoms.data(), w.Wp, cache.node_free.data(), w.n_pad,
                                              static_cast<int32_t>(node), slack[node], e);
      int64_t sf[kDims];
      sr::shortfall_node(m, xp[q], cache.node_free.data(), w.n_pad, static_cast<int32_t>(node), left[node], e, sf);
      r->admits[node] += m == 0;
      r->near[node] += m != 0 && (m & ~kR) == 0;
      for (size_t b = 0; b < SR_WHY_COUNT; ++b) {
        r->refuses[node * SR_WHY_COUNT + b] += m >> b & 1;
        r->sole[node * SR_WHY_COUNT + b] += m == 1u << b;
      }
      for (size_t d = 0; d < kDims; ++d) {
        if (m != dim_bit(d)) continue;
        int64_t& best = r->sole_min[node * kDims + d];
        int32_t& at = r->sole_at[node * kDims + d];
        t->sole_short += sf[d] > 0;
        t->ties += at >= 0 && sf[d] == best;
        if (at < 0 || sf[d] < best || (sf[d] == best && slot[i] < at)) best = sf[d], at = slot[i];
      }
    }
  }
  return true;
}

// The node-view layout beside the one the same call has as sr_shortfall_*: the shared input parts where they
// were, the slots behind them, no downloaded or zeroed byte, the partials the whole device block.
bool layout_ok(const sr::StageLayout& at, const sr::StageLayout& plain, const sr::Workload& w, sr::NodeViewChunks ch) {
  bool ok = true;
  for (int i = 0; i < sr::IN_PARTS; ++i) ok = ok && at.in[i].off == plain.in[i].off && at.in[i].bytes == plain.in[i].bytes;
  for (int i = 0; i < sr::OUT_PARTS; ++i) ok = ok && at.out[i].bytes == 0;
  ok = ok && at.view_slot.off == plain.in_bytes && at.view_slot.bytes == w.pod_src.size() * 4 &&
       at.in_bytes == ((at.view_slot.off + at.view_slot.bytes + 7) & ~size_t(7));
  ok = ok && at.out_bytes == 0 && at.zero_bytes == 0 && at.view_part.off == 0 &&
       at.view_part.bytes == sr::kNodeViewRowBytes * static_cast<size_t>(w.n_pad) * static_cast<size_t>(ch.chunks) &&
       at.dev_out_bytes == at.view_part.bytes;
  return ok && plain.view_slot.bytes == 0 && plain.view_part.bytes == 0;
}

int check_views(int config, const sr_cluster& c, const sr_snapshot* snap, const sr::PlanQueries& pq, Tally* t) {
  const int32_t nb = static_cast<int32_t>(pq.pods.size());
  const size_t ns = snap->nodes.size();
  if (nb == 0 || ns == 0) return 0;
  std::vector<int32_t> off(static_cast<size_t>(nb) + 1);
  for (int32_t i = 0; i <= nb; ++i) off[i] = i;
  const sr_candidates stops{nb, off.data(), pq.pods.data(), nullptr};
  std::vector<uint32_t> flags(c.pods.flags, c.pods.flags + c.pods.n);
  if (nb >= 3) flags[pq.pods[nb / 2]] |= SR_POD_FB_OTHER;
  sr_cluster cf = c;
  cf.pods.flags = flags.data();
  sr::EncoderCache cache;
  cache.want_why = true;
  sr::Workload w;
  std::string err;
  if (sr::encode_workload(&cache, snap, &cf, &stops, &w, &err) != SR_OK) return 3;
  if (w.pod_src.empty()) return 0;
  for (int32_t i = 0; i < nb; ++i) t->fallback += w.status_host[i] == SR_CAND_FALLBACK;
  // launch 1: shuffled slots below nb + 2; launch 2: the same order of slots above them (so equal shortfalls of
  // the two launches tie and the lower slot, launch 1's, must win whichever is merged first)
  const size_t slots = static_cast<size_t>(nb) + 2;
  std::vector<int32_t> slot1(slots), slot2(slots);
  for (size_t i = 0; i < slots; ++i) slot1[i] = static_cast<int32_t>(i);
  uint32_t rnd = 4711u + static_cast<uint32_t>(config);
  for (size_t i = slots - 1; i > 0; --i) {
    rnd = rnd * 1664525u + 1013904223u;
    std::swap(slot1[i], slot1[(rnd >> 8) % (i + 1)]);
  }
  for (size_t i = 0; i < slots; ++i) slot2[i] = slot1[i] + static_cast<int32_t>(slots);
  const size_t stride = static_cast<size_t>(sr::node_view_stride(static_cast<int32_t>(ns)));
  const size_t tot_bytes = sr::node_view_layout(stride, 1).bytes;
  sr::ExplainStage st;
  const int32_t pers[] = {0, 1, 3, 8, nb + 5};
  for (int32_t per : pers) {
    char* totals = static_cast<char*>(malloc(tot_bytes));
    std::memset(totals, 0, tot_bytes);
    Arrays got(ns), want(ns);
    sr_node_view_out go = got.out(), wo = want.out();
    sr::node_view_clear(&go, ns);
    sr::node_view_clear(&wo, ns);
    bool ok = true;
    int32_t judged = 0;
    sr::NodeViewChunks ch;
    for (int launch = 0; launch < 2; ++launch) {
      const bool lists = launch == 0;
      const std::vector<int32_t>& slot = lists ? slot1 : slot2;
      if (st.plan(w, cache.node_free, snap, lists ? &pq : nullptr, true, false, false, &err) != SR_OK) return 3;
      const sr::StageLayout plain = st.at();
      const sr::NodeViewAsk ask{slot.data(), per};
      if (st.plan(w, cache.node_free, snap, lists ? &pq : nullptr, false, true, true, &err, &ask) != SR_OK) {
        printf("plan failed: %s\n", err.c_str());
        return 3;
      }
      const sr::StageLayout& at = st.at();
      ch = st.chunks();
      ok = ok && layout_ok(at, plain, w, ch) && ch.chunks >= 1 && ch.per >= 1 &&
           static_cast<long long>(ch.chunks) * ch.per >= st.n_pods() &&
           static_cast<long long>(ch.chunks - 1) * ch.per < st.n_pods() && (per == 0 || ch.per == per);
      t->many_chunks += ch.chunks > 1;
      t->ragged += st.n_pods() % ch.per != 0;
      char* in = static_cast<char*>(malloc(at.in_bytes));
      char* dev = static_cast<char*>(malloc(at.dev_out_bytes));
      st.pack(in);
      std::memset(dev, kPoison, at.dev_out_bytes);
      sr::ExplainPlanArgs pa;
      sr::NodeViewArgs na;
      st.view_args(in, dev, totals, &pa, &na);
      emulate(pa, na);
      judged += st.n_pods();
      free(in), free(dev);
      ok = ok && direct(w, cache, snap, pq, lists, slot, &want, t);
    }
    *go.judged = judged;
    sr::node_view_unpack(totals, stride, ns, &go);
    free(totals);
    const bool same = got == want;
    printf("config %d node view chunk %d: pods %d per %d chunks %d: %s%s\n", config, per, st.n_pods(), ch.per, ch.chunks,
           ok ? "layout ok" : "LAYOUT WRONG", same ? ", results equal" : ", RESULTS DIFFER");
    ++t->calls;
    t->bad += !(ok && same);
  }
  return 0;
}

// node_view_chunks on its own: the bound of the header, whatever the number of queries.
bool chunks_ok() {
  bool ok = true;
  for (int32_t Wp : {1, 2, 4, 5, 55, 547, 4096})
    for (int32_t n : {1, 2, 7, 100, 1310, 65535, 65536, 1000000}) {
      const sr::NodeViewChunks c = sr::node_view_chunks(Wp, n);
      const long long gx = (Wp + 3) / 4;
      ok = ok && c.per >= 1 && c.chunks >= 1 && c.chunks <= n && 1ll * c.chunks * c.per >= n &&
           1ll * (c.chunks - 1) * c.per < n && c.chunks * gx <= sr::kNodeViewBlocks + gx;
      const sr::NodeViewChunks o = sr::node_view_chunks(Wp, n, 3);
      ok = ok && o.chunks <= sr::kNodeViewMaxChunks && 1ll * o.chunks * o.per >= n && (n > 3 * 65535 || o.per == 3);
    }
  return ok && sr::node_view_chunks(4, 0).chunks == 0;
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
  // the candidates of shortfall_check: the pods of every on-demand node, asked at the last pod, the earlier pod q
  // of candidate i on spot node (5 i + q / 2) % ns
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
    at.push_back(k - 1);
  }
  const sr_candidates cands{nod, coff.data(), cp.data(), nullptr};
  Tally t;
  sr::PlanQueries pq;
  int rc = 0;
  if (sr::plan_queries(snap, &c, &cands, at.data(), map.data(), &pq) != SR_OK) rc = 3;
  if (rc == 0) rc = check_views(config, c, snap, pq, &t);
  printf("config %d: spot %d candidates %d batched %zu; calls %lld, sole queries with a shortfall %lld, ties %lld, "
         "touched pairs %lld, fallback pods %lld, launches of several chunks %lld, with a ragged last chunk %lld\n",
         config, ns, nod, pq.batched.size(), t.calls, t.sole_short, t.ties, t.touched, t.fallback, t.many_chunks, t.ragged);
  sr_snapshot_destroy(snap);
  sr_synth_destroy(s);
  if (rc) return rc;
  if (t.bad) {
    printf("FAILED: %lld calls disagree\n", t.bad);
    return 1;
  }
  return t.sole_short > 0 && t.ties > 0 && t.touched > 0 && t.fallback > 0 && t.many_chunks > 0 && t.ragged > 0 ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv) {
  if (!chunks_ok()) {
    printf("FAILED: node_view_chunks breaks its bound\n");
    return 1;
  }
  if (argc > 1) return run_config(atoi(argv[1]), argc > 2 ? atoi(argv[2]) : 0, argc > 3 ? atoi(argv[3]) : 0);
  const int runs[][3] = {{1, 0, 0}, {2, 12, 70}, {3, 20, 130}};
  for (const auto& r : runs) {
    const int rc = run_config(r[0], r[1], r[2]);
    if (rc) {
      printf(rc == 2 ? "FAILED: the run proves nothing (see the header)\n" : "FAILED\n");
      return rc;
    }
  }
  printf("ok\n");
  return 0;
}
