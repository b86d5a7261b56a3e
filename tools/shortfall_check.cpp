// Host-only check of the statements sr_shortfall_pods / sr_shortfall_plan follow (csrc/explain_plan.hpp:
// shortfall_node, node_left) together with the plan_queries path, on synthetic configs.  The candidates of a
// config are asked at their last pod, their earlier pods spread over the spot nodes by a fixed rule (several
// on one node, so entries merge); every batched query's stop pod is evaluated on every spot node by
// explain_node_ctx and shortfall_node, and every number is recomputed from the snapshot's own node state:
//   bit d set  <=>  shortfall_d >= 1, and then shortfall_d == request_d + requested_d + acc_d - allocatable_d;
//   PODS set   <=>  pods shortfall >= 1, and then == pods + earlier pods there + 1 - allowed pods.
// The same pods are asked without a context too.
// The staging pass then takes every config's batched stop pods through csrc/explain_stage.hpp the way the planner
// does, for every combination of {no lists, lists} x {explain, shortfall} x {node_mask} x {node_short}: plan, pack
// into a heap block of exactly in_bytes, args over it and an output block of exactly dev_out_bytes (poisoned
// behind the zeroed prefix), the kernels followed on the host through the argument pointers alone, unpack of a
// copy of the first out_bytes through a shuffled slot mapping -- and compares every caller array with the same
// quantities computed without the unit.  The parts of both layouts must lie inside their buffers, apart from each
// other, aligned to their element types, and add up to in_bytes / out_bytes / dev_out_bytes.
// Stand-alone (its own main), so it is the program to build with sanitizers:
//   make -C k8s-spot-rescheduler_amd bin/shortfall_check       && k8s-spot-rescheduler_amd/bin/shortfall_check
//   make -C k8s-spot-rescheduler_amd bin/shortfall_check_san   && k8s-spot-rescheduler_amd/bin/shortfall_check_san
// Exit status 1: a number disagrees; 2: no query showed a shortfall or a touched node, or the staging pass saw no
// fallback pod or no active pod off its asked index (the run proves nothing).
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

struct Tally {
  long long pairs = 0, with_short = 0, touched = 0, bad = 0, queries = 0;
  // the staging pass: combinations run and failed, cleared slots of fallback pods compared, active pods whose
  // position differs from their asked index
  long long staged = 0, staged_bad = 0, fallback_slots = 0, reindexed = 0;
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
  std::vector<sr::PlanCtxEntry> entries;  // the lists in active-pod order
  std::vector<int32_t> eoff;
  sr::active_lists(w, pq, &entries, &eoff);
  for (int32_t q = 0; q < na; ++q) {
    const sr::PlanCtxEntry *lo = entries.data() + eoff[q], *hi = entries.data() + eoff[q + 1];
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
        printf("query %d node %d: mask %#x shortfalls %lld %lld %lld %lld\n", q, n, m,
               static_cast<long long>(sf[0]), static_cast<long long>(sf[1]), static_cast<long long>(sf[2]),
               static_cast<long long>(sf[3]));
    }
  }
  return 0;
}

// ---- the staging pass (csrc/explain_stage.hpp)

struct Combo {
  bool lists, shortfall, mask, nshort;
};

constexpr unsigned char kPoison = 0xA5;
constexpr size_t kDims = SR_SHORT_COUNT;
constexpr uint32_t kShortBits = 1u << sr::WHY_PODS | 1u << sr::WHY_CPU | 1u << sr::WHY_MEMORY | 1u << sr::WHY_EPHEMERAL;
uint32_t short_bit(size_t d) { return d < 3 ? 1u << (sr::WHY_CPU + d) : 1u << sr::WHY_PODS; }
size_t up8(size_t b) { return (b + 7) & ~size_t(7); }

template <class T>
void poison(std::vector<T>* v, size_t n) {
  v->resize(n);
  if (n) std::memset(v->data(), kPoison, n * sizeof(T));
}

// The caller's arrays of one call: `slots` entries each, poisoned; the optional ones only where the call asks.
struct Results {
  std::vector<int32_t> feasible, first, counts, near, only_nodes, only_at;
  std::vector<int64_t> only_min, node_short;
  std::vector<uint16_t> node_mask;
  std::vector<uint8_t> fallback;
  Results(size_t slots, size_t ns, const Combo& k) {
    const size_t sf = k.shortfall ? slots : 0;
    poison(&feasible, slots), poison(&first, slots), poison(&counts, slots * SR_WHY_COUNT), poison(&fallback, slots);
    poison(&node_mask, k.mask ? slots * ns : 0);
    poison(&near, sf), poison(&only_nodes, sf * kDims), poison(&only_min, sf * kDims), poison(&only_at, sf * kDims);
    poison(&node_short, k.nshort ? sf * ns * kDims : 0);
  }
  sr_explain_out out() {
    return {feasible.data(), first.data(), counts.data(), node_mask.empty() ? nullptr : node_mask.data(), fallback.data()};
  }
  sr_shortfall_out sh() {
    return {near.data(), only_nodes.data(), only_min.data(), only_at.data(), node_short.empty() ? nullptr : node_short.data()};
  }
  bool operator==(const Results& o) const {
    return feasible == o.feasible && first == o.first && counts == o.counts && near == o.near &&
           only_nodes == o.only_nodes && only_at == o.only_at && only_min == o.only_min && node_short == o.node_short &&
           node_mask == o.node_mask && fallback == o.fallback;
  }
};

// Every part inside its buffer, behind the part before it (so no two overlap), aligned to its element type and of
// the size the call's switches give it; the byte counts the sums of the parts, each padded to 8 bytes (the
// download ends unpadded with the masks, the partials follow at the next boundary).
bool layout_ok(const sr::StageLayout& at, const sr::Workload& w, const sr::ExplainStage& st, const Combo& k) {
  const size_t na = w.pod_src.size(), ns = static_cast<size_t>(w.n_spot), n_pad = static_cast<size_t>(w.n_pad);
  const size_t sf = k.shortfall ? na : 0, blocks = static_cast<size_t>((w.Wp + 3) / 4);
  const size_t in_want[sr::IN_PARTS] = {w.atoms.size() * 8, 3 * n_pad * 8, st.programs().off.size() * 4,
                                        st.programs().ops.size() * 4, na * sizeof(sr::ExplainPod),
                                        k.lists ? st.entries().size() * sizeof(sr::PlanCtxEntry) : 0,
                                        k.lists ? (na + 1) * 4 : 0, k.shortfall ? n_pad * 8 : k.lists ? n_pad * 4 : 0};
  const size_t out_want[sr::OUT_PARTS] = {na * sr::kExplainSums * 4, sf * sr::kShortSums * 4, sf * kDims * 8, sf * kDims * 4,
                                          k.nshort ? sf * ns * kDims * 8 : 0, k.mask ? na * ns * 2 : 0,
                                          sf * blocks * kDims * 8, sf * blocks * kDims * 4};
  const size_t in_elem[sr::IN_PARTS] = {8, 8, 4, 4, 8, 8, 4, k.shortfall ? size_t(8) : size_t(4)};
  const size_t out_elem[sr::OUT_PARTS] = {4, 4, 8, 4, 8, 2, 8, 4};
  bool ok = true;
  size_t end = 0, sum = 0;
  for (int i = 0; i < sr::IN_PARTS; ++i) {
    const sr::StagePart& p = at.in[i];
    ok = ok && p.off >= end && p.bytes == in_want[i] && p.elem == in_elem[i] && p.off % in_elem[i] == 0 &&
         p.off + p.bytes <= at.in_bytes;
    end = p.off + p.bytes;
    sum += up8(p.bytes);
  }
  ok = ok && at.in_bytes == sum;
  end = sum = 0;
  for (int i = 0; i < sr::OUT_PARTS; ++i) {
    const sr::StagePart& p = at.out[i];
    ok = ok && p.off >= end && p.bytes == out_want[i] && p.elem == out_elem[i] && p.off % out_elem[i] == 0 &&
         (p.bytes == 0 || p.off + p.bytes <= at.dev_out_bytes);
    if (i <= sr::OUT_MASKS) ok = ok && p.off + p.bytes <= at.out_bytes;  // the download holds all but the partials
    else ok = ok && p.off >= at.out_bytes;
    end = p.off + p.bytes;
    if (i < sr::OUT_MASKS) sum += up8(p.bytes);
  }
  ok = ok && at.out_bytes == sum + out_want[sr::OUT_MASKS];
  ok = ok && at.dev_out_bytes == (k.shortfall ? up8(at.out_bytes) + out_want[sr::OUT_PMIN] + out_want[sr::OUT_PAT] : at.out_bytes);
  return ok && at.zero_bytes == out_want[sr::OUT_SUMS] + out_want[sr::OUT_SSUMS];
}

// The kernels on the host, through the argument pointers alone: a block of four row words after the other, the
// sums added into (they start from the zeroed prefix), a block's partials written, then k_shortfall_close.
void emulate(const sr::ExplainPlanArgs& pa, const sr::ShortfallArgs& sa, const Combo& k) {
  const sr::ExplainArgs& a = pa.x;
  int32_t n_cls = 0;
  for (int32_t q = 0; q < a.n_pods; ++q) n_cls = std::max(n_cls, a.pods[q].cls + 1);
  sr::ExplainPrograms x;
  x.off.assign(a.xoff, a.xoff + n_cls + 1);
  x.ops.assign(a.xops, a.xops + x.off[n_cls]);
  const int32_t blocks = sr::shortfall_blocks(a.Wp);
  for (int32_t q = 0; q < a.n_pods; ++q) {
    const sr::ExplainPod p = a.pods[q];
    const sr::PlanCtxEntry *lo = k.lists ? pa.ctx + pa.ctx_off[q] : nullptr, *hi = k.lists ? pa.ctx + pa.ctx_off[q + 1] : nullptr;
    int32_t* sums = a.sums + static_cast<size_t>(q) * sr::kExplainSums;
    for (int32_t b = 0; b < blocks; ++b) {
      uint64_t bmin[kDims] = {sr::kShortNone, sr::kShortNone, sr::kShortNone, sr::kShortNone};
      int32_t bat[kDims] = {-1, -1, -1, -1};
      for (int32_t node = b * 256; node < std::min(a.n_spot, (b + 1) * 256); ++node) {
        const sr::PlanCtxEntry* e = k.lists ? sr::find_ctx(lo, hi, node) : nullptr;
        int32_t slack = 0;  // (read on a touched node only)
        if (k.lists && k.shortfall)
          slack = static_cast<int32_t>(std::max<int64_t>(-(1 << 30), std::min<int64_t>(sa.node_left[node], 1 << 30)));
        else if (k.lists)
          slack = pa.node_slack[node];
        const uint32_t m = sr::explain_node_ctx(x, p, a.atoms, a.Wp, a.node_free, a.n_pad, node, slack, e);
        for (int r = 0; r < SR_WHY_COUNT; ++r) sums[r] += m >> r & 1;
        if (m == 0) {
          ++sums[sr::kExplainFeasible];
          sums[sr::kExplainFirst] = std::max(sums[sr::kExplainFirst], a.n_pad - node);
        }
        const size_t at = static_cast<size_t>(q) * a.n_spot + node;
        if (a.node_mask) a.node_mask[at] = static_cast<uint16_t>(m);
        if (!k.shortfall) continue;
        int64_t sf[kDims];
        sr::shortfall_node(m, p, a.node_free, a.n_pad, node, sa.node_left[node], e, sf);
        if (sa.node_short) std::copy_n(sf, kDims, sa.node_short + at * kDims);
        int32_t* ss = sa.sums + static_cast<size_t>(q) * sr::kShortSums;
        ss[0] += m != 0 && (m & ~kShortBits) == 0;
        for (size_t d = 0; d < kDims; ++d)
          if (m == short_bit(d)) {
            ++ss[1 + d];
            if (static_cast<uint64_t>(sf[d]) < bmin[d]) bmin[d] = static_cast<uint64_t>(sf[d]), bat[d] = node;
          }
      }
      if (!k.shortfall) continue;
      const size_t o = (static_cast<size_t>(q) * sa.blocks + b) * kDims;
      std::copy_n(bmin, kDims, sa.part_min + o);
      std::copy_n(bat, kDims, sa.part_at + o);
    }
  }
  if (!k.shortfall) return;
  for (size_t t = 0; t < static_cast<size_t>(a.n_pods) * kDims; ++t) {
    uint64_t m = sr::kShortNone;
    int32_t at = -1;
    for (int32_t b = 0; b < sa.blocks; ++b) {
      const size_t o = (t / kDims * sa.blocks + b) * kDims + t % kDims;
      if (sa.part_min[o] < m) m = sa.part_min[o], at = sa.part_at[o];
    }
    sa.only_min[t] = at < 0 ? 0 : static_cast<int64_t>(m);
    sa.only_at[t] = at;
  }
}

// What the call must leave in the caller's arrays, computed from the workload, the snapshot and the asked lists
// without the staging unit: asked pod i into slot[i], a pod the encode handed back as fallback cleared.
bool direct(const sr::Workload& w, const sr::EncoderCache& cache, const sr_snapshot* snap, const sr::PlanQueries& pq,
            const Combo& k, const std::vector<int32_t>& slot, Results* r, Tally* t) {
  const size_t n = pq.pods.size(), ns = snap->nodes.size();
  sr::ExplainPrograms x;
  std::vector<sr::ExplainPod> xp;
  if (!sr::build_explain(w, &x)) return false;
  sr::explain_pods(w, &xp);
  std::vector<int32_t> slack;
  std::vector<int64_t> left;
  sr::node_slack(snap, w.n_pad, &slack);
  sr::node_left(snap, w.n_pad, &left);
  auto zero = [&](size_t o) {
    std::fill_n(r->counts.begin() + o * SR_WHY_COUNT, SR_WHY_COUNT, 0);
    if (k.mask) std::fill_n(r->node_mask.begin() + o * ns, ns, uint16_t(0));
    if (!k.shortfall) return;
    std::fill_n(r->only_nodes.begin() + o * kDims, kDims, 0);
    std::fill_n(r->only_min.begin() + o * kDims, kDims, int64_t(0));
    std::fill_n(r->only_at.begin() + o * kDims, kDims, -1);
    if (k.nshort) std::fill_n(r->node_short.begin() + o * ns * kDims, ns * kDims, int64_t(0));
  };
  for (size_t i = 0; i < n; ++i) {  // nothing evaluated
    const size_t o = static_cast<size_t>(slot[i]);
    zero(o);
    r->feasible[o] = r->first[o] = -1;
    r->fallback[o] = w.status_host[i] == SR_CAND_FALLBACK ? 1 : 0;
    if (k.shortfall) r->near[o] = -1;
    t->fallback_slots += r->fallback[o];
  }
  for (size_t q = 0; q < w.pod_src.size(); ++q) {
    const size_t i = static_cast<size_t>(w.pod_src[q] - w.pod_base), o = static_cast<size_t>(slot[i]);
    const sr::PlanCtxEntry *lo = pq.entries.data() + pq.off[i], *hi = pq.entries.data() + pq.off[i + 1];
    zero(o);
    r->feasible[o] = 0;
    if (k.shortfall) r->near[o] = 0;
    for (size_t node = 0; node < ns; ++node) {
      const sr::PlanCtxEntry* e = k.lists ? sr::find_ctx(lo, hi, static_cast<int32_t>(node)) : nullptr;
      const uint32_t m = sr::explain_node_ctx(x, xp[q], w.atoms.data(), w.Wp, cache.node_free.data(), w.n_pad,
                                              static_cast<int32_t>(node), slack[node], e);
      for (int b = 0; b < SR_WHY_COUNT; ++b) r->counts[o * SR_WHY_COUNT + b] += m >> b & 1;
      if (m == 0 && r->feasible[o]++ == 0) r->first[o] = static_cast<int32_t>(node);
      if (k.mask) r->node_mask[o * ns + node] = static_cast<uint16_t>(m);
      if (!k.shortfall) continue;
      int64_t sf[kDims];
      sr::shortfall_node(m, xp[q], cache.node_free.data(), w.n_pad, static_cast<int32_t>(node), left[node], e, sf);
      if (k.nshort) std::copy_n(sf, kDims, r->node_short.begin() + (o * ns + node) * kDims);
      r->near[o] += m != 0 && (m & ~kShortBits) == 0;
      for (size_t d = 0; d < kDims; ++d) {
        if (m != short_bit(d)) continue;
        ++r->only_nodes[o * kDims + d];
        if (r->only_at[o * kDims + d] < 0 || sf[d] < r->only_min[o * kDims + d])  // the lowest position on ties
          r->only_min[o * kDims + d] = sf[d], r->only_at[o * kDims + d] = static_cast<int32_t>(node);
      }
    }
  }
  return true;
}

// The batched stop pods of `pq` as the planner's explain() takes them, through every combination of the switches.
int check_staging(int config, const sr_cluster& c, const sr_snapshot* snap, const sr::PlanQueries& pq, Tally* t) {
  const int32_t nb = static_cast<int32_t>(pq.pods.size());
  const size_t ns = snap->nodes.size();
  if (nb == 0) return 0;
  std::vector<int32_t> off(static_cast<size_t>(nb) + 1);
  for (int32_t i = 0; i <= nb; ++i) off[i] = i;
  const sr_candidates stops{nb, off.data(), pq.pods.data(), nullptr};
  // a private copy of the pod flags in which the middle stop pod is outside the encoded predicate set: the encode
  // hands it back as fallback, so the active order is not the asked order and a cleared slot lies between filled
  // ones
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
  for (size_t q = 0; q < w.pod_src.size(); ++q) t->reindexed += w.pod_src[q] - w.pod_base != static_cast<int32_t>(q);
  // a shuffled slot mapping with two slots nobody writes
  const size_t slots = static_cast<size_t>(nb) + 2;
  std::vector<int32_t> slot(slots);
  for (size_t i = 0; i < slots; ++i) slot[i] = static_cast<int32_t>(i);
  uint32_t rnd = 12345u + static_cast<uint32_t>(config);
  for (size_t i = slots - 1; i > 0; --i) {
    rnd = rnd * 1664525u + 1013904223u;
    std::swap(slot[i], slot[(rnd >> 8) % (i + 1)]);
  }
  sr::ExplainStage st;  // one for all combinations, as the context keeps one
  for (int bits = 0; bits < 16; ++bits) {
    const Combo k{(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0};
    if (k.nshort && !k.shortfall) continue;
    if (st.plan(w, cache.node_free, snap, k.lists ? &pq : nullptr, k.shortfall, k.mask, k.nshort, &err) != SR_OK) {
      printf("plan failed: %s\n", err.c_str());
      return 3;
    }
    const sr::StageLayout& at = st.at();
    bool ok = layout_ok(at, w, st, k);
    // exact-size heap blocks: a part outside its buffer is the sanitizer's to report
    char* in = static_cast<char*>(malloc(at.in_bytes));
    char* dev = static_cast<char*>(malloc(at.dev_out_bytes));
    char* image = static_cast<char*>(malloc(at.out_bytes));
    st.pack(in);
    std::memset(dev, kPoison, at.dev_out_bytes);
    std::memset(dev, 0, at.zero_bytes);
    sr::ExplainPlanArgs pa;
    sr::ShortfallArgs sa;
    st.args(in, dev, &pa, &sa);
    emulate(pa, sa, k);
    std::memcpy(image, dev, at.out_bytes);
    Results got(slots, ns, k), want(slots, ns, k);
    sr_explain_out out = got.out();
    sr_shortfall_out sh = got.sh();
    for (int32_t i = 0; i < nb; ++i)
      sr::clear_slot(&out, k.shortfall ? &sh : nullptr, static_cast<size_t>(slot[i]), ns,
                     w.status_host[i] == SR_CAND_FALLBACK ? 1 : 0);
    st.unpack(image, slot.data(), &out, k.shortfall ? &sh : nullptr);
    free(in), free(dev), free(image);
    const bool same = direct(w, cache, snap, pq, k, slot, &want, t) && got == want;
    printf("config %d staging lists %d shortfall %d node_mask %d node_short %d: pods %zu in %zu out %zu device %zu: %s%s\n",
           config, k.lists, k.shortfall, k.mask, k.nshort, w.pod_src.size(), at.in_bytes, at.out_bytes, at.dev_out_bytes,
           ok ? "layout ok" : "LAYOUT WRONG", same ? ", results equal" : ", RESULTS DIFFER");
    ++t->staged;
    t->staged_bad += !(ok && same);
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
  // staged: an odd number of them, so that with these pools the masks end off an 8-byte boundary and the
  // partials behind them start after padding
  sr::PlanQueries odd = pq;
  if (odd.pods.size() > 1 && odd.pods.size() % 2 == 0) {
    odd.pods.pop_back(), odd.batched.pop_back(), odd.off.pop_back();
    odd.entries.resize(static_cast<size_t>(odd.off.back()));
  }
  if (rc == 0) rc = check_staging(config, c, snap, odd, &t);
  printf("config %d: spot %d candidates %d batched %zu queries %lld pairs %lld touched %lld with a shortfall %lld; "
         "staging combinations %lld, fallback slots in them %lld, active pods off their asked index %lld\n",
         config, ns, nod, batched, t.queries, t.pairs, t.touched, t.with_short, t.staged, t.fallback_slots, t.reindexed);
  sr_snapshot_destroy(snap);
  sr_synth_destroy(s);
  if (rc) return rc;
  if (t.bad) {
    printf("FAILED: %lld pairs disagree\n", t.bad);
    return 1;
  }
  if (t.staged_bad) {
    printf("FAILED: %lld staging combinations disagree\n", t.staged_bad);
    return 1;
  }
  // (a staging pass without a fallback pod, or whose active order is the asked order, proves nothing either)
  return t.with_short > 0 && t.touched > 0 && t.fallback_slots > 0 && t.reindexed > 0 ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv) {
  // small pools by default (a sanitizer build runs them in seconds); `shortfall_check <config> [od] [spot]` for one
  if (argc > 1) return run_config(atoi(argv[1]), argc > 2 ? atoi(argv[2]) : 0, argc > 3 ? atoi(argv[3]) : 0);
  const int runs[][3] = {{1, 0, 0}, {2, 12, 70}, {3, 20, 130}};
  for (const auto& r : runs) {
    const int rc = run_config(r[0], r[1], r[2]);
    if (rc) {
      printf(rc == 2 ? "FAILED: no shortfall, touched node, fallback slot or re-indexed pod seen\n" : "FAILED\n");
      return rc;
    }
  }
  printf("ok\n");
  return 0;
}
