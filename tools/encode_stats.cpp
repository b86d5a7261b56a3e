// Host-only harness: NewNodeMap + snapshot + encode_workload on a synthetic
// config, printing the workload's dimensions and host-side timings (no GPU).
//   make -C k8s-spot-rescheduler_amd tools && k8s-spot-rescheduler_amd/bin/encode_stats 3 [max candidates] [check | reuse [ticks [burst]] | residency [ticks [burst]]]
//   (reuse-perm: pods on spot nodes change requests between ticks, the spot order moves;
//    reuse-scalar: every spot node allocating an extended resource is filled past its allocatable
//    for two ticks in six and freed again, so scalar query rows go empty <-> non-empty while reused)
// Encodes are timed cold (empty encoder cache), warm (the same snapshot
// again) and after one spot node changed (a fresh snapshot with one more pod
// on one node), the steady state of a planner between two ticks.
#include <chrono>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../k8s-spot-rescheduler_amd/csrc/host.hpp"
#include "../k8s-spot-rescheduler_amd/csrc/residency.hpp"
#include "../k8s-spot-rescheduler_amd/csrc/synth/sr_synth.h"

namespace sr { extern double encode_phase_ms[16]; }

static double ms_since(std::chrono::steady_clock::time_point a) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
}

static void phases(const char* tag) {
  const double* p = sr::encode_phase_ms;
  printf("  %-6s phases(ms): views %.3f pass1 %.3f ports %.3f gather %.3f shards %.3f specs-new %.3f keys %.3f "
         "classes %.3f atoms %.3f lb+empty %.3f pods %.3f trows %.3f recs %.3f lists %.3f reuse %.3f\n",
         tag, p[0], p[5], p[1], p[9], p[14], p[7], p[2], p[3], p[4], p[8], p[10], p[12], p[13], p[6], p[11]);
}

// ---- `residency` mode: the planner's slot bookkeeping (residency.hpp) on a
// host model of the staging arena H, the device arena D and the tables.
namespace {

struct Cluster {  // what main() built
  sr_cluster& c;
  sr_node_map_params& prm;
  sr_node_map& m;
  std::vector<int32_t>&spot, &off, &idx;
  int32_t& ns;
  const std::vector<int32_t>&coff, &cp;
  int32_t nod;
};

// One workload slot of the model.  The buffers grow as the planner's do (a
// quarter of headroom); a new one is filled with a pattern no section holds.
struct ModelSlot {
  sr::Workload w;
  sr::Residency res;
  std::vector<char> H, D;
  size_t tables_cap = 0;
  // node records, free values, atoms and thresholds as of the last K0 commit: the model of the tables
  bool tables_valid = false;
  std::vector<uint64_t> t_node_rec, t_atoms;
  std::vector<int64_t> t_node_free, t_thr;
};

bool grow(std::vector<char>& b, size_t bytes, bool force) {
  if (bytes <= b.size() && !force) return false;
  b.assign(std::max<size_t>(std::max(bytes, b.size()) + bytes / 4, 4096), static_cast<char>(0xEE));
  return true;
}

struct Residual {  // the summary
  int ticks = 0, full = 0, inc = 0, skip = 0, bad = 0;
  int uncommitted = 0, arena = 0, tables = 0, staging = 0, reorders = 0, enc_errors = 0, moved = 0;
  int tick = 0;
  void fail(const char* what, const char* sec, long i) {
    if (bad++ < 8) printf("residency tick %d: %s: %s at %ld\n", tick, what, sec, i);
  }
};

template <class T>
long first_diff(const char* buf, size_t off, const std::vector<T>& v) {  // -1: the section equals its source
  if (v.empty() || std::memcmp(buf + off, v.data(), v.size() * sizeof(T)) == 0) return -1;
  const T* b = reinterpret_cast<const T*>(buf + off);
  long i = 0;
  while (b[i] == v[i]) ++i;
  return i;
}

// Every section of `buf` but the node section and the pod records against its source vector.
void check_sections(Residual& R, const char* what, const char* buf, const sr::ArenaLayout& at, const sr::Workload& w,
                    const sr::TickLists& tl, bool atoms) {
  auto sec = [&](const char* name, size_t off, const auto& v) {
    const long i = first_diff(buf, off, v);
    if (i >= 0) R.fail(what, name, i);
  };
  sec("cls_prog_off", at.cls_prog_off, w.cls_prog_off);
  sec("cls_prog", at.cls_prog, w.cls_prog);
  sec("cls_prog8", at.cls_prog8, w.cls_prog8);
  sec("cand_off", at.cand_off, w.cand_off);
  sec("cand_global", at.cand_global, w.cand_global);
  sec("list", at.list, w.list);
  if (at.dyn) sec("dyn_cand", at.dyn_cand, w.dyn_cand), sec("dyn_pod", at.dyn_pod, w.dyn_pod), sec("ds_info", at.ds_info, w.ds_info);
  if (at.ext) sec("ext_cand", at.ext_cand, w.ext_cand), sec("pod_ext", at.pod_ext, w.pod_ext), sec("list_ext", at.list_ext, w.list_ext);
  if (atoms) sec("atoms", at.atoms, w.atoms);
  if (at.ext) sec("node_scal", at.node_scal, w.node_scal);
  if (at.dyn) sec("sp_tab", at.sp_tab, w.sp_tab), sec("dk_dom", at.dk_dom, w.dk_dom);
  sec("t_thr", at.t_thr, w.t_thr);
  if (at.node_patch) sec("node_patch", at.node_patch, tl.node_patch);
  if (at.pod_patch) sec("pod_patch", at.pod_patch, tl.pod_patch);
  if (at.k0_cols) sec("k0_cols", at.k0_cols, tl.k0_cols);
  if (at.k0_rows) sec("k0_rows", at.k0_rows, tl.k0_rows);
}

// One prepare (and run, unless `commit` is false) of the model slot for the
// workload just encoded into it.  inject: bit 0 staging, 1 arena, 2 tables moved.
void residency_tick(Residual& R, ModelSlot& S, const sr::EncoderCache& E, sr::TickLists& tl, int inject, bool commit) {
  const sr::Workload& w = S.w;
  const sr::ResidencySwitches sw;
  sr::TickPlan p;
  ++R.ticks;
  S.res.observe(w, E, sw, &tl, &p);
  const sr::ArenaLayout& at = p.at;
  if (p.reorder_due) {  // durations by a fixed rule: the list moves
    std::vector<uint32_t> cycles(w.cand_global.size());
    for (size_t k = 0; k < cycles.size(); ++k) cycles[k] = static_cast<uint32_t>((k * 2654435761u) >> 8);
    sr::reorder_list_by_cost(S.w, cycles.data(), E.list_head, 64);
    ++R.reorders;
  }
  const bool st_moved = grow(S.H, at.bytes, inject & 1), ar_moved = grow(S.D, at.bytes, inject & 2);
  const size_t t_bytes = (static_cast<size_t>(w.n_classes) + w.t_dim.size()) * w.Wp * 8;
  const bool tb_moved = t_bytes > S.tables_cap || (inject & 4);
  if (tb_moved) S.tables_cap = std::max(t_bytes, S.tables_cap) + t_bytes / 4, S.tables_valid = false;
  R.staging += (inject & 1) != 0, R.arena += (inject & 2) != 0, R.tables += (inject & 4) != 0;
  S.res.resolve(w, E, sw, st_moved, ar_moved, tb_moved, p.reorder_due, S.H.data(), &tl, &p);
  // A: the staging arena is current
  const char* H = S.H.data();
  if (long i = first_diff(H, at.node_rec, E.node_rec); i >= 0) R.fail("A staging", "node_rec", i);
  if (long i = first_diff(H, at.node_free, E.node_free); i >= 0) R.fail("A staging", "node_free", i);
  if (long i = first_diff(H, at.pod_rec, w.pod_rec); i >= 0) R.fail("A staging", "pod_rec", i);
  check_sections(R, "A staging", H, at, w, tl, true);
  // the copies; E: bytes_uploaded counts them
  uint64_t counted = 0;
  for (const sr::ArenaCopy& c : tl.copies) {
    if (c.off + c.bytes > at.bytes) R.fail("copy", "out of the arena", static_cast<long>(c.off));
    else std::memcpy(S.D.data() + c.off, H + c.off, c.bytes);
    counted += c.counted ? c.bytes : 0;
  }
  if (tl.copies.size() > sr::kAtomRowCopies + 5) R.fail("copy", "list longer than its bound", static_cast<long>(tl.copies.size()));
  if (counted != p.bytes_uploaded) R.fail("E bytes_uploaded", "sum of the counted copies", static_cast<long>(counted));
  S.res.upload_queued(w, p);
  if (w.list.size() / 4 > 1024 && S.res.want_cost(w)) S.res.cost_queued(w);  // (sr_ctx::list_cost_min)
  if (!commit) {  // prepared, never run: no K0, no commit
    ++R.uncommitted;
    return;
  }
  char* D = S.D.data();
  uint64_t* d_rec = reinterpret_cast<uint64_t*>(D + at.node_rec);
  int64_t* d_free = reinterpret_cast<int64_t*>(D + at.node_free);
  uint64_t* d_pod = reinterpret_cast<uint64_t*>(D + at.pod_rec);
  const uint64_t* d_np = reinterpret_cast<const uint64_t*>(D + at.node_patch);
  const size_t NP = static_cast<size_t>(w.n_pad);
  auto node_differs = [&](size_t n, const uint64_t* rec, const int64_t* fr) {
    bool x = std::memcmp(rec + n * 8, &E.node_rec[n * 8], 64) != 0;
    for (size_t dm = 0; dm < 3; ++dm) x = x || fr[dm * NP + n] != E.node_free[dm * NP + n];
    return x;
  };
  if (p.skip) {  // C: a K0-less run
    ++R.skip;
    if (S.res.class_flip) R.fail("C K0-less", "class_flip", 0);
    if (!S.tables_valid || S.t_atoms != w.atoms) R.fail("C K0-less", "atoms against the last K0 commit", 0);
    check_sections(R, "C K0-less device", D, at, w, tl, true);
    for (size_t n = 0; n < NP; ++n) {
      if (!node_differs(n, d_rec, d_free)) continue;
      bool in_patch = false, in_args = false;
      for (int32_t k = 0; k < p.n_node_patch; ++k) in_patch = in_patch || d_np[k * sr::kNodePatchWords] == n;
      for (int32_t k = 0; k < p.n_dirty; ++k) in_args = in_args || static_cast<size_t>(p.dirty_node[k]) == n;
      if (!in_patch || !in_args) R.fail("C K0-less device", "node not in the patches / kernel arguments", static_cast<long>(n));
    }
    for (int32_t k = 0; k < p.n_node_patch; ++k) {  // the patches K2 reads are the current records
      const size_t n = d_np[k * sr::kNodePatchWords];
      if (std::memcmp(d_np + k * sr::kNodePatchWords + 1, &E.node_rec[n * 8], 64) != 0) R.fail("C K0-less", "patch record", static_cast<long>(n));
    }
    for (size_t i = 0; i < w.pod_rec.size(); ++i) {
      if (d_pod[i] == w.pod_rec[i]) continue;
      const size_t q = i / 6;
      if (i % 6 < 4 || std::find(S.res.pending.begin(), S.res.pending.end(), static_cast<int32_t>(q)) == S.res.pending.end())
        R.fail("C K0-less device", "pod_rec", static_cast<long>(i));
    }
    return;
  }
  // a K0 run: D, the incremental lists against the tables' model (before K0 writes)
  if (p.k0_inc) {
    ++R.inc;
    if (!S.tables_valid || S.t_thr.size() != w.t_thr.size() || S.t_atoms.size() != w.atoms.size()) {
      R.fail("D incremental K0", "no tables of this shape", 0);
    } else {
      auto has_col = [&](size_t col) { return std::binary_search(tl.k0_cols.begin(), tl.k0_cols.end(), static_cast<int32_t>(col)); };
      for (size_t n = 0; n < NP; ++n)
        if (node_differs(n, S.t_node_rec.data(), S.t_node_free.data()) && !has_col(n >> 6)) R.fail("D incremental K0", "node's column", static_cast<long>(n));
      for (size_t i = 0; i < w.atoms.size(); ++i)
        if (w.atoms[i] != S.t_atoms[i] && !has_col(i % w.Wp)) R.fail("D incremental K0", "atom word's column", static_cast<long>(i));
      for (size_t r = 0; r < w.t_thr.size(); ++r)
        if (w.t_thr[r] != S.t_thr[r] && w.t_thr[r] != sr::kTSpare &&
            std::find(tl.k0_rows.begin(), tl.k0_rows.end(), static_cast<int32_t>(r)) == tl.k0_rows.end())
          R.fail("D incremental K0", "T row", static_cast<long>(r));
    }
  } else {
    ++R.full;
  }
  // what k0_common does with the patches
  for (int32_t k = 0; k < p.n_node_patch; ++k) {
    const uint64_t* e = d_np + k * sr::kNodePatchWords;
    std::memcpy(d_rec + e[0] * 8, e + 1, 64);
    for (size_t dm = 0; dm < 3; ++dm) d_free[dm * NP + e[0]] = static_cast<int64_t>(e[9 + dm]);
  }
  const uint64_t* d_pp = reinterpret_cast<const uint64_t*>(D + at.pod_patch);
  for (int32_t k = 0; k < p.n_pod_patch; ++k) {
    d_pod[d_pp[k * 3] * 6 + 4] = d_pp[k * 3 + 1];
    d_pod[d_pp[k * 3] * 6 + 5] = d_pp[k * 3 + 2];
  }
  // B: after K0 the device arena is current
  if (long i = first_diff(D, at.node_rec, E.node_rec); i >= 0) R.fail("B device", "node_rec", i);
  if (long i = first_diff(D, at.node_free, E.node_free); i >= 0) R.fail("B device", "node_free", i);
  if (long i = first_diff(D, at.pod_rec, w.pod_rec); i >= 0) R.fail("B device", "pod_rec", i);
  check_sections(R, "B device", D, at, w, tl, true);
  S.res.k0_queued(w);
  S.tables_valid = true;
  S.t_node_rec = E.node_rec, S.t_node_free = E.node_free, S.t_atoms = w.atoms, S.t_thr = w.t_thr;
}

// Ticks of fresh snapshots (pods added one at a time, in bursts, all removed
// again; every fourth group of four ticks the spot order moves), each planned
// for two inputs on two slots over one encoder: a 16-candidate prefix, then
// every candidate, as sr_plan_first does.  By tick number: a prepare that is
// never run, each allocation moved once, a failing encode.
int residency_check(Cluster& K, int ticks, int burst) {
  sr::EncoderCache cache;
  sr::TickLists tl;
  ModelSlot slot[2];
  Residual R;
  std::string err;
  std::vector<std::pair<int32_t, int32_t>> extra;
  uint64_t x = 0x9E3779B97F4A7C15ull;
  auto rnd = [&](uint64_t n) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x % n; };
  sr_cluster& c = K.c;
  const int32_t n_prefix = std::min(16, K.nod);
  sr_candidates input[2] = {{n_prefix, K.coff.data(), K.cp.data(), nullptr}, {K.nod, K.coff.data(), K.cp.data(), nullptr}};
  for (int r = 0; r < ticks && !K.cp.empty(); ++r) {
    R.tick = r;
    if (r % 16 >= 12) {  // pods on spot nodes change their cpu request: NewNodeMap re-sorts the spot list
      for (int k = 0, nk = 1 + static_cast<int>(rnd(3)); k < nk; ++k) {
        const int32_t node = K.spot[rnd(static_cast<uint64_t>(K.ns))];
        if (K.off[node + 1] == K.off[node]) continue;
        const int32_t pod = K.idx[K.off[node] + static_cast<int32_t>(rnd(static_cast<uint64_t>(K.off[node + 1] - K.off[node])))];
        const int64_t d = static_cast<int64_t>(rnd(400)) - 150;
        auto bump = [&](const int64_t* a) { const_cast<int64_t*>(a)[pod] = std::max<int64_t>(0, a[pod] + d); };
        bump(c.pods.cpu_sort_milli);
        bump(c.pods.req_milli_cpu);
        if (c.acc_milli_cpu) bump(c.acc_milli_cpu);
        const_cast<uint64_t*>(c.pod_stamp)[pod] = (x | 1);
      }
      std::vector<int32_t> before(K.spot.begin(), K.spot.begin() + K.ns);
      if (sr_new_node_map(&c, &K.prm, &K.m) != SR_OK) return 1;
      R.moved += !std::equal(before.begin(), before.end(), K.spot.begin());
    }
    sr_snapshot* s2 = nullptr;
    sr_snapshot_create(&c, K.spot.data(), K.ns, K.off.data(), K.idx.data(), &s2);
    if (r % 9 == 8) extra.clear();
    const int add = r % 5 == 4 ? burst : r % 7 == 3 ? 0 : 1 + static_cast<int>(rnd(3));  // a burst, a quiet tick, a few
    for (int a = 0; a < add; ++a)
      extra.emplace_back(K.cp[rnd(K.cp.size())], static_cast<int32_t>(rnd(static_cast<uint64_t>(K.ns))));
    for (auto& e : extra) sr_snapshot_add_pod(s2, &c, e.first, e.second);
    for (int i = 0; i < 2; ++i) {
      ModelSlot& S = slot[i];
      if (r == 22 && i == 1) {  // an encode that fails (offsets not monotone)
        std::vector<int32_t> bad_off(K.coff.begin(), K.coff.begin() + K.nod + 1);
        int32_t k = 1;
        while (k + 1 < K.nod && bad_off[k] == bad_off[k + 1]) ++k;
        if (k + 1 < K.nod) std::swap(bad_off[k], bad_off[k + 1]);  // (the ends stay: the pod count is the same)
        sr_candidates bad{K.nod, bad_off.data(), K.cp.data(), nullptr};
        if (k + 1 < K.nod && sr::encode_workload(&cache, s2, &c, &bad, &S.w, &err) != SR_OK) {
          S.res.encode_failed();
          ++R.enc_errors;
          continue;
        }
      }
      if (sr::encode_workload(&cache, s2, &c, &input[i], &S.w, &err) != SR_OK) {
        printf("encode failed: %s\n", err.c_str());
        return 1;
      }
      const int inject = i == 1 ? (r == 18 ? 1 : r == 10 ? 2 : r == 14 ? 4 : 0) : 0;
      residency_tick(R, S, cache, tl, inject, !(r == 6 && i == 1));
    }
    sr_snapshot_destroy(s2);
  }
  printf("residency check: %d ticks (%d full K0, %d incremental, %d K0-less), never run %d, arena moved %d, "
         "tables moved %d, staging moved %d, list reorders %d, encode errors %d, spot order moved %d, violations %d\n",
         R.ticks, R.full, R.inc, R.skip, R.uncommitted, R.arena, R.tables, R.staging, R.reorders, R.enc_errors, R.moved,
         R.bad);
  return R.bad ? 2 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  sr_synth_params p{};
  p.config = argc > 1 ? atoi(argv[1]) : 3;
  p.pinned_fraction = -1;
  const bool realistic = std::getenv("SR_SYNTH_REALISTIC") != nullptr;
  if (realistic) {  // bench --variant realistic (spotplanner/synth.py REALISTIC)
    p.stateful_fraction = 0.15;
    p.init_fraction = 0.2;
    p.gpu_fraction = 0.3;
  }
  const bool affinity = std::getenv("SR_SYNTH_AFFINITY") != nullptr;
  if (affinity) {  // bench --variant affinity (spotplanner/synth.py AFFINITY)
    p.anti_fraction = 0.10;
    p.spread_fraction = 0.10;
  }
  sr_synth* s = sr_synth_generate(&p);
  sr_cluster c;
  sr_synth_view(s, &c);
  sr_node_label od, sp;
  sr_synth_labels(s, &od, &sp);
  const int nn = c.nodes.n, np = c.pods.n;
  std::vector<int32_t> spot(nn), odn(nn), off(nn + 1), idx(np);
  std::vector<int64_t> req(nn), fr(nn);
  int32_t ns = 0, nod = 0;
  sr_node_map m{spot.data(), &ns, odn.data(), &nod, off.data(), idx.data(), req.data(), fr.data()};
  sr_node_map_params prm{od, sp, 0};
  auto t0 = std::chrono::steady_clock::now();
  if (sr_new_node_map(&c, &prm, &m) != SR_OK) return 1;
  const double ms_map = ms_since(t0);
  sr_snapshot* snap = nullptr;
  t0 = std::chrono::steady_clock::now();
  sr_snapshot_create(&c, spot.data(), ns, off.data(), idx.data(), &snap);
  const double ms_snap = ms_since(t0);
  std::vector<int32_t> coff{0}, cp;
  const int max_cands = argc > 2 ? atoi(argv[2]) : nod;
  if (max_cands < nod) nod = max_cands;
  for (int i = 0; i < nod; ++i) {
    int node = odn[i];
    for (int j = off[node]; j < off[node + 1]; ++j)
      if (!(c.pods.flags[idx[j]] & (SR_POD_MIRROR | SR_POD_DAEMONSET_CONTROLLER))) cp.push_back(idx[j]);
    coff.push_back(cp.size());
  }
  sr_candidates cands{nod, coff.data(), cp.data(), nullptr};
  sr::Workload w;
  sr::EncoderCache cache;
  std::string err;
  printf("config %d: nodes %d pods %d spot %d od %d cand_pods %zu\n", p.config, nn, np, ns, nod, cp.size());
  printf("new_node_map %.2f ms, snapshot %.2f ms\n", ms_map, ms_snap);
  t0 = std::chrono::steady_clock::now();
  if (sr::encode_workload(&cache, snap, &c, &cands, &w, &err) != SR_OK) {
    printf("encode failed: %s\n", err.c_str());
    return 1;
  }
  printf("cold encode %.3f ms (new specs %d, memo hits %d)\n", ms_since(t0), cache.last_new_specs, cache.last_memo_hits);
  phases("cold");
  double best = 1e30;
  for (int r = 0; r < 20; ++r) {
    t0 = std::chrono::steady_clock::now();
    sr::encode_workload(&cache, snap, &c, &cands, &w, &err);
    best = std::min(best, ms_since(t0));
  }
  printf("warm encode (same snapshot) best %.3f ms\n", best);
  phases("warm");
  // one spot node changed: a fresh snapshot (as every tick builds) with one
  // more pod on spot position 7
  best = 1e30;
  int last_state = 0, last_static = 0;
  for (int r = 0; r < 10; ++r) {
    sr_snapshot* s2 = nullptr;
    sr_snapshot_create(&c, spot.data(), ns, off.data(), idx.data(), &s2);
    if (r & 1) sr_snapshot_add_pod(s2, &c, cp.empty() ? 0 : cp[0], std::min(7, ns - 1));
    t0 = std::chrono::steady_clock::now();
    sr::encode_workload(&cache, s2, &c, &cands, &w, &err);
    best = std::min(best, ms_since(t0));
    last_state = cache.last_state_changed;
    last_static = cache.last_static_changed;
    sr_snapshot_destroy(s2);
  }
  printf("one-node-changed encode (fresh snapshot) best %.3f ms (state nodes %d, static rebuilt %d, memo hits %d, "
         "reused %d, pod patches %d)\n", best, last_state, last_static, cache.last_memo_hits, cache.last_reused,
         cache.last_pod_patches);
  phases("1node");
  const bool check_perm = argc > 3 && std::string(argv[3]) == "check-perm";
  if (argc > 3 && (std::string(argv[3]) == "check" || check_perm)) {
    // the state view patched node by node equals the one rebuilt from scratch:
    // consecutive fresh snapshots, each with a few more pods on random spot nodes
    std::vector<std::pair<int32_t, int32_t>> extra;
    uint64_t x = 88172645463325252ull;
    auto rnd = [&](uint64_t n) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x % n; };
    int ticks = 0, patched = 0;
    int moved_ticks = 0;
    for (int r = 0; r < 300 && !cp.empty(); ++r) {
      if (check_perm && r > 0) {  // pods on spot nodes change cpu requests: the spot order moves
        for (int k = 0, nk = 1 + static_cast<int>(rnd(3)); k < nk; ++k) {
          const int32_t node = spot[rnd(static_cast<uint64_t>(ns))];
          if (off[node + 1] == off[node]) continue;
          const int32_t pod = idx[off[node] + static_cast<int32_t>(rnd(static_cast<uint64_t>(off[node + 1] - off[node])))];
          const int64_t d = static_cast<int64_t>(rnd(400)) - 150;
          auto bump = [&](const int64_t* a) { const_cast<int64_t*>(a)[pod] = std::max<int64_t>(0, a[pod] + d); };
          bump(c.pods.cpu_sort_milli);
          bump(c.pods.req_milli_cpu);
          if (c.acc_milli_cpu) bump(c.acc_milli_cpu);
          const_cast<uint64_t*>(c.pod_stamp)[pod] = (x | 1);
        }
        std::vector<int32_t> before(spot.begin(), spot.begin() + ns);
        if (sr_new_node_map(&c, &prm, &m) != SR_OK) return 1;
        moved_ticks += !std::equal(before.begin(), before.end(), spot.begin());
      }
      sr_snapshot* s2 = nullptr;
      sr_snapshot_create(&c, spot.data(), ns, off.data(), idx.data(), &s2);
      if (r % 7 == 6) extra.clear();  // sometimes the extra pods leave again
      const int add = 1 + static_cast<int>(rnd(3));
      for (int a = 0; a < add; ++a)
        extra.emplace_back(cp[rnd(cp.size())], static_cast<int32_t>(rnd(static_cast<uint64_t>(ns))));
      for (auto& e : extra) sr_snapshot_add_pod(s2, &c, e.first, e.second);
      sr::encode_workload(&cache, s2, &c, &cands, &w, &err);
      patched += cache.patched_from != ~0ull;
      sr::EncoderCache fresh;
      sr::Workload w2;
      sr::encode_workload(&fresh, s2, &c, &cands, &w2, &err);
      for (int d = 0; d < 3; ++d)
        if (cache.sorted_free[d] != fresh.sorted_free[d] || cache.node_vals[d] != fresh.node_vals[d]) {
          printf("views differ at tick %d, dimension %d\n", r, d);
          return 2;
        }
      if (cache.node_rec != fresh.node_rec || cache.node_free != fresh.node_free ||
          cache.podcount_row != fresh.podcount_row) {
        printf("node records differ at tick %d\n", r);
        return 2;
      }
      sr_snapshot_destroy(s2);
      ++ticks;
    }
    printf("state views consistent: %d ticks (%d patched node by node, spot order moved %d)\n", ticks, patched,
           moved_ticks);
  }
  const bool perm = argc > 3 && std::string(argv[3]) == "reuse-perm";
  const bool scal = argc > 3 && std::string(argv[3]) == "reuse-scalar";
  if (argc > 3 && (std::string(argv[3]) == "reuse" || perm || scal)) {
    // candidate-side reuse: every tick a fresh snapshot with a few more (or
    // fewer) pods on random spot nodes and the same candidate input; the
    // reused workload must plan like one encoded from scratch: same atoms,
    // programs and requests, per pod the same dead flag, class and threshold
    // per dimension
    std::vector<std::pair<int32_t, int32_t>> extra;
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&](uint64_t n) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x % n; };
    const int ticks = argc > 4 ? atoi(argv[4]) : 200;
    const int burst = argc > 5 ? atoi(argv[5]) : 24;  // pods added every fifth tick (many new free values)
    int reused = 0, full = 0, bad = 0;
    long patches = 0;
    double ms_reuse = 0, ms_views = 0;
    int permuted = 0, flips = 0;
    // reuse-scalar: a candidate pod listing one extended resource (no volume
    // limit key) and, per spot node allocating that name, enough copies of it
    // to exceed the allocatable
    std::vector<std::pair<int32_t, int32_t>> fill;
    if (scal && c.pod_scalar_off && c.node_scalar_off) {
      int32_t gp = -1, name = 0;
      int64_t rq = 0;
      for (int32_t q : cp) {
        const int32_t b = c.pod_scalar_off[q], e = c.pod_scalar_off[q + 1];
        bool ok = e > b;
        for (int32_t i = b; i < e && ok; ++i) ok = c.pod_scalar_name[i] >= 0 && c.pod_scalar_acc[i] > 0;
        if (c.volumes) ok = ok && c.volumes->att_off[q] == c.volumes->att_off[q + 1];
        if (ok) { gp = q; name = c.pod_scalar_name[b]; rq = c.pod_scalar_acc[b]; break; }
      }
      for (int32_t k = 0; gp >= 0 && k < ns; ++k)
        for (int32_t i = c.node_scalar_off[spot[k]]; i < c.node_scalar_off[spot[k] + 1]; ++i)
          if (c.node_scalar_name[i] == name)
            for (int64_t u = 0; u <= c.node_scalar_alloc[i] / rq; ++u) fill.emplace_back(gp, k);
      printf("reuse-scalar: pod %d fills %zu slots\n", gp, fill.size());
      if (fill.empty()) return 3;
    }
    // the pods added at random: in reuse-scalar mode only pods without
    // attachable volumes (a candidate's attachable volume on a spot node sends
    // it to the reference path, and such a fallback ends the reuse)
    std::vector<int32_t> pool;
    for (int32_t q : cp) {
      bool ok = true;
      if (scal && c.pod_scalar_off)
        for (int32_t i = c.pod_scalar_off[q]; i < c.pod_scalar_off[q + 1] && ok; ++i) ok = c.pod_scalar_name[i] >= 0;
      if (scal && c.volumes) ok = ok && c.volumes->att_off[q] == c.volumes->att_off[q + 1];
      if (ok) pool.push_back(q);
    }
    for (int r = 0; r < ticks && !pool.empty(); ++r) {
      if (perm && r > 0) {
        // reuse-perm: pods on spot nodes change their cpu request (and stamp):
        // NewNodeMap re-sorts the spot list, the snapshot follows its order
        for (int k = 0, nk = 1 + static_cast<int>(rnd(3)); k < nk; ++k) {
          const int32_t node = spot[rnd(static_cast<uint64_t>(ns))];
          if (off[node + 1] == off[node]) continue;
          const int32_t pod = idx[off[node] + static_cast<int32_t>(rnd(static_cast<uint64_t>(off[node + 1] - off[node])))];
          const int64_t d = static_cast<int64_t>(rnd(400)) - 150;
          auto bump = [&](const int64_t* a) { const_cast<int64_t*>(a)[pod] = std::max<int64_t>(0, a[pod] + d); };
          bump(c.pods.cpu_sort_milli);
          bump(c.pods.req_milli_cpu);
          if (c.acc_milli_cpu) bump(c.acc_milli_cpu);
          const_cast<uint64_t*>(c.pod_stamp)[pod] = (x | 1);
        }
        std::vector<int32_t> before(spot.begin(), spot.begin() + ns);
        if (sr_new_node_map(&c, &prm, &m) != SR_OK) return 1;
        permuted += !std::equal(before.begin(), before.end(), spot.begin());
      }
      sr_snapshot* s2 = nullptr;
      sr_snapshot_create(&c, spot.data(), ns, off.data(), idx.data(), &s2);
      if (r % 9 == 8) extra.clear();
      const int add = r % 5 == 4 ? burst : 1 + static_cast<int>(rnd(3));  // sometimes a burst: many new free values
      for (int a = 0; a < add; ++a)
        extra.emplace_back(pool[rnd(pool.size())], static_cast<int32_t>(rnd(static_cast<uint64_t>(ns))));
      for (auto& e : extra) sr_snapshot_add_pod(s2, &c, e.first, e.second);
      if (scal && r % 6 >= 2 && r % 6 < 4)
        for (auto& e : fill) sr_snapshot_add_pod(s2, &c, e.first, e.second);
      // the realistic variant compares with a full encode by a copy of the
      // encoder as it was before this call: its class and atom numbering
      // depends on the dictionaries' history (scalar and volume queries)
      std::unique_ptr<sr::EncoderCache> twin;
      if (realistic || affinity) twin.reset(new sr::EncoderCache(cache));
      t0 = std::chrono::steady_clock::now();
      if (sr::encode_workload(&cache, s2, &c, &cands, &w, &err) != SR_OK) return 1;
      const double ms = ms_since(t0);
      if (cache.last_reused) {
        ++reused;
        flips += w.class_flip;
        patches += cache.last_pod_patches;
        ms_reuse += ms;
        ms_views += sr::encode_phase_ms[0];
      } else {
        ++full;
      }
      sr::EncoderCache fresh;
      sr::Workload f;
      if (sr::encode_workload(twin ? twin.get() : &fresh, s2, &c, &cands, &f, &err) != SR_OK) return 1;
      auto fail = [&](const char* what, long i) {
        if (bad++ < 5) printf("tick %d (reused %d): %s differs at %ld\n", r, cache.last_reused, what, i);
      };
      if (w.atoms != f.atoms) {
        long a = 0;
        while (a < f.n_atoms && std::equal(f.atoms.begin() + a * f.Wp, f.atoms.begin() + (a + 1) * f.Wp, w.atoms.begin() + a * f.Wp)) ++a;
        fail("atoms", a);
      }
      if (w.sp_tab != f.sp_tab) fail("spread tables", 0);
      if (w.dyn_cand != f.dyn_cand || w.dyn_pod != f.dyn_pod || w.dk_dom != f.dk_dom) fail("domain path", 0);
      if (w.pod_src != f.pod_src || w.cand_off != f.cand_off || w.list != f.list || w.status_host != f.status_host)
        fail("candidate lists", 0);
      const int32_t nb = f.empty_class >= 0 ? f.empty_class : f.n_classes;  // classes before the empty one
      if (w.cls_prog_off.size() < static_cast<size_t>(nb) + 1 ||
          !std::equal(f.cls_prog_off.begin(), f.cls_prog_off.begin() + nb + 1, w.cls_prog_off.begin()) ||
          !std::equal(f.cls_prog.begin(), f.cls_prog.begin() + f.cls_prog_off[nb], w.cls_prog.begin()))
        fail("class programs", 0);
      auto thr = [](const sr::Workload& v, int32_t row) { return row == 0 ? INT64_MIN : v.t_thr[row]; };
      for (size_t q = 0; q < f.pod_src.size(); ++q) {
        const int32_t* a = &w.pod_rows[q * 4];
        const int32_t* b = &f.pod_rows[q * 4];
        const bool da = a[0] == w.empty_class, db = b[0] == f.empty_class;
        if (da != db || (!da && a[0] != b[0])) fail("class", static_cast<long>(q));
        for (int d = 0; d < 3 && !da; ++d)
          if (thr(w, a[1 + d]) != thr(f, b[1 + d]) || w.t_dim[a[1 + d]] != f.t_dim[b[1 + d]]) fail("threshold", static_cast<long>(q));
        for (int k = 0; k < 4; ++k)
          if (w.pod_rec[q * 6 + k] != f.pod_rec[q * 6 + k]) fail("request words", static_cast<long>(q));
        const uint64_t Wp64 = static_cast<uint64_t>(w.Wp);
        if (w.pod_rec[q * 6 + 4] != (static_cast<uint64_t>(a[0]) * Wp64 | static_cast<uint64_t>(w.n_classes + a[1]) * Wp64 << 32) ||
            w.pod_rec[q * 6 + 5] != (static_cast<uint64_t>(w.n_classes + a[2]) * Wp64 |
                                     static_cast<uint64_t>(w.n_classes + a[3]) * Wp64 << 32))
          fail("row words", static_cast<long>(q));
      }
      sr_snapshot_destroy(s2);
    }
    printf("reuse check: %d ticks (%d reused, %d full), %ld pod patches, reuse encode avg %.3f ms (views %.3f), "
           "spot order moved %d, class flips %d, mismatches %d\n", reused + full, reused, full, patches,
           reused ? ms_reuse / reused : 0.0, reused ? ms_views / reused : 0.0, permuted, flips, bad);
    if (bad) return 2;
  }
  if (argc > 3 && std::string(argv[3]) == "residency") {
    Cluster K{c, prm, m, spot, off, idx, ns, coff, cp, nod};
    const int rc = residency_check(K, argc > 4 ? atoi(argv[4]) : 60, argc > 5 ? atoi(argv[5]) : 24);
    if (rc) return rc;
  }
  printf("Wp %d atoms %d classes %d program ops %zu t_rows %zu\n", w.Wp, w.n_atoms, w.n_classes, w.cls_prog.size(),
         w.t_dim.size());
  int tc[4] = {0, 0, 0, 0};
  for (int d : w.t_dim) tc[d]++;
  printf("t rows: cpu %d mem %d eph %d all %d; max cand pods %d\n", tc[0], tc[1], tc[2], tc[3], w.max_cand_pods);
  sr_snapshot_destroy(snap);
  sr_synth_destroy(s);
  return 0;
}
