// seq_pdb_check — the serial rule of sr_plan_sequence_pdb on random lists.
//
// Host only.  Candidates here have an outcome that does not depend on the
// snapshot (no pods / reference path / drains / fails), which leaves exactly
// what csrc/seq_pdb.cpp decides: needs, refusals, the stop and the commits.
// The planner's rounds (pdb_round + commit, as planner.cpp and seq_pdb.hip
// run them) are compared with a second, naive implementation of the pass that
// walks the candidates one by one and counts pods per group from the
// caller's arrays, without the need CSR.
//
//   seq_pdb_check [lists] [seed]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "seq_pdb.hpp"

namespace {

constexpr int32_t kOk = -1, kFallback = -2, kEmpty = -3, kSkipped = -4, kPdb = -5, kFailed = 0;
enum { kEnd = 0, kBudget = 1, kStopFallback = 2 };

struct Pass {
  std::vector<int32_t> status, drained, remaining;
  int32_t stop = kEnd, stop_cand = -1, rounds = 0;
  int32_t by_last_need = 0;  // (naive) refusals of a candidate with several needs that only its last need decides
  bool operator==(const Pass& o) const {
    return status == o.status && drained == o.drained && remaining == o.remaining && stop == o.stop &&
           stop_cand == o.stop_cand;
  }
};

struct List {
  std::vector<int32_t> off, pod_group, allowed;
  std::vector<uint8_t> kind;
  int32_t first = 0, max_drains = 1;
};

// The pass as the header states it, one candidate at a time.
Pass naive(const List& in) {
  const int32_t n = static_cast<int32_t>(in.kind.size()), base = in.off[0];
  Pass r;
  r.status.assign(n, kSkipped);
  r.remaining = in.allowed;
  for (int32_t c = in.first; c < n; ++c) {
    if (in.off[c + 1] == in.off[c]) {
      r.status[c] = kEmpty;
      continue;
    }
    // (groups ascending, as the needs of the CSR: the last group with pods is the candidate's last need)
    int32_t needs = 0, over = 0;
    bool last_over = false;
    for (size_t g = 0; g < in.allowed.size(); ++g) {
      int32_t need = 0;
      for (int32_t q = in.off[c] - base; q < in.off[c + 1] - base; ++q) need += in.pod_group[q] == static_cast<int32_t>(g);
      if (need == 0) continue;
      last_over = need > r.remaining[g];
      needs += 1;
      over += last_over;
    }
    if (over > 0) {
      r.status[c] = kPdb;
      r.by_last_need += needs > 1 && over == 1 && last_over;
      continue;
    }
    if (in.kind[c] == sr::kPdbFallback) {
      r.status[c] = kFallback;
      r.stop = kStopFallback;
      r.stop_cand = c;
      return r;
    }
    if (in.kind[c] == sr::kPdbFails) {
      r.status[c] = kFailed;
      continue;
    }
    r.status[c] = kOk;
    for (int32_t q = in.off[c] - base; q < in.off[c + 1] - base; ++q)
      if (in.pod_group[q] >= 0) r.remaining[in.pod_group[q]] -= 1;
    r.drained.push_back(c);
    if (static_cast<int32_t>(r.drained.size()) == in.max_drains) {
      r.stop = kBudget;
      return r;
    }
  }
  return r;
}

// The planner's loop: rounds over the list, the refused set fixed per round.
Pass rounds(const List& in) {
  const int32_t n = static_cast<int32_t>(in.kind.size());
  Pass r;
  r.status.assign(n, kSkipped);
  sr::PdbLedger l;
  sr::pdb_build(n, in.off.data(), static_cast<int32_t>(in.allowed.size()), in.allowed.data(), in.pod_group.data(), &l);
  // a candidate without pods is kPdbEmpty whatever the generator drew
  std::vector<uint8_t> kind = in.kind;
  for (int32_t c = 0; c < n; ++c)
    if (in.off[c + 1] == in.off[c]) kind[c] = sr::kPdbEmpty;
  int32_t cursor = in.first - 1;
  for (;;) {
    int32_t next = cursor + 1;
    while (next < n && kind[next] == sr::kPdbEmpty) r.status[next++] = kEmpty;
    if (next >= n) break;
    const sr::PdbRound rd = sr::pdb_round(l, kind.data(), n, cursor);
    r.rounds += rd.live ? 1 : 0;
    for (int32_t i = cursor + 1; i <= rd.end; ++i)
      r.status[i] = kind[i] == sr::kPdbEmpty ? kEmpty : l.refused(i) ? kPdb : kind[i] == sr::kPdbDrains ? kOk : kFailed;
    if (rd.winner < 0) {
      if (rd.stop >= 0) {
        r.status[rd.stop] = kFallback;
        r.stop = kStopFallback;
        r.stop_cand = rd.stop;
      }
      break;
    }
    l.commit(rd.winner);
    r.drained.push_back(rd.winner);
    cursor = rd.winner;
    if (static_cast<int32_t>(r.drained.size()) == in.max_drains) {
      r.stop = kBudget;
      break;
    }
  }
  r.remaining = l.remaining;
  return r;
}

// Three candidates of m pods, pod k in group k; every group allows two evictions, the last one only one.  The
// first candidate is accepted with its last need exactly at the allowance and commits m needs; the other two
// meet m - 1 needs that still hold and are refused by the last one alone.
bool many_needs_case(int m) {
  List in;
  in.off = {3, 3 + m, 3 + 2 * m, 3 + 3 * m};
  in.kind.assign(3, sr::kPdbDrains);
  for (int c = 0; c < 3; ++c)
    for (int k = 0; k < m; ++k) in.pod_group.push_back(k);
  in.allowed.assign(static_cast<size_t>(m), 2);
  in.allowed.back() = 1;
  in.max_drains = 1 << 30;
  const Pass a = naive(in), b = rounds(in);
  std::vector<int32_t> left(static_cast<size_t>(m), 1);
  left.back() = 0;
  return a == b && b.status == std::vector<int32_t>{kOk, kPdb, kPdb} && b.drained == std::vector<int32_t>{0} &&
         b.remaining == left && b.stop == kEnd && b.rounds == 1 && a.by_last_need == 2;
}

int fail(const char* what, uint32_t seed, int i) {
  std::fprintf(stderr, "seq_pdb_check: %s (seed %u, list %d)\n", what, seed, i);
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  const int lists = argc > 1 ? std::atoi(argv[1]) : 20000;
  const uint32_t seed = argc > 2 ? static_cast<uint32_t>(std::strtoul(argv[2], nullptr, 10)) : 1u;
  std::mt19937 rng(seed);
  auto pick = [&](int lo, int hi) { return lo + static_cast<int>(rng() % static_cast<uint32_t>(hi - lo + 1)); };
  long refusals = 0, drains = 0, stops = 0, passed_fallbacks = 0, n_rounds = 0, by_last_need = 0;
  for (int i = 0; i < lists; ++i) {
    List in;
    const int n = pick(0, 40), groups = pick(1, 8);
    in.off.push_back(pick(0, 5));  // (a list that does not start at pod 0)
    for (int c = 0; c < n; ++c) {
      const int np = pick(0, 4) == 0 ? 0 : pick(1, 6);
      in.off.push_back(in.off.back() + np);
      const int k = pick(0, 9);
      in.kind.push_back(k == 0 ? sr::kPdbFallback : k < 6 ? sr::kPdbDrains : sr::kPdbFails);
      const int home = pick(0, groups - 1);  // most pods of a candidate share a group, as replicas do
      for (int q = 0; q < np; ++q) in.pod_group.push_back(pick(0, 3) == 0 ? -1 : pick(0, 2) ? home : pick(0, groups - 1));
    }
    for (int g = 0; g < groups; ++g) in.allowed.push_back(pick(0, 6));
    in.first = pick(0, 3) ? 0 : pick(0, n);
    in.max_drains = pick(0, 2) ? 1 << 30 : pick(1, 5);
    if (sr::pdb_validate(groups, in.allowed.data(), in.pod_group.data(), static_cast<int64_t>(in.pod_group.size())))
      return fail("a valid list was rejected", seed, i);
    const Pass a = naive(in), b = rounds(in);
    if (!(a == b)) return fail("the rounds differ from the serial pass", seed, i);
    if (b.rounds > static_cast<int32_t>(b.drained.size()) + 1) return fail("an empty round", seed, i);
    for (int32_t x : b.remaining)
      if (x < 0) return fail("a negative allowance", seed, i);
    for (int c = 0; c < n; ++c) {
      refusals += a.status[c] == kPdb;
      passed_fallbacks += a.status[c] == kPdb && in.kind[c] == sr::kPdbFallback;
    }
    drains += static_cast<long>(a.drained.size());
    stops += a.stop == kStopFallback;
    n_rounds += b.rounds;
    by_last_need += a.by_last_need;
  }
  for (int m : {2, 64, 65, 300, 1025})
    if (!many_needs_case(m)) return fail("many needs, decided by the last one", seed, -m);
  // the argument rules
  const int32_t allowed[2] = {1, 0}, neg[2] = {1, -1}, group[3] = {0, -1, 1}, high[3] = {0, 2, 1}, low[3] = {0, -2, 1};
  bool ok = !sr::pdb_validate(2, allowed, group, 3) && !sr::pdb_validate(0, nullptr, nullptr, 3) &&
            !sr::pdb_validate(2, allowed, nullptr, 0) && sr::pdb_validate(-1, allowed, group, 3) &&
            sr::pdb_validate(2, nullptr, group, 3) && sr::pdb_validate(2, allowed, nullptr, 3) &&
            sr::pdb_validate(2, neg, group, 3) && sr::pdb_validate(2, allowed, high, 3) &&
            sr::pdb_validate(2, allowed, low, 3);
  if (!ok) return fail("the argument rules", seed, -1);
  if (lists >= 1000 && !(refusals && drains && stops && passed_fallbacks && by_last_need))
    return fail("a vacuous run", seed, -1);
  std::printf("seq_pdb_check ok: %d lists, %ld drains, %ld refusals (%ld of fallback candidates, %ld decided by the "
              "last of several needs), %ld fallback stops, %ld rounds\n", lists, drains, refusals, passed_fallbacks,
              by_last_need, stops, n_rounds);
  return 0;
}
