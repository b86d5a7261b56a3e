// seq_pdb.hpp — the disruption budgets of sr_plan_sequence_pdb, host side.
//
// HIP-free: plain arrays in and out, so the serial rule can be checked on a
// CPU (tools/seq_pdb_check.cpp).  A candidate's needs are the pods it has in
// each disruption group; a candidate is refused while some need exceeds what
// the group still allows; a drain spends its needs.  Allowances only fall
// during a pass, so a refused candidate stays refused.
#pragma once

#include <climits>
#include <cstdint>
#include <vector>

namespace sr {

struct PdbLedger {
  int32_t n_groups = 0;
  // the candidates' needs: a CSR of (group, count) by the caller's candidate
  // index, groups ascending within a candidate (the device holds a copy)
  std::vector<int32_t> need_off, need_group, need_count;
  std::vector<int32_t> remaining;  // [n_groups] the host's mirror of the device's allowances

  bool refused(int32_t c) const {
    for (int32_t k = need_off[c]; k < need_off[c + 1]; ++k)
      if (need_count[k] > remaining[need_group[k]]) return true;
    return false;
  }
  void commit(int32_t c) {
    for (int32_t k = need_off[c]; k < need_off[c + 1]; ++k) remaining[need_group[k]] -= need_count[k];
  }
};

// The argument rules of sr_pdb_limits with n_groups > 0: nullptr when they
// hold, else what is wrong.  n_pods: pods of the candidate list.
const char* pdb_validate(int32_t n_groups, const int32_t* allowed, const int32_t* pod_group, int64_t n_pods);

// Needs and allowances of a validated call.  pod_group is parallel to the
// candidates' pods, so pod q of the list (cand_pod_off[c] - cand_pod_off[0] <=
// q < cand_pod_off[c + 1] - cand_pod_off[0]) belongs to candidate c.
void pdb_build(int32_t n_cand, const int32_t* cand_pod_off, int32_t n_groups, const int32_t* allowed,
               const int32_t* pod_group, PdbLedger* out);

// The candidate a round stops at: the first unrefused fallback candidate above
// the floor (INT32_MAX: none).  A refused one is passed over.
template <class IsFallback>
int32_t pdb_first_stop(const PdbLedger& l, int32_t floor, int32_t n_cand, IsFallback is_fallback) {
  for (int32_t i = floor + 1; i < n_cand; ++i)
    if (is_fallback(i) && !l.refused(i)) return i;
  return INT32_MAX;
}

// One round as the device decides it, on candidates whose outcome does not
// depend on the snapshot (the check program's model): between two commits the
// allowances stand, so the refused set is fixed and the winner is the first
// drainable, unrefused candidate above the floor and below the stop.
enum PdbKind : uint8_t { kPdbEmpty = 0, kPdbFallback = 1, kPdbDrains = 2, kPdbFails = 3 };
struct PdbRound {
  int32_t winner = -1;  // the round's drain
  int32_t stop = -1;    // the unrefused fallback candidate the pass stops at (no winner below it)
  int32_t end = -1;     // the last candidate the round judged
  bool live = false;    // some candidate of the round needs the device (has pods, not refused, below the stop)
};
PdbRound pdb_round(const PdbLedger& l, const uint8_t* kind, int32_t n_cand, int32_t floor);

}  // namespace sr
