// seq_pdb.cpp — see seq_pdb.hpp.
#include "seq_pdb.hpp"

#include <algorithm>

namespace sr {

const char* pdb_validate(int32_t n_groups, const int32_t* allowed, const int32_t* pod_group, int64_t n_pods) {
  if (n_groups < 0) return "sr_pdb_limits: n_groups < 0";
  if (n_groups == 0) return nullptr;
  if (!allowed) return "sr_pdb_limits: allowed is NULL with n_groups > 0";
  if (!pod_group && n_pods > 0) return "sr_pdb_limits: pod_group is NULL with n_groups > 0";
  for (int32_t g = 0; g < n_groups; ++g)
    if (allowed[g] < 0) return "sr_pdb_limits: a negative allowance";
  for (int64_t q = 0; q < n_pods; ++q)
    if (pod_group[q] < -1 || pod_group[q] >= n_groups) return "sr_pdb_limits: a group id outside [-1, n_groups)";
  return nullptr;
}

void pdb_build(int32_t n_cand, const int32_t* cand_pod_off, int32_t n_groups, const int32_t* allowed,
               const int32_t* pod_group, PdbLedger* out) {
  out->n_groups = n_groups;
  out->remaining.assign(allowed, allowed + n_groups);
  out->need_off.assign(static_cast<size_t>(n_cand) + 1, 0);
  out->need_group.clear();
  out->need_count.clear();
  std::vector<int32_t> gs;
  const int32_t base = n_cand > 0 ? cand_pod_off[0] : 0;
  for (int32_t c = 0; c < n_cand; ++c) {
    gs.clear();
    for (int32_t q = cand_pod_off[c] - base; q < cand_pod_off[c + 1] - base; ++q)
      if (pod_group[q] >= 0) gs.push_back(pod_group[q]);
    std::sort(gs.begin(), gs.end());
    for (size_t i = 0; i < gs.size();) {
      size_t j = i;
      while (j < gs.size() && gs[j] == gs[i]) ++j;
      out->need_group.push_back(gs[i]);
      out->need_count.push_back(static_cast<int32_t>(j - i));
      i = j;
    }
    out->need_off[c + 1] = static_cast<int32_t>(out->need_group.size());
  }
}

PdbRound pdb_round(const PdbLedger& l, const uint8_t* kind, int32_t n_cand, int32_t floor) {
  PdbRound r;
  const int32_t stop = pdb_first_stop(l, floor, n_cand, [&](int32_t i) { return kind[i] == kPdbFallback; });
  const int32_t lim = stop == INT32_MAX ? n_cand : stop;
  for (int32_t i = floor + 1; i < lim; ++i) {
    if (kind[i] == kPdbEmpty || kind[i] == kPdbFallback || l.refused(i)) continue;
    r.live = true;
    if (kind[i] == kPdbDrains && r.winner < 0) r.winner = i;
  }
  if (r.winner >= 0) {
    r.end = r.winner;
  } else {
    r.end = lim - 1;
    if (stop != INT32_MAX) r.stop = stop;
  }
  return r;
}

}  // namespace sr
