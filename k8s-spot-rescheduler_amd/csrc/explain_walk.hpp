// explain_walk.hpp — the program walk of the explain kernels (explain.hip, explain_plan.hip): one
// statement of it, so the two cannot drift apart.  Device code only.
#pragma once

#include "explain_dev.hpp"

namespace sr {

// The mask the explain program of class `cls` gives the lane's node (bit `lane`
// of row word `word`): wave-uniform loads of atoms[a][word], each lane tests its
// own bit.  The reason of an operation is data, so a mask per lane needs no
// register indexed by it.  An open ORed term accumulates apart and is closed
// into NODE_AFFINITY.  *pods_judged (wave-uniform): the program holds an AND on
// atom 0, the pod-count row, so WHY_PODS is the row's answer and not a decided
// class's silence.
__device__ __forceinline__ uint32_t explain_walk(const ExplainArgs& a, int cls, int word, int lane, bool* pods_judged) {
  uint32_t mask = 0;
  const uint64_t me = 1ull << lane;
  bool in_terms = false, any = false, term = false, pods = false;
  const int end = a.xoff[cls + 1];
  for (int i = a.xoff[cls]; i < end; ++i) {
    const int op = a.xops[i];
    const int kind = op & 7;
    const uint32_t why = 1u << (op >> 3 & 31);
    const bool bit = kind != X_ALL && (a.atoms[static_cast<size_t>(op >> 8) * a.Wp + word] & me) != 0;
    if (kind == X_AND) {
      mask |= bit ? 0u : why;
      pods = pods || (op >> 3) == WHY_PODS;  // atom 0, reason PODS
    } else if (kind == X_ANDNOT) {
      mask |= bit ? why : 0u;
    } else if (kind == X_TERM_START) {
      any = any || (in_terms && term);
      in_terms = true;
      term = bit;
    } else if (kind == X_TERM_AND) {
      term = term && bit;
    } else {
      mask |= why;
    }
  }
  if (in_terms && !(any || term)) mask |= 1u << WHY_NODE_AFFINITY;
  *pods_judged = pods;
  return mask;
}

constexpr int kXThreads = 256, kXWaves = kXThreads / 64;
constexpr int kXCols = SR_WHY_COUNT + 2;  // per wave: a count per reason, feasible nodes, first feasible

// Counts, feasible nodes and the first feasible node of one block into
// sums[q]: ballots, LDS partials, one atomic per column and block.  Every wave
// of the block calls it (it holds the block's barrier).
__device__ __forceinline__ void explain_reduce(int (*s_part)[kXCols], uint32_t mask, bool valid, int word, int lane,
                                               int wave, int n_pad, int* sums_q) {
  // lane r < 12 holds the nodes refusing for reason r, lane 12 the feasible
  // nodes, lane 13 the first feasible one as n_pad - position
  int mine = 0;
  for (int r = 0; r < SR_WHY_COUNT; ++r) {
    const uint64_t b = __ballot((mask >> r & 1) != 0);
    if (lane == r) mine = __popcll(b);
  }
  const uint64_t ok = __ballot(valid && mask == 0);
  if (lane == kExplainFeasible) mine = __popcll(ok);
  if (lane == kExplainFirst) mine = ok ? n_pad - (word * 64 + __ffsll(static_cast<unsigned long long>(ok)) - 1) : 0;
  if (lane < kXCols) s_part[wave][lane] = mine;
  __syncthreads();
  const int tid = static_cast<int>(threadIdx.x);
  if (tid < kXCols) {
    int v = 0;
    for (int w = 0; w < kXWaves; ++w) v = tid == kExplainFirst ? max(v, s_part[w][tid]) : v + s_part[w][tid];
    int* dst = sums_q + tid;
    if (v != 0) {
      if (tid == kExplainFirst) atomicMax(dst, v);
      else atomicAdd(dst, v);
    }
  }
}

}  // namespace sr
