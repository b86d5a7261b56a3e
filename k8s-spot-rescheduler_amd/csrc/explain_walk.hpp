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

// The context entry of the lane's node in query q's list: the entries of the wave's own word lie contiguously,
// the wave finds the first with a wave-uniform binary search and walks them with wave-uniform loads, and the
// lane owning an entry's node keeps it.  Returns the earlier pods on the node (0: untouched, acc zeros).
__device__ __forceinline__ int explain_touched(const ExplainPlanArgs& pa, int q, int word, int node, int64_t acc[3]) {
  const int c0 = pa.ctx_off[q], c1 = pa.ctx_off[q + 1];
  int touched = 0;
  acc[0] = acc[1] = acc[2] = 0;
  if (c0 < c1) {
    int lo = c0, hi = c1;
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (pa.ctx[mid].node < word * 64) lo = mid + 1;
      else hi = mid;
    }
    for (int i = lo; i < c1; ++i) {
      const int en = pa.ctx[i].node;
      if (en >= word * 64 + 64) break;
      if (en == node) {
        touched = pa.ctx[i].pods;
        for (int d = 0; d < 3; ++d) acc[d] = pa.ctx[i].acc[d];
      }
    }
  }
  return touched;
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

// --- the shortfall kernels (k_shortfall, k_shortfall_plan) ---

static_assert(kXWaves == 4, "shortfall_blocks (explain_args.hpp) counts four row words a block");

// The mask bit of a dimension: SR_SHORT_CPU / MEMORY / EPHEMERAL follow WHY_CPU.., SR_SHORT_PODS is WHY_PODS.
__device__ __forceinline__ uint32_t short_bit(int d) { return d < 3 ? 1u << (WHY_CPU + d) : 1u << WHY_PODS; }
constexpr uint32_t kShortBits = 1u << WHY_PODS | 1u << WHY_CPU | 1u << WHY_MEMORY | 1u << WHY_EPHEMERAL;

// shortfall_node's pod term: 1 + earlier pods there - left, saturating at INT64_MAX (only read where the bit is set)
__device__ __forceinline__ int64_t short_pods(int64_t left, int touched) {
  const uint64_t u = uint64_t(1) + static_cast<uint64_t>(touched) - static_cast<uint64_t>(left);
  return static_cast<int64_t>(u < static_cast<uint64_t>(INT64_MAX) ? u : static_cast<uint64_t>(INT64_MAX));
}
// node_slack's clamp of node_left
__device__ __forceinline__ int short_slack(int64_t left) {
  return static_cast<int>(left < -(1 << 30) ? -(1 << 30) : left > (1 << 30) ? (1 << 30) : left);
}

struct ShortLds {
  int cnt[kXWaves][1 + SR_SHORT_COUNT];  // near, only_nodes
  uint64_t min[kXWaves][SR_SHORT_COUNT];
  int at[kXWaves][SR_SHORT_COUNT];
};

// The wave's part, before the block's barrier (the one explain_reduce holds): near-miss and only-d nodes by
// ballot; per dimension the smallest shortfall among the wave's only-d nodes by a 64-bit butterfly (skipped,
// wave-uniformly, when the wave has none) and the lowest lane attaining it by a second ballot.  A pad is not
// valid, so it never votes and its sf (zeros: nothing was subtracted for it) is never read.
__device__ __forceinline__ void shortfall_wave(ShortLds* s, uint32_t mask, bool valid, const int64_t sf[SR_SHORT_COUNT],
                                               int word, int lane, int wave) {
  const uint64_t nb = __ballot(valid && mask != 0 && (mask & ~kShortBits) == 0);
  if (lane == 0) s->cnt[wave][0] = __popcll(nb);
  for (int d = 0; d < SR_SHORT_COUNT; ++d) {
    const bool only = valid && mask == short_bit(d);
    const uint64_t ob = __ballot(only);
    uint64_t m = kShortNone;
    int at = -1;
    if (ob != 0) {
      const uint64_t key = only ? static_cast<uint64_t>(sf[d]) : kShortNone;
      m = key;
      for (int x = 32; x >= 1; x >>= 1) {
        const uint64_t o = __shfl_xor(static_cast<unsigned long long>(m), x, 64);
        m = o < m ? o : m;
      }
      const uint64_t hit = __ballot(only && key == m);
      at = word * 64 + __ffsll(static_cast<unsigned long long>(hit)) - 1;
    }
    if (lane == 0) {
      s->cnt[wave][1 + d] = __popcll(ob);
      s->min[wave][d] = m;
      s->at[wave][d] = at;
    }
  }
}

// The block's part, after the barrier: the counts as explain_reduce adds its own (one atomic per column and
// block), the block's minimum per dimension as a partial.  The waves lie in position order, so a strict
// compare keeps the lowest position among equals.  Every block writes its four partials, so they need no
// initial value.
__device__ __forceinline__ void shortfall_block(const ShortLds* s, const ShortfallArgs& sa, int q) {
  const int tid = static_cast<int>(threadIdx.x);
  if (tid < 1 + SR_SHORT_COUNT) {
    int v = 0;
    for (int w = 0; w < kXWaves; ++w) v += s->cnt[w][tid];
    if (v != 0) atomicAdd(sa.sums + static_cast<size_t>(q) * kShortSums + tid, v);
  } else if (tid >= 64 && tid < 64 + SR_SHORT_COUNT) {
    const int d = tid - 64;
    uint64_t m = kShortNone;
    int at = -1;
    for (int w = 0; w < kXWaves; ++w)
      if (s->min[w][d] < m) {
        m = s->min[w][d];
        at = s->at[w][d];
      }
    const size_t o = (static_cast<size_t>(q) * sa.blocks + blockIdx.x) * SR_SHORT_COUNT + d;
    sa.part_min[o] = m;
    sa.part_at[o] = at;
  }
}

// The lane's node's four shortfalls to node_short: 32 contiguous bytes.
__device__ __forceinline__ void shortfall_store(const ShortfallArgs& sa, size_t q, int n_spot, int node,
                                                const int64_t sf[SR_SHORT_COUNT]) {
  int64_t* dst = sa.node_short + (q * n_spot + node) * SR_SHORT_COUNT;
  for (int d = 0; d < SR_SHORT_COUNT; ++d) dst[d] = sf[d];
}

}  // namespace sr
