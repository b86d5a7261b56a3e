// node_view.hip — what each spot node refuses, reduced over the queries (sr_node_view_pods,
// sr_node_view_plan, gfx950).
//
// The mapping of explain.hip / explain_plan.hip: a block of four waves takes four 64-bit row words, a lane one
// node, the program walk is explain_walk.hpp's and the context entry of a touched node explain_touched's.
// blockIdx.y is a chunk of consecutive active queries (node_view.hpp: node_view_chunks) and not one query:
// the wave loops over its chunk and every lane folds each query's mask and shortfalls into its node's row
// (node_view_fold), which it keeps in registers -- 26 counts and four (shortfall, slot + 1) pairs.  A lane
// shares its row with no other lane, so a block writes its rows as one partial per chunk with plain coalesced
// stores ([cols][n_pad]): no LDS, no barrier, no atomic.  k_node_view_close, one thread per node and column,
// merges the chunks' partials into the call's totals (node_view_merge): sums commute and the minimum is the
// lexicographic (shortfall, slot) pair, so no result depends on the order of blocks, chunks or launches.  A pad
// (node >= n_spot) holds INT64_MIN in node_free: it is left out before anything is subtracted and writes nothing.
#include <hip/hip_runtime.h>

#include "explain_dev.hpp"
#include "explain_walk.hpp"
#include "node_view.hpp"

namespace sr {

namespace {

__global__ __launch_bounds__(kXThreads) void k_node_view(ExplainPlanArgs pa, NodeViewArgs na) {
  const ExplainArgs& a = pa.x;
  const int lane = static_cast<int>(threadIdx.x) & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int word = static_cast<int>(blockIdx.x) * kXWaves + wave;
  if (word >= a.Wp) return;  // (wave-uniform; the kernel holds no barrier)
  const int node = word * 64 + lane;
  const bool valid = node < a.n_spot;
  const int chunk = static_cast<int>(blockIdx.y);
  const int q0 = chunk * na.per, q1 = min(q0 + na.per, a.n_pods);

  int32_t cnt[kNodeViewCnt];
  uint64_t best[SR_SHORT_COUNT];
  int32_t at[SR_SHORT_COUNT];
#pragma unroll
  for (int k = 0; k < kNodeViewCnt; ++k) cnt[k] = 0;
#pragma unroll
  for (int d = 0; d < SR_SHORT_COUNT; ++d) {
    best[d] = 0;
    at[d] = 0;
  }
  int64_t left = 0, free[3] = {0, 0, 0};
  if (valid) {
    left = na.node_left[node];
    for (int d = 0; d < 3; ++d) free[d] = a.node_free[static_cast<size_t>(d) * a.n_pad + node];
  }

  for (int q = q0; q < q1; ++q) {
    const ExplainPod p = a.pods[q];
    const int slot1 = na.slot[q] + 1;
    bool pods_judged;
    uint32_t mask = explain_walk(a, p.cls, word, lane, &pods_judged);
    int touched = 0;
    int64_t acc[3] = {0, 0, 0};
    if (na.lists) touched = explain_touched(pa, q, word, node, acc);
    if (!valid) continue;
    // the lane's part of k_shortfall / k_shortfall_plan (without lists nothing is touched)
    int64_t sf[SR_SHORT_COUNT] = {0, 0, 0, 0};
    if (touched > 0 && pods_judged)
      mask = (mask & ~(1u << WHY_PODS)) | (short_slack(left) - touched < 1 ? 1u << WHY_PODS : 0u);
    if (p.resources) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const int64_t f = free[d] - acc[d];
        if (p.req[d] > f) {
          mask |= 1u << (WHY_CPU + d);
          sf[SR_SHORT_CPU + d] = p.req[d] - f;
        }
      }
    }
    if (mask >> WHY_PODS & 1) sf[SR_SHORT_PODS] = short_pods(left, touched);
    // node_view_fold
    cnt[kNodeViewAdmits] += mask == 0;
    cnt[kNodeViewNear] += mask != 0 && (mask & ~kShortBits) == 0;
#pragma unroll
    for (int r = 0; r < SR_WHY_COUNT; ++r) {
      cnt[kNodeViewRefuses + r] += static_cast<int32_t>(mask >> r & 1);
      cnt[kNodeViewSole + r] += mask == 1u << r;
    }
#pragma unroll
    for (int d = 0; d < SR_SHORT_COUNT; ++d) {
      const uint64_t v = static_cast<uint64_t>(sf[d]);
      if (mask == short_bit(d) && (at[d] == 0 || v < best[d] || (v == best[d] && slot1 < at[d]))) {
        best[d] = v;
        at[d] = slot1;
      }
    }
  }

  if (!valid) return;
  const size_t stride = static_cast<size_t>(a.n_pad), c = static_cast<size_t>(chunk);
#pragma unroll
  for (int k = 0; k < kNodeViewCnt; ++k) na.part_cnt[(c * kNodeViewCnt + k) * stride + node] = cnt[k];
#pragma unroll
  for (int d = 0; d < SR_SHORT_COUNT; ++d) {
    na.part_min[(c * SR_SHORT_COUNT + d) * stride + node] = best[d];
    na.part_at[(c * SR_SHORT_COUNT + d) * stride + node] = at[d];
  }
}

// One thread per node and column (blockIdx.y: the 26 counts, then the four pairs): the chunks' partials of one
// launch into the call's totals.  A thread per node alone left a launch of n_spot / 256 blocks walking 34 columns
// of every chunk one after the other.
constexpr int kNodeViewCloseCols = kNodeViewCnt + SR_SHORT_COUNT;

__global__ __launch_bounds__(kXThreads) void k_node_view_close(int n_spot, int n_pad, NodeViewArgs na) {
  const int node = static_cast<int>(blockIdx.x) * kXThreads + static_cast<int>(threadIdx.x);
  if (node >= n_spot) return;
  const size_t stride = static_cast<size_t>(n_pad), ts = static_cast<size_t>(na.tot_stride);
  const size_t chunks = static_cast<size_t>(na.chunks);
  const int col = static_cast<int>(blockIdx.y);  // (block-uniform)
  if (col < kNodeViewCnt) {
    int32_t v = na.tot_cnt[col * ts + node];
    for (size_t c = 0; c < chunks; ++c) v += na.part_cnt[(c * kNodeViewCnt + col) * stride + node];
    na.tot_cnt[col * ts + node] = v;
    return;
  }
  const int d = col - kNodeViewCnt;
  uint64_t best = na.tot_min[d * ts + node];
  int32_t at = na.tot_at[d * ts + node];
  for (size_t c = 0; c < chunks; ++c) {
    const uint64_t v = na.part_min[(c * SR_SHORT_COUNT + d) * stride + node];
    const int32_t s = na.part_at[(c * SR_SHORT_COUNT + d) * stride + node];
    if (s != 0 && (at == 0 || v < best || (v == best && s < at))) {
      best = v;
      at = s;
    }
  }
  na.tot_min[d * ts + node] = best;
  na.tot_at[d * ts + node] = at;
}

}  // namespace

hipError_t launch_node_view(const ExplainPlanArgs& a, const NodeViewArgs& na, hipStream_t s) {
  if (a.x.n_pods <= 0 || a.x.n_spot <= 0) return hipSuccess;
  const NodeViewChunks want = node_view_chunks(a.x.Wp, a.x.n_pods, na.per);
  if (na.per < 1 || want.chunks != na.chunks || na.chunks > kNodeViewMaxChunks || a.x.n_pad != a.x.Wp * 64 ||
      na.tot_stride < a.x.n_spot || (na.lists && !a.ctx_off))
    return hipErrorInvalidValue;
  ExplainPlanArgs all = a;
  all.x.pod0 = 0;
  hipLaunchKernelGGL(k_node_view, dim3(static_cast<unsigned>(shortfall_blocks(a.x.Wp)), static_cast<unsigned>(na.chunks)),
                     dim3(kXThreads), 0, s, all, na);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_node_view_close,
                     dim3(static_cast<unsigned>((a.x.n_spot + kXThreads - 1) / kXThreads), kNodeViewCloseCols),
                     dim3(kXThreads), 0, s, a.x.n_spot, a.x.n_pad, na);
  return hipGetLastError();
}

}  // namespace sr
