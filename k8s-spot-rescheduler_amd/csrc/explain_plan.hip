// explain_plan.hip — per-node refusal reasons of a candidate's stop pod in the context of its earlier
// pods (sr_explain_plan, gfx950).
//
// The grid of explain.hip: blockIdx.y is the query, a block of four waves
// takes four 64-bit row words, a lane one node, and the program walk is the
// same code (explain_walk.hpp).  A query carries the plain context of its
// earlier pods (explain_plan.hpp): a list sorted by node of {node, pods, acc[3]}.
// The entries of a wave's own word lie contiguously in it; the wave finds the
// first with a wave-uniform binary search and walks them with wave-uniform
// loads, and the lane owning an entry's node keeps it.  On such a touched node
// PODS is slack - pods < 1 (replacing the bit the atom-0 row gave) and CPU /
// MEMORY / EPHEMERAL compare the request with free - acc; every other bit
// stays as the walk left it.  A query with an empty list costs what k_explain
// costs and two more scalar loads.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "explain_dev.hpp"
#include "explain_walk.hpp"

namespace sr {

namespace {

__global__ __launch_bounds__(kXThreads) void k_explain_plan(ExplainPlanArgs pa) {
  __shared__ int s_part[kXWaves][kXCols];
  const ExplainArgs& a = pa.x;
  const int q = a.pod0 + static_cast<int>(blockIdx.y);
  const int lane = static_cast<int>(threadIdx.x) & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int word = static_cast<int>(blockIdx.x) * kXWaves + wave;
  const bool live = word < a.Wp;  // (wave-uniform; every wave reaches the barrier of explain_reduce)
  const int node = word * 64 + lane;
  const bool valid = live && node < a.n_spot;
  uint32_t mask = 0;
  if (live) {
    const ExplainPod p = a.pods[q];
    bool pods_judged;
    mask = explain_walk(a, p.cls, word, lane, &pods_judged);
    // the context entries of this word: [first entry with node >= 64 word, first with node >= 64 (word + 1))
    int64_t acc[3];
    const int touched = explain_touched(pa, q, word, node, acc);  // earlier pods on the lane's node
    if (touched > 0 && pods_judged)
      mask = (mask & ~(1u << WHY_PODS)) | (pa.node_slack[node] - touched < 1 ? 1u << WHY_PODS : 0u);
    if (p.resources) {  // node < n_pad = 64 Wp: the pads hold INT64_MIN, are never touched and are cleared below
      for (int d = 0; d < 3; ++d)
        if (p.req[d] > a.node_free[static_cast<size_t>(d) * a.n_pad + node] - acc[d]) mask |= 1u << (WHY_CPU + d);
    }
    if (!valid) mask = 0;
    if (a.node_mask && valid) a.node_mask[static_cast<size_t>(q) * a.n_spot + node] = static_cast<uint16_t>(mask);
  }
  explain_reduce(s_part, mask, valid, word, lane, wave, a.n_pad, a.sums + static_cast<size_t>(q) * kExplainSums);
}

// sr_shortfall_plan: k_explain_plan keeping, per lane, the differences behind the four resource bits (as
// k_shortfall does for k_explain).  The nodes' pod slack is node_left clamped, so pa.node_slack is not read.  A
// pad is never touched and holds INT64_MIN in node_free: it is left out before anything is subtracted.
__global__ __launch_bounds__(kXThreads) void k_shortfall_plan(ExplainPlanArgs pa, ShortfallArgs sa) {
  __shared__ int s_part[kXWaves][kXCols];
  __shared__ ShortLds s_short;
  const ExplainArgs& a = pa.x;
  const int q = a.pod0 + static_cast<int>(blockIdx.y);
  const int lane = static_cast<int>(threadIdx.x) & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int word = static_cast<int>(blockIdx.x) * kXWaves + wave;
  const bool live = word < a.Wp;
  const int node = word * 64 + lane;
  const bool valid = live && node < a.n_spot;
  uint32_t mask = 0;
  int64_t sf[SR_SHORT_COUNT] = {0, 0, 0, 0};
  if (live) {
    const ExplainPod p = a.pods[q];
    bool pods_judged;
    mask = explain_walk(a, p.cls, word, lane, &pods_judged);
    int64_t acc[3];
    const int touched = explain_touched(pa, q, word, node, acc);
    if (valid) {
      const int64_t left = sa.node_left[node];
      if (touched > 0 && pods_judged)
        mask = (mask & ~(1u << WHY_PODS)) | (short_slack(left) - touched < 1 ? 1u << WHY_PODS : 0u);
      if (p.resources) {
        for (int d = 0; d < 3; ++d) {
          const int64_t free = a.node_free[static_cast<size_t>(d) * a.n_pad + node] - acc[d];
          if (p.req[d] > free) {
            mask |= 1u << (WHY_CPU + d);
            sf[SR_SHORT_CPU + d] = p.req[d] - free;
          }
        }
      }
      if (mask >> WHY_PODS & 1) sf[SR_SHORT_PODS] = short_pods(left, touched);
      if (a.node_mask) a.node_mask[static_cast<size_t>(q) * a.n_spot + node] = static_cast<uint16_t>(mask);
      if (sa.node_short) shortfall_store(sa, static_cast<size_t>(q), a.n_spot, node, sf);
    } else {
      mask = 0;
    }
  }
  shortfall_wave(&s_short, mask, valid, sf, word, lane, wave);
  explain_reduce(s_part, mask, valid, word, lane, wave, a.n_pad, a.sums + static_cast<size_t>(q) * kExplainSums);
  shortfall_block(&s_short, sa, q);
}

}  // namespace

hipError_t launch_shortfall_plan(const ExplainPlanArgs& a, const ShortfallArgs& sa, hipStream_t s) {
  const unsigned gx = static_cast<unsigned>(shortfall_blocks(a.x.Wp));
  if (static_cast<int32_t>(gx) != sa.blocks) return hipErrorInvalidValue;
  for (int32_t q0 = 0; q0 < a.x.n_pods; q0 += 65535) {  // (gridDim.y)
    ExplainPlanArgs part = a;
    part.x.pod0 = q0;
    hipLaunchKernelGGL(k_shortfall_plan, dim3(gx, static_cast<unsigned>(std::min(65535, a.x.n_pods - q0))),
                       dim3(kXThreads), 0, s, part, sa);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_explain_plan(const ExplainPlanArgs& a, hipStream_t s) {
  const unsigned gx = static_cast<unsigned>((a.x.Wp + kXWaves - 1) / kXWaves);
  for (int32_t q0 = 0; q0 < a.x.n_pods; q0 += 65535) {  // (gridDim.y)
    ExplainPlanArgs part = a;
    part.x.pod0 = q0;
    hipLaunchKernelGGL(k_explain_plan, dim3(gx, static_cast<unsigned>(std::min(65535, a.x.n_pods - q0))),
                       dim3(kXThreads), 0, s, part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace sr
