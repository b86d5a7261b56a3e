// explain.hip — per-node refusal reasons of a pod (sr_explain_pods, gfx950).
//
// blockIdx.y is the queried pod; a block of four waves takes four 64-bit row
// words, a lane one node.  The wave walks the pod's explain program
// (explain_walk.hpp, shared with explain_plan.hip) and keeps its node's 16-bit
// mask in a register.  The resource reasons
// are the lane's compares of the pod's requests with its node's free values.
// Padding nodes (>= n_spot) are cleared before anything is counted.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "explain_dev.hpp"
#include "explain_walk.hpp"

namespace sr {

namespace {

__global__ __launch_bounds__(kXThreads) void k_explain(ExplainArgs a) {
  __shared__ int s_part[kXWaves][kXCols];
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
    if (p.resources) {  // node < n_pad = 64 Wp: the pads hold INT64_MIN and are cleared below
      for (int d = 0; d < 3; ++d)
        if (p.req[d] > a.node_free[static_cast<size_t>(d) * a.n_pad + node]) mask |= 1u << (WHY_CPU + d);
    }
    if (!valid) mask = 0;
    if (a.node_mask && valid) a.node_mask[static_cast<size_t>(q) * a.n_spot + node] = static_cast<uint16_t>(mask);
  }
  explain_reduce(s_part, mask, valid, word, lane, wave, a.n_pad, a.sums + static_cast<size_t>(q) * kExplainSums);
}

// sr_shortfall_pods: k_explain keeping, per lane, the differences behind the four resource bits.  The masks,
// counts, feasible and first are k_explain's.  A pad holds INT64_MIN in node_free: it is left out before anything
// is subtracted (its mask is cleared as above, its shortfalls stay zero and it votes in no reduction).
__global__ __launch_bounds__(kXThreads) void k_shortfall(ExplainArgs a, ShortfallArgs sa) {
  __shared__ int s_part[kXWaves][kXCols];
  __shared__ ShortLds s_short;
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
    if (valid) {
      if (p.resources) {
        for (int d = 0; d < 3; ++d) {
          const int64_t free = a.node_free[static_cast<size_t>(d) * a.n_pad + node];
          if (p.req[d] > free) {
            mask |= 1u << (WHY_CPU + d);
            sf[SR_SHORT_CPU + d] = p.req[d] - free;
          }
        }
      }
      if (mask >> WHY_PODS & 1) sf[SR_SHORT_PODS] = short_pods(sa.node_left[node], 0);
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

// One thread per (query, dimension): the query's partials in block order, so the lowest position among equals.
__global__ __launch_bounds__(kXThreads) void k_shortfall_close(int n, ShortfallArgs sa) {
  const int t = static_cast<int>(blockIdx.x) * kXThreads + static_cast<int>(threadIdx.x);
  if (t >= n) return;
  const int q = t / SR_SHORT_COUNT, d = t % SR_SHORT_COUNT;
  uint64_t m = kShortNone;
  int at = -1;
  for (int b = 0; b < sa.blocks; ++b) {
    const size_t o = (static_cast<size_t>(q) * sa.blocks + b) * SR_SHORT_COUNT + d;
    const uint64_t v = sa.part_min[o];
    if (v < m) {
      m = v;
      at = sa.part_at[o];
    }
  }
  sa.only_min[t] = at < 0 ? 0 : static_cast<int64_t>(m);
  sa.only_at[t] = at;
}

}  // namespace

hipError_t launch_shortfall(const ExplainArgs& a, const ShortfallArgs& sa, hipStream_t s) {
  const unsigned gx = static_cast<unsigned>(shortfall_blocks(a.Wp));
  if (static_cast<int32_t>(gx) != sa.blocks) return hipErrorInvalidValue;
  for (int32_t q0 = 0; q0 < a.n_pods; q0 += 65535) {  // (gridDim.y)
    ExplainArgs part = a;
    part.pod0 = q0;
    hipLaunchKernelGGL(k_shortfall, dim3(gx, static_cast<unsigned>(std::min(65535, a.n_pods - q0))), dim3(kXThreads), 0,
                       s, part, sa);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_shortfall_close(int32_t n_pods, const ShortfallArgs& sa, hipStream_t s) {
  if (n_pods <= 0) return hipSuccess;
  const int n = n_pods * SR_SHORT_COUNT;
  hipLaunchKernelGGL(k_shortfall_close, dim3(static_cast<unsigned>((n + kXThreads - 1) / kXThreads)), dim3(kXThreads), 0,
                     s, n, sa);
  return hipGetLastError();
}

hipError_t launch_explain(const ExplainArgs& a, hipStream_t s) {
  const unsigned gx = static_cast<unsigned>((a.Wp + kXWaves - 1) / kXWaves);
  for (int32_t q0 = 0; q0 < a.n_pods; q0 += 65535) {  // (gridDim.y)
    ExplainArgs part = a;
    part.pod0 = q0;
    hipLaunchKernelGGL(k_explain, dim3(gx, static_cast<unsigned>(std::min(65535, a.n_pods - q0))), dim3(kXThreads), 0, s,
                       part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace sr
