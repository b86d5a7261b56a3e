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

}  // namespace

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
