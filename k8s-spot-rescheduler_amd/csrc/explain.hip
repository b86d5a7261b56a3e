// explain.hip — per-node refusal reasons of a pod (sr_explain_pods, gfx950).
//
// blockIdx.y is the queried pod; a block of four waves takes four 64-bit row
// words, a lane one node.  The wave walks the pod's explain program with
// wave-uniform loads of atoms[a][word]; each lane tests its own bit and keeps
// its node's 16-bit mask in a register (the reason of an operation is data, so
// a mask per lane needs no register indexed by it).  An open ORed term
// accumulates apart and is closed into NODE_AFFINITY.  The resource reasons
// are the lane's compares of the pod's requests with its node's free values.
// Padding nodes (>= n_spot) are cleared before anything is counted.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "explain_dev.hpp"

namespace sr {

namespace {

constexpr int kXThreads = 256, kXWaves = kXThreads / 64;
constexpr int kXCols = SR_WHY_COUNT + 2;  // per wave: a count per reason, feasible nodes, first feasible

__global__ __launch_bounds__(kXThreads) void k_explain(ExplainArgs a) {
  __shared__ int s_part[kXWaves][kXCols];
  const int q = a.pod0 + static_cast<int>(blockIdx.y);
  const int lane = static_cast<int>(threadIdx.x) & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int word = static_cast<int>(blockIdx.x) * kXWaves + wave;
  const bool live = word < a.Wp;  // (wave-uniform; every wave reaches the barrier below)
  const int node = word * 64 + lane;
  const bool valid = live && node < a.n_spot;
  uint32_t mask = 0;
  if (live) {
    const ExplainPod p = a.pods[q];
    const uint64_t me = 1ull << lane;
    bool in_terms = false, any = false, term = false;
    const int end = a.xoff[p.cls + 1];
    for (int i = a.xoff[p.cls]; i < end; ++i) {
      const int op = a.xops[i];
      const int kind = op & 7;
      const uint32_t why = 1u << (op >> 3 & 31);
      const bool bit = kind != X_ALL && (a.atoms[static_cast<size_t>(op >> 8) * a.Wp + word] & me) != 0;
      if (kind == X_AND) {
        mask |= bit ? 0u : why;
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
    if (p.resources) {  // node < n_pad = 64 Wp: the pads hold INT64_MIN and are cleared below
      for (int d = 0; d < 3; ++d)
        if (p.req[d] > a.node_free[static_cast<size_t>(d) * a.n_pad + node]) mask |= 1u << (WHY_CPU + d);
    }
    if (!valid) mask = 0;
    if (a.node_mask && valid) a.node_mask[static_cast<size_t>(q) * a.n_spot + node] = static_cast<uint16_t>(mask);
  }
  // lane r < 12 holds the nodes refusing for reason r, lane 12 the feasible
  // nodes, lane 13 the first feasible one as n_pad - position
  int mine = 0;
  for (int r = 0; r < SR_WHY_COUNT; ++r) {
    const uint64_t b = __ballot((mask >> r & 1) != 0);
    if (lane == r) mine = __popcll(b);
  }
  const uint64_t ok = __ballot(valid && mask == 0);
  if (lane == kExplainFeasible) mine = __popcll(ok);
  if (lane == kExplainFirst) mine = ok ? a.n_pad - (word * 64 + __ffsll(static_cast<unsigned long long>(ok)) - 1) : 0;
  if (lane < kXCols) s_part[wave][lane] = mine;
  __syncthreads();
  const int tid = static_cast<int>(threadIdx.x);
  if (tid < kXCols) {
    int v = 0;
    for (int w = 0; w < kXWaves; ++w) v = tid == kExplainFirst ? max(v, s_part[w][tid]) : v + s_part[w][tid];
    int* dst = a.sums + static_cast<size_t>(q) * kExplainSums + tid;
    if (v != 0) {
      if (tid == kExplainFirst) atomicMax(dst, v);
      else atomicAdd(dst, v);
    }
  }
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
