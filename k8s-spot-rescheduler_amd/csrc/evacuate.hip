// evacuate.hip — what a spot reclaim strands, one scenario per block of waves (sr_evacuate_plan, gfx950).
//
// A scenario is one dependent chain of possibly thousands of pods -- where pod k lands depends on where pods
// 0..k-1 went -- so the parallelism inside it is across nodes, and here across the waves of a block as well:
// wave w takes the row words r W + w of round r, a lane one node of its word.  Per pod and word it is
// k_blockers' lane: explain_walk for the pod's class, then PODS as slack - added < 1 where the scenario itself
// put pods on the node, and the three resource compares against free - used.  A lost node (a bit of the
// scenario's mask in LDS) and a pad are never a target and vote in no row.  After each round every wave leaves
// its lowest fitting position in LDS and one barrier decides the pod: the smallest position wins, and only
// after the last round is the pod stranded.  The slots the waves leave their positions in alternate between
// two sets from barrier to barrier, so a wave still reading one round's set is never overtaken by the next
// round's writes.
// The context is dense and private to the block: used[3][n_pad] and added[n_pad] in the block's slice of a
// global scratch buffer that is zero before the launch.  The word -> wave map is fixed for a launch, so the
// deltas of a node are read and written by one and the same lane and need no barrier; after the scenario the
// block puts its slice back to zero by walking the scenario's own node_of_pod, and takes the next scenario
// grid-stride.  Every decision is block-uniform and every wave takes every barrier.  Per-reason ballots are kept
// only when counts are wanted (lane r of a wave carries reason r's sum over its words) and summed over the
// waves through LDS: no atomic touches global memory, and no result depends on the grid, the waves a block or
// the order of the scenarios.
#include <hip/hip_runtime.h>

#include "evacuate.hpp"
#include "evacuate_dev.hpp"
#include "explain_walk.hpp"

namespace sr {

namespace {

constexpr int kNoFit = 0x7fffffff;

__global__ __launch_bounds__(kEvacMaxWaves * 64) void k_evacuate(EvacuateArgs b) {
  extern __shared__ uint32_t s_lost[];  // [2 Wp] the scenario's lost set, word w's low half at 2 w
  __shared__ int s_fit[2][kEvacMaxWaves];
  __shared__ int s_cnt[kEvacMaxWaves][SR_WHY_COUNT];
  const ExplainArgs& a = b.x;
  const int tid = static_cast<int>(threadIdx.x), threads = static_cast<int>(blockDim.x);
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int W = b.waves;  // (blockDim.x / 64)
  const size_t n_pad = static_cast<size_t>(a.n_pad);
  int64_t* used = b.used + static_cast<size_t>(blockIdx.x) * 3 * n_pad;
  int32_t* added = b.added + static_cast<size_t>(blockIdx.x) * n_pad;
  const int rounds = (a.Wp + W - 1) / W;
  int flip = 0;  // the set of s_fit the next barrier decides on (block-uniform)
  for (int s = static_cast<int>(blockIdx.x); s < b.n_scen; s += static_cast<int>(gridDim.x)) {
    // the lost set: cleared, then a bit per lost position
    for (int i = tid; i < 2 * a.Wp; i += threads) s_lost[i] = 0;
    __syncthreads();
    for (int i = b.lost_off[s] + tid; i < b.lost_off[s + 1]; i += threads) {
      const int p = b.lost_pos[i];
      if (p >= 0 && p < a.n_spot) atomicOr(&s_lost[p >> 5], 1u << (p & 31));
    }
    __syncthreads();
    const int p0 = b.scen_off[s], p1 = b.scen_off[s + 1];
    int stranded = 0, first = -1;
    for (int k = p0; k < p1; ++k) {
      const BlockerPod bp = b.pods[k];
      int placed = -1, mine = 0;
      for (int r = 0; r < rounds; ++r) {
        const int word = r * W + wave;
        int fit = kNoFit;
        if (word < a.Wp) {  // (wave-uniform)
          const int node = word * 64 + lane;
          const bool lost = (s_lost[node >> 5] >> (node & 31) & 1u) != 0;
          const bool valid = node < a.n_spot && !lost;
          bool pods_judged;
          uint32_t mask = explain_walk(a, bp.p.cls, word, lane, &pods_judged);
          if (valid) {  // a pad holds INT64_MIN in node_free and is never touched: it is left out here
            const int touched = added[node];
            if (touched > 0 && pods_judged)
              mask = (mask & ~(1u << WHY_PODS)) | (short_slack(b.node_left[node]) - touched < 1 ? 1u << WHY_PODS : 0u);
            if (bp.p.resources) {
              for (int d = 0; d < 3; ++d)
                if (bp.p.req[d] > a.node_free[static_cast<size_t>(d) * n_pad + node] - used[static_cast<size_t>(d) * n_pad + node])
                  mask |= 1u << (WHY_CPU + d);
            }
          } else {
            mask = 0;
          }
          const uint64_t ok = __ballot(valid && mask == 0);
          if (ok != 0) fit = word * 64 + __ffsll(static_cast<unsigned long long>(ok)) - 1;
          if (b.counts) {
            for (int q = 0; q < SR_WHY_COUNT; ++q) {
              const uint64_t v = __ballot((mask >> q & 1) != 0);
              if (lane == q) mine += __popcll(v);
            }
          }
        }
        if (lane == 0) s_fit[flip][wave] = fit;
        __syncthreads();
        int best = kNoFit;
        for (int w = 0; w < W; ++w) best = min(best, s_fit[flip][w]);
        flip ^= 1;
        if (best != kNoFit) {  // (block-uniform)
          placed = best;
          break;
        }
      }
      if (tid == 0) b.node_of_pod[k] = placed;
      if (placed < 0) {
        ++stranded;
        if (first < 0) first = k - p0;
        if (b.counts) {  // (block-uniform: a kernel argument)
          if (lane < SR_WHY_COUNT) s_cnt[wave][lane] = mine;
          __syncthreads();
          if (tid < SR_WHY_COUNT) {
            int v = 0;
            for (int w = 0; w < W; ++w) v += s_cnt[w][tid];
            b.counts[static_cast<size_t>(k) * SR_WHY_COUNT + tid] = v;
          }
        }
        continue;
      }
      // AddPod: the lane that judges `placed` owns its deltas
      if ((placed >> 6) % W == wave && (placed & 63) == lane) {
        added[placed] += 1;
        for (int d = 0; d < 3; ++d) used[static_cast<size_t>(d) * n_pad + placed] += bp.acc[d];
      }
    }
    if (tid == 0) {
      b.stranded[s] = stranded;
      b.first[s] = first;
    }
    // the undo log: the scenario's own mapping (thread 0 wrote it: the barrier makes it the block's)
    __syncthreads();
    for (int k = p0 + tid; k < p1; k += threads) {
      const int at = b.node_of_pod[k];
      if (at >= 0 && at < a.n_spot) {
        added[at] = 0;
        for (int d = 0; d < 3; ++d) used[static_cast<size_t>(d) * n_pad + at] = 0;
      }
    }
    __syncthreads();
  }
}

}  // namespace

hipError_t launch_evacuate(const EvacuateArgs& b, int32_t blocks, hipStream_t s) {
  if (b.n_scen <= 0) return hipSuccess;
  if (blocks < 1 || b.waves < 1 || b.waves > kEvacMaxWaves || b.x.Wp > kEvacMaxWp) return hipErrorInvalidValue;
  const size_t lds = static_cast<size_t>(b.x.Wp) * 8;
  hipLaunchKernelGGL(k_evacuate, dim3(static_cast<unsigned>(blocks)), dim3(static_cast<unsigned>(b.waves) * 64), lds, s, b);
  return hipGetLastError();
}

}  // namespace sr
