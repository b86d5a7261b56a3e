// blockers.hip — canDrainNode's loop without its early return, one candidate per wave (sr_blockers_plan,
// gfx950).
//
// The plan of a candidate is a dependent chain -- where pod k lands depends on where pods 0..k-1 went -- so the
// only parallelism inside it is across nodes: a wave takes one candidate, a lane one node, and the wave steps
// through the 64-bit row words in order.  Per pod and word it is k_explain_plan's lane: explain_walk for the
// pod's class, then on a node the candidate itself has touched PODS as slack - touched < 1 and the three
// resource compares against free - acc.  The first word whose ballot of mask == 0 is non-zero places the pod on
// its lowest set bit; a pod that reaches the last word without one is a blocker, and only then (and only when
// counts are wanted) were the per-reason ballots of every word worth keeping: lane r carries reason r's sum,
// so the row needs no reduction at the end.
// The context is the candidate's own: a list of distinct nodes sorted by node in the wave's LDS (kBlockersCtx
// entries, blockers.hpp; the host batches no longer candidate), lane i keeping the nodes of entries i, 64 + i, ...
// in registers.  The entries of a word are found with ballots over those registers and read with wave-uniform
// LDS loads; an insert shifts the tail up by one, every lane moving its own entries.  Waves share nothing: no
// barrier and no atomic, and a wave beyond the last candidate leaves at once.
#include <hip/hip_runtime.h>

#include "blockers.hpp"
#include "blockers_dev.hpp"
#include "explain_walk.hpp"

namespace sr {

namespace {

struct BlockersLds {
  int32_t node[kBlockersCtx];
  int32_t pods[kBlockersCtx];
  int64_t acc[3][kBlockersCtx];
};

constexpr int kNoNode = 0x7fffffff;

// LDS written by some lanes of the wave and read by others: the wave runs in lockstep, the compiler must not
// move the accesses across this point.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int kBlockersSlots = kBlockersCtx / 64;  // list entries a lane keeps the node of
static_assert(kBlockersCtx % 64 == 0, "a lane keeps the node of entries lane, 64 + lane, ...");

// Entries of the sorted list with node < x: the lanes' registers hold the list in order, kNoNode behind it.
__device__ __forceinline__ int below(const int (&my_node)[kBlockersSlots], int n, int x) {
  int v = 0;
#pragma unroll
  for (int j = 0; j < kBlockersSlots; ++j)
    if (j * 64 < n) v += __popcll(__ballot(my_node[j] < x));  // (wave-uniform: slots past the list hold nothing)
  return v;
}

__global__ __launch_bounds__(kBlockersThreads) void k_blockers(BlockersArgs b) {
  __shared__ BlockersLds s_ctx[kBlockersWaves];
  const ExplainArgs& a = b.x;
  const int lane = static_cast<int>(threadIdx.x) & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int c = static_cast<int>(blockIdx.x) * kBlockersWaves + wave;
  if (c >= b.n_cand) return;  // (wave-uniform; the kernel holds no barrier)
  BlockersLds& s = s_ctx[wave];
  const int p0 = b.cand_off[c], p1 = b.cand_off[c + 1];
  int n = 0;  // entries of the list (wave-uniform)
  // entry 64 j + lane's node in my_node[j], kNoNode from n on: the list's positions by ballots, without LDS
  int my_node[kBlockersSlots];
#pragma unroll
  for (int j = 0; j < kBlockersSlots; ++j) my_node[j] = kNoNode;
  int blockers = 0, first = -1;
  for (int k = p0; k < p1; ++k) {
    const BlockerPod bp = b.pods[k];
    int placed = -1, mine = 0;
    for (int word = 0; word < a.Wp; ++word) {
      const int node = word * 64 + lane;
      const bool valid = node < a.n_spot;
      bool pods_judged;
      uint32_t mask = explain_walk(a, bp.p.cls, word, lane, &pods_judged);
      // the list's entries of this word: [lo, hi), the list being sorted and my_node kNoNode behind it
      const int lo = below(my_node, n, word * 64), hi = below(my_node, n, word * 64 + 64);
      int touched = 0;
      int64_t acc[3] = {0, 0, 0};
      for (int i = lo; i < hi; ++i)
        if (s.node[i] == node) {
          touched = s.pods[i];
          for (int d = 0; d < 3; ++d) acc[d] = s.acc[d][i];
        }
      if (valid) {  // a pad holds INT64_MIN in node_free and is never touched: it is left out here
        if (touched > 0 && pods_judged)
          mask = (mask & ~(1u << WHY_PODS)) | (short_slack(b.node_left[node]) - touched < 1 ? 1u << WHY_PODS : 0u);
        if (bp.p.resources) {
          for (int d = 0; d < 3; ++d)
            if (bp.p.req[d] > a.node_free[static_cast<size_t>(d) * a.n_pad + node] - acc[d]) mask |= 1u << (WHY_CPU + d);
        }
      } else {
        mask = 0;
      }
      const uint64_t ok = __ballot(valid && mask == 0);
      if (ok != 0) {
        placed = word * 64 + __ffsll(static_cast<unsigned long long>(ok)) - 1;
        break;
      }
      if (b.counts) {
        for (int r = 0; r < SR_WHY_COUNT; ++r) {
          const uint64_t v = __ballot((mask >> r & 1) != 0);
          if (lane == r) mine += __popcll(v);
        }
      }
    }
    if (lane == 0) b.node_of_pod[k] = placed;
    if (placed < 0) {
      ++blockers;
      if (first < 0) first = k - p0;
      if (b.counts && lane < SR_WHY_COUNT) b.counts[static_cast<size_t>(k) * SR_WHY_COUNT + lane] = mine;
      continue;
    }
    // AddPod: (placed, 1, acc) into the sorted list
    const int pos = below(my_node, n, placed);
    const bool there = pos < n && s.node[pos] == placed;  // (wave-uniform)
    if (there) {
      if (lane == 0) {
        s.pods[pos] += 1;
        for (int d = 0; d < 3; ++d) s.acc[d][pos] += bp.acc[d];
      }
    } else if (n < kBlockersCtx) {  // (always: a batched candidate has at most kBlockersCtx pods)
      // the tail [pos, n) moves up by one, every lane its own entries: all reads, then all writes; n < kBlockersCtx,
      // so position n is inside
      int mp[kBlockersSlots];
      int64_t ma[kBlockersSlots][3];
#pragma unroll
      for (int j = 0; j < kBlockersSlots; ++j) {
        const int at = j * 64 + lane;
        mp[j] = 0;
        ma[j][0] = ma[j][1] = ma[j][2] = 0;
        if (at >= pos && at < n) {
          mp[j] = s.pods[at];
          for (int d = 0; d < 3; ++d) ma[j][d] = s.acc[d][at];
        }
      }
      wave_sync();
#pragma unroll
      for (int j = 0; j < kBlockersSlots; ++j) {
        const int at = j * 64 + lane;
        if (at >= pos && at < n) {
          s.node[at + 1] = my_node[j];
          s.pods[at + 1] = mp[j];
          for (int d = 0; d < 3; ++d) s.acc[d][at + 1] = ma[j][d];
        }
      }
      if (lane == 0) {
        s.node[pos] = placed;
        s.pods[pos] = 1;
        for (int d = 0; d < 3; ++d) s.acc[d][pos] = bp.acc[d];
      }
      ++n;
    }
    wave_sync();
#pragma unroll
    for (int j = 0; j < kBlockersSlots; ++j) my_node[j] = j * 64 + lane < n ? s.node[j * 64 + lane] : kNoNode;
  }
  if (lane == 0) {
    b.blockers[c] = blockers;
    b.first[c] = first;
  }
}

}  // namespace

hipError_t launch_blockers(const BlockersArgs& b, hipStream_t s) {
  if (b.n_cand <= 0) return hipSuccess;
  const unsigned gx = static_cast<unsigned>((b.n_cand + kBlockersWaves - 1) / kBlockersWaves);
  hipLaunchKernelGGL(k_blockers, dim3(gx), dim3(kBlockersThreads), 0, s, b);
  return hipGetLastError();
}

}  // namespace sr
