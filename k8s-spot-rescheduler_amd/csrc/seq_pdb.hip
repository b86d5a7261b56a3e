// seq_pdb.hip — the ledger step of an sr_plan_sequence_pdb round (gfx950).
//
// K2 plans every active candidate above the floor and leaves the first
// drainable one in d_min[0]; with disruption budgets that candidate may be a
// refused one, and K2 wrote only ITS mapping to the host.  So the round's
// winner is found here, after K2 in stream order, from out_status and the
// device-resident allowances, and its mapping is published from out_node.
// Between two commits neither the snapshot nor `remaining` changes, so the
// refused flags computed at the start of the step hold for the whole round
// (DESIGN.md 1.1.1).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "kernels.hpp"

namespace sr {

namespace {

constexpr int kPdbThreads = 1024;

// One block.  Phase 1 (all reads of `remaining`): refused flags of the active
// candidates in (floor, fb_stop) and the smallest active index among the
// drainable, unrefused ones -- the active candidates ascend in the caller's
// index, so it is the first such candidate.  Phase 2, after the barrier: the
// winner's words to the host, its needs off `remaining`, and `win` for the
// ledger kernel.
__global__ __launch_bounds__(kPdbThreads) void k3_pdb_winner(SeqPdbRound p) {
  __shared__ int s_win;
  const SeqRound& r = p.r;
  const int tid = static_cast<int>(threadIdx.x);
  if (tid == 0) s_win = INT_MAX;
  __syncthreads();
  int best = INT_MAX;
  for (int ci = tid; ci < r.n_cand; ci += kPdbThreads) {
    const int g = r.cand_global[ci];
    bool ref = false;
    if (g > r.floor && g < r.fb_stop) {
      for (int k = p.need_off[g]; k < p.need_off[g + 1]; ++k) ref |= p.need_count[k] > p.remaining[p.need_group[k]];
      if (!ref && r.out_status[ci] < 0) best = min(best, ci);  // (ci ascends per thread: the first one stays)
    }
    p.refused[ci] = ref ? 1 : 0;
  }
  for (int d = 32; d > 0; d >>= 1) best = min(best, __shfl_xor(best, d, 64));
  if ((tid & 63) == 0 && best != INT_MAX) atomicMin(&s_win, best);
  __syncthreads();
  const int wi = s_win;
  const bool any = wi != INT_MAX;
  const int g = any ? r.cand_global[wi] : -1;
  const int off = any ? r.cand_off[wi] : 0;
  const int np = any ? r.cand_off[wi + 1] - off : 0;
  // every word carries the round's tag and is accepted on its own (write_winner)
  const uint64_t tag = static_cast<uint64_t>(p.seq) << 32;
  auto put = [&](int i, int v) {
    __hip_atomic_store(p.words + i, tag | static_cast<uint32_t>(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  };
  for (int q = tid; q < np; q += kPdbThreads) put(kPdbHeader + q, r.out_node[off + q]);
  if (tid == 0) put(0, g);
  if (tid == 1) put(1, np);
  if (tid == 2) {
    p.win[0] = any ? g : INT_MAX;
    p.win[1] = any ? wi : -1;
  }
  if (any)  // the commit: a group appears once in a candidate's needs, so no two threads meet
    for (int k = p.need_off[g] + tid; k < p.need_off[g + 1]; k += kPdbThreads)
      p.remaining[p.need_group[k]] -= p.need_count[k];
}

// The ledger (k3_sequence's copy with the round's own winner): the active
// candidates in (floor, min(winner, fb_stop - 1)] keep their K2 outcome in the
// sequence's arrays; a refused one is recorded as not planned.
__global__ __launch_bounds__(256) void k3_pdb_ledger(SeqPdbRound p) {
  const SeqRound& r = p.r;
  const int win = p.win[0];
  const int end = win < r.fb_stop ? win : r.fb_stop - 1;
  for (int ci = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x); ci < r.n_cand;
       ci += static_cast<int>(gridDim.x * blockDim.x)) {
    const int g = r.cand_global[ci];
    if (g <= r.floor || g > end) continue;
    const bool ref = p.refused[ci] != 0;
    r.seq_status[g] = ref ? -5 /* SR_CAND_PDB */ : r.out_status[ci];
    const int o = r.cand_off[ci], np = r.cand_off[ci + 1] - o;
    const int dst = r.in_off[g] - r.in_off[0];
    for (int k = 0; k < np; ++k) r.seq_node[dst + k] = ref ? -1 : r.out_node[o + k];
  }
}

}  // namespace

hipError_t launch_sequence_pdb(const SeqPdbRound& p, hipStream_t s) {
  hipLaunchKernelGGL(k3_pdb_winner, dim3(1), dim3(kPdbThreads), 0, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || p.r.n_cand <= 0) return e;
  const unsigned blocks = static_cast<unsigned>(std::min(64, (p.r.n_cand + 255) / 256));
  hipLaunchKernelGGL(k3_pdb_ledger, dim3(blocks), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace sr
