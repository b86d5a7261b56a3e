// planner.cpp — device context, resident buffers and the planning tick.  (The read-only query calls --
// sr_explain_*, sr_shortfall_*, sr_node_view_*, sr_blockers_plan, sr_evacuate_plan -- are query.cpp's; the
// context holds their state as one member and shares the device, the stream and the error string with them.)
//
// sr_ctx plays the role of the reference's predicate checker (created once,
// rescheduler.go:149).  One tick (sr_plan_run) is three kernels on a single
// HIP stream; K3 writes the result straight into mapped host memory:
//   K0 tables -> K2 placement -> [RCCL allreduce(min)] -> K3 winner
// There is no CPU path: without a HIP device sr_create fails.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "dev_buf.hpp"
#include "host.hpp"
#include "kernels.hpp"
#include "query.hpp"
#include "residency.hpp"
#include "result_words.hpp"
#include "seq_pdb.hpp"

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

namespace {

// RCCL is loaded on first use (sr_comm_unique_id / sr_comm_init): a
// single-GPU planner never maps it.  The calls keep their rccl.h signatures.
struct Rccl {
  decltype(&ncclGetUniqueId) get_unique_id = nullptr;
  decltype(&ncclCommInitRank) comm_init_rank = nullptr;
  decltype(&ncclAllReduce) all_reduce = nullptr;
  decltype(&ncclCommDestroy) comm_destroy = nullptr;
  decltype(&ncclGetErrorString) error_string = nullptr;
  bool ok = false;
};

const Rccl& rccl() {
  static const Rccl r = [] {
    Rccl x;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) return x;
    x.get_unique_id = reinterpret_cast<decltype(x.get_unique_id)>(dlsym(h, "ncclGetUniqueId"));
    x.comm_init_rank = reinterpret_cast<decltype(x.comm_init_rank)>(dlsym(h, "ncclCommInitRank"));
    x.all_reduce = reinterpret_cast<decltype(x.all_reduce)>(dlsym(h, "ncclAllReduce"));
    x.comm_destroy = reinterpret_cast<decltype(x.comm_destroy)>(dlsym(h, "ncclCommDestroy"));
    x.error_string = reinterpret_cast<decltype(x.error_string)>(dlsym(h, "ncclGetErrorString"));
    x.ok = x.get_unique_id && x.comm_init_rank && x.all_reduce && x.comm_destroy && x.error_string;
    return x;
  }();
  return r;
}

using sr::DevBuf;
using sr::HostBuf;
using sr::dev_reserve;
using sr::host_reserve;

// One workload slot: an encoded candidate input with its device arena and
// pinned staging copy.  sr_plan_first's prefix batches and an every-candidate
// plan are different inputs; with a slot each, a tick whose inputs equal the
// previous tick's reuses each one's candidate side (CandReuse) and its
// device-resident records instead of re-encoding and re-uploading them.
struct Slot {
  sr::Workload wl;
  sr::Residency res;  // what the buffers below hold (residency.hpp)
  DevBuf arena;
  HostBuf h_arena;
  DevBuf tables;      // S and T rows (K0 writes, K2 reads)
  HostBuf h_cycles;   // the K2 durations of the work list by cost (complete at ev_cost)
  hipEvent_t ev_cost = nullptr;
  uint64_t key = 0;   // fingerprint of the input it was last prepared for
  uint64_t used = 0;  // clock of its last prepare (least recently used is replaced)
};

}  // namespace

struct sr_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  DevBuf out_node, out_status, out_bytes, dmin, prof, scratch;
  HostBuf h_result, h_status, h_node, h_bytes;
  HostBuf h_early;           // mapped: K2's per-candidate result words (single-rank runs)
  HostBuf h_comm;            // pinned: the reduced words of a caller-provided collective
  // Device work of the last run may still be going (K2 planning the candidates past the winner, the ledger
  // kernel, the cost copy); settle() waits for it before a buffer moves.  The one rule, for every way a run
  // ends: set before the walk whenever device work of this run may outlive the call (also when the walk then
  // fails); cleared if and only if a wait of this run synchronised the stream (ResultWait::synced), or
  // copy_back did.  A run that ends with K3 leaves nothing behind once its words are there: K3 follows all
  // of it in stream order and the words are its last stores.
  bool in_flight = false;
  uint64_t* d_early = nullptr;  // device address of h_early
  uint64_t issued_checks = 0;  // checks of the prepared workload's plan (known after a full run)
  bool issued_known = false;
  std::vector<std::unique_ptr<Slot>> slots;  // SR_PLAN_SLOTS (default 4), made on first use
  int32_t n_slots = 4;
  Slot* cur = nullptr;       // the slot of the last prepare
  uint64_t slot_clock = 0;
  sr::TickLists lists;  // this call's patches, K0 lists and copies (prepare)
  sr::TickPlan plan;    // ... and its decisions
  int32_t k0_incremental = 1;  // SR_K0_INCREMENTAL=0: K0 always rewrites every row
  int32_t k0_skip = 1;         // SR_K0_SKIP=0: every run launches K0
  // SR_K2_SPLIT=0: one K2 launch.  Otherwise a work list the encoder split
  // (more entries than SR_K2_SPLIT_MIN, 4096: more waves than the chip holds
  // at once, with domain-path candidates) is planned by two kernels side by
  // side: the node-order candidates on the node-order kernel (fewer
  // registers, several waves per SIMD), the rest on the general kernel on a
  // second stream (C4's affinity variant, 15,000 entries: K2 142 -> 89 us; C3's,
  // 1,500, split too: 20 -> 39 us)
  int32_t k2_split = 1;
  // SR_LIST_COST=0: the work list stays longest-first by pod count.  Otherwise
  // the first run of a candidate generation records each candidate's K2 wave
  // duration, and the reused workloads of the next ticks dispatch the longest
  // waves first (a candidate whose pods scan far along their rows is short by
  // pod count but one of the longest waves: C4's last-starting waves)
  int32_t list_cost = 1;
  int32_t list_cost_min = 1024;  // SR_LIST_COST_MIN: only lists longer than this (C4 15,000 entries: K2 69 -> 45 us;
                                 // round 6, C3's 1,500: K2 -0.3 us, realistic C3 -0.7 us, affinity C3 16.3 -> 13.3 us;
                                 // C1 / C2 / C5's 300 entries keep the pod-count order)
  // SR_K2_COOP: a cost-ordered list's costliest entries planned by cooperative
  // blocks on the node-order kernel (four waves per block: the chain and
  // three waves scanning far resolutions with it); 0: none
  int32_t k2_coop = 64;
  // SR_K2_DISPATCH_EVENTS=0: the split launch's fork and join as marker
  // packets (hipEventRecord) instead of the completion signals of K0 and of
  // the general kernel's dispatch
  int32_t k2_dispatch_events = 1;
  DevBuf out_cycles;
  // sr_plan_sequence: the ledger of what each round decided (by the caller's
  // candidate and pod indices; K3 of a round fills it, one copy brings it down
  // at the end of the sequence) and the caller's cand_pod_off on the device
  DevBuf seq_status, seq_node, seq_off;
  HostBuf h_seq_status, h_seq_node, h_seq_off;
  // sr_plan_sequence_pdb: the candidates' needs {off, group, count} and the allowances, uploaded once per call
  // from h_pdb; the round's refused flags and {winner, active index} (seq_pdb.hip)
  DevBuf pdb_need, pdb_remaining, pdb_refused, pdb_win;
  HostBuf h_pdb;
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  uint64_t run_count = 0;      // runs of this context: d_min alternates between two buffers
  bool dmin_ready[2] = {false, false};  // buffer reset by the previous run's K2 (a K0-less run needs it)
  sr::EncoderCache enc;      // what the encoder keeps across calls (encode.cpp)
  hipEvent_t ev_upload = nullptr;  // the last upload (a staging buffer is reused after it)
  int32_t prefix_batch = 16;       // first batch of sr_plan_first (SR_PREFIX_BATCH; tools/gpu_prefix.sh)
  sr::DevWorkload dw{};
  bool prepared = false;
  int32_t timing = 0;        // SR_TIME_* kernel bits of the current setting
  int32_t timing_every = 1;  // sample every n-th run
  int64_t timing_runs = 0;   // runs since sr_set_timing
  int32_t timing_cur = 0;    // SR_TIME_* bits of the current run
  // HIP event pairs bracketing timed kernels, read back lazily (flush_timing)
  // so a timed run does not have to synchronise the stream.
  std::vector<hipEvent_t> ev_start, ev_end;
  std::vector<int8_t> ev_kernel;
  size_t ev_used = 0;
  uint32_t seq = 0;  // run sequence number (wraps: tags compare as uint32)
  sr_timing t{};
  ncclComm_t comm = nullptr;
  // sr_comm_init_shm: the ranks of one node reduce through host memory.  One
  // POSIX shared-memory segment holds, per rank and per tick parity, the
  // rank's published input words and the outcome words its K2 writes (mapped
  // into every rank's GPU); each rank's host walks them in global candidate
  // order up to the first drainable one (no collective, no K3: result_words.hpp,
  // DESIGN.md §7).
  struct Shm {
    uint64_t* host = nullptr;  // the segment (every rank's regions)
    uint64_t* dev = nullptr;   // its device address in this process
    size_t bytes = 0;
    int32_t max_cand = 0;      // input candidates per rank and call
    uint32_t session = 0;
    uint64_t tick = 0;         // runs through the segment (identical on every rank)
    int32_t base = -1;         // the prepared call's first local candidate (cand_global[0] / nranks), -1: none
    std::string name;
  } shm;
  sr_allreduce_min_fn host_fn = nullptr;  // sr_comm_init_host: the caller's allreduce(min)
  void* host_user = nullptr;
  int nranks = 1, rank = 0;
  int64_t last_rank_next = -1;  // reduced smallest unplanned global index of the last collective run (-1: none)
  FILE* prof_file = nullptr;  // SR_K2_PROFILE: per-wave K2 records appended per run
  int32_t k2_mode = 0;        // SR_K2_MODE=1: pod-order K2 only (A/B measurement)
  int32_t node_patch = 1;     // SR_NODE_PATCH=0: a changed node section always goes up whole
  int32_t k2_narrow = 1;      // SR_K2_NARROW: 32-bit scaled window visits in node order (0: 64-bit only)
  int32_t k2_wpb = 0;         // SR_K2_WPB: K2 waves per block (1, 2, 4; 0 = by list length)
  int32_t k2_excl = 1;        // SR_K2_EXCL: exclusive candidates (one host port) with the taken-mask step
  int32_t k2_map_regs = 1;    // SR_K2_MAP_REGS: the winner's mapping goes to the host from the wave's registers / LDS
  int32_t k2_node_kernel = 1; // SR_K2_NODE_KERNEL: node-order-only K2 kernel when every candidate takes that path
  int32_t s_head_only = 1;    // SR_S_HEAD_ONLY: K0 writes S-row heads only on rows wider than 64 words (0: never)
  sr::QueryCtx query;  // the query calls' state (query.hpp): device, stream and &err are set by sr_create
};

sr::QueryCtx* sr::query_ctx(sr_ctx* ctx) { return &ctx->query; }

namespace {

std::string& err_string(sr_ctx* ctx) { return ctx->err; }  // (for HIP_TRY)

sr_status hip_fail(sr_ctx* ctx, hipError_t e, const char* what) { return sr::hip_fail(ctx->err, e, what); }

// Run tags of every context of the process: a tag is never reused while the
// process lives (2^32 runs), so words a freed context left behind cannot match.
std::atomic<uint32_t> g_run_seq{0};

// A run may return while K2 still plans the candidates after the winner (the
// stream keeps later work in order); host-side reallocation of its buffers
// waits for it here.
sr_status settle(sr_ctx* ctx) {
  if (!ctx->in_flight) return SR_OK;
  ctx->in_flight = false;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return SR_OK;
}

// The stream fallback of a run's wait for its result words (sr::ResultWait): a failure is recorded as HIP_TRY
// records it.
bool sync_stream(void* user) {
  sr_ctx* ctx = static_cast<sr_ctx*>(user);
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) hip_fail(ctx, e, "hipStreamSynchronize(ctx->stream)");
  return e == hipSuccess;
}

// How a wait or a walk over the result words ended, as the caller sees it.  missing: what to say of an own
// word that was never written; silent_rank: ResultWait::silent_rank of a walk with peers.
sr_status words_status(sr_ctx* ctx, sr::WordsStatus st, const char* missing, int32_t silent_rank = -1) {
  switch (st) {
    case sr::kWordsOk:
      return SR_OK;
    case sr::kWordsSyncFailed:  // (sync_stream said why)
      return SR_ERR_HIP;
    case sr::kWordsPeerSilent:
      ctx->err = "rank " + std::to_string(silent_rank) + " published no outcome for this tick within 60 s";
      return SR_ERR_RCCL;
    case sr::kWordsNoCandidate:
      ctx->err = "ledger result names no candidate of this round";
      return SR_ERR_HIP;
    case sr::kWordsNotWritten:
      break;
  }
  ctx->err = missing;
  return SR_ERR_HIP;
}

sr::CandView cand_view(const sr::Workload& w) {
  return sr::CandView{w.cand_src.data(), w.cand_off.data(), w.status_host.data(),
                      static_cast<int32_t>(w.cand_global.size()), w.n_input_cand, w.max_cand_pods};
}

bool has_comm(const sr_ctx* ctx) { return ctx->comm != nullptr || ctx->host_fn != nullptr || ctx->shm.host != nullptr; }

// allreduce(min) of n <= 8 uint64 words in device memory, stream-ordered:
// RCCL in place, or the caller's collective on a pinned host copy.
sr_status allreduce_min_dev(sr_ctx* ctx, void* words, int32_t n) {
  if (ctx->comm) {
    ncclResult_t r = rccl().all_reduce(words, words, static_cast<size_t>(n), ncclUint64, ncclMin, ctx->comm,
                                       ctx->stream);
    if (r != ncclSuccess) {
      ctx->err = std::string("ncclAllReduce: ") + rccl().error_string(r);
      return SR_ERR_RCCL;
    }
    return SR_OK;
  }
  HIP_TRY(ctx, host_reserve(ctx->h_comm, 64));
  uint64_t* h = static_cast<uint64_t*>(ctx->h_comm.p);
  HIP_TRY(ctx, hipMemcpyAsync(h, words, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->host_fn(ctx->host_user, h, n) != 0) {
    ctx->err = "caller-provided allreduce(min) failed";
    return SR_ERR_RCCL;
  }
  HIP_TRY(ctx, hipMemcpyAsync(words, h, sizeof(uint64_t) * n, hipMemcpyHostToDevice, ctx->stream));
  return SR_OK;
}

// The slot for this input: the one last prepared for an input with the same
// fingerprint (the encoder then compares the input in full), else a new one
// while fewer than n_slots exist, else the least recently used.
Slot& pick_slot(sr_ctx* ctx, const sr_candidates* cands) {
  const int32_t n = cands->n_cand;
  uint64_t key = 0x5107ull + static_cast<uint64_t>(n);
  if (n > 0) {
    const int32_t b = cands->cand_pod_off[0], e = cands->cand_pod_off[n];
    auto mixin = [&](uint64_t x) { key = (key ^ x) * 0x100000001B3ull; };
    mixin(static_cast<uint32_t>(b));
    mixin(static_cast<uint32_t>(e));
    if (e > b) {
      mixin(static_cast<uint32_t>(cands->cand_pods[b]));
      mixin(static_cast<uint32_t>(cands->cand_pods[b + (e - b) / 2]));
      mixin(static_cast<uint32_t>(cands->cand_pods[e - 1]));
    }
    if (cands->cand_global) {
      mixin(static_cast<uint32_t>(cands->cand_global[0]));
      mixin(static_cast<uint32_t>(cands->cand_global[n - 1]));
    }
  }
  Slot* pick = nullptr;
  for (auto& sl : ctx->slots)
    if (sl->key == key) pick = sl.get();
  if (!pick && static_cast<int32_t>(ctx->slots.size()) < ctx->n_slots) {
    ctx->slots.push_back(std::make_unique<Slot>());
    pick = ctx->slots.back().get();
  }
  if (!pick) {
    pick = ctx->slots.front().get();
    for (auto& sl : ctx->slots)
      if (sl->used < pick->used) pick = sl.get();
  }
  pick->key = key;
  pick->used = ++ctx->slot_clock;
  return *pick;
}

// The shared-memory walk finds global index g on rank g % N: interleaved shards only.
sr_status check_shm_shards(sr_ctx* ctx, const sr_candidates* cands) {
  const int32_t n = cands->n_cand, N = ctx->nranks;
  if (n > ctx->shm.max_cand) {
    ctx->err = "more candidates than sr_comm_init_shm's max_cand";
    return SR_ERR_CAPACITY;
  }
  const int32_t* G = cands->cand_global;
  if (n > 0 && !G && N > 1) {
    ctx->err = "the shared-memory transport needs cand_global (interleaved shards)";
    return SR_ERR_INVALID_ARG;
  }
  const int64_t b = n > 0 && G ? G[0] / N : 0;
  for (int32_t i = 0; i < n; ++i)
    if ((G ? G[i] : i) != (b + i) * N + ctx->rank) {
      ctx->err = "the shared-memory transport needs interleaved shards: cand_global[i] = (first + i) * nranks + rank";
      return SR_ERR_INVALID_ARG;
    }
  ctx->shm.base = n > 0 ? static_cast<int32_t>(b) : -1;
  return SR_OK;
}

sr::ResidencySwitches switches(const sr_ctx* ctx) {
  sr::ResidencySwitches sw;
  sw.k0_skip = ctx->k0_skip;
  sw.k0_incremental = ctx->k0_incremental;
  sw.node_patch = ctx->node_patch;
  sw.list_cost = ctx->list_cost;
  sw.k2_mode = ctx->k2_mode;
  return sw;
}

// A reused workload's list in the order of its last run's K2 durations.
sr_status reorder_list(sr_ctx* ctx, Slot& sl) {
  HIP_TRY(ctx, hipEventSynchronize(sl.ev_cost));
  sr::reorder_list_by_cost(sl.wl, static_cast<const uint32_t*>(sl.h_cycles.p), ctx->enc.list_head, ctx->k2_coop);
  return SR_OK;
}

// The slot's arenas and tables and the context's output buffers, sized for
// this call; moved[0..2]: the staging, arena or tables allocation is a new one.
sr_status reserve_buffers(sr_ctx* ctx, Slot& sl, size_t arena_bytes, bool moved[3]) {
  const sr::Workload& w = sl.wl;
  const int32_t na = static_cast<int32_t>(w.pod_src.size());
  const int32_t ncand = static_cast<int32_t>(w.cand_global.size());
  if (ctx->ev_upload) HIP_TRY(ctx, hipEventSynchronize(ctx->ev_upload));  // staging buffer free again
  const size_t h_cap = sl.h_arena.cap;
  HIP_TRY(ctx, host_reserve(sl.h_arena, arena_bytes));
  moved[0] = sl.h_arena.cap != h_cap;
  const size_t arena_cap = sl.arena.cap;
  HIP_TRY(ctx, dev_reserve(sl.arena, arena_bytes));  // a new allocation holds no node records
  moved[1] = sl.arena.cap != arena_cap;
  const size_t n_rows = static_cast<size_t>(w.n_classes) + w.t_dim.size();
  const size_t row_bytes = static_cast<size_t>(w.Wp) * sizeof(uint64_t);
  const size_t t_cap = sl.tables.cap;
  HIP_TRY(ctx, dev_reserve(sl.tables, n_rows * row_bytes));
  moved[2] = sl.tables.cap != t_cap;
  HIP_TRY(ctx, dev_reserve(ctx->out_node, sizeof(int32_t) * std::max(1, na)));
  HIP_TRY(ctx, dev_reserve(ctx->out_status, sizeof(int32_t) * std::max(1, ncand)));
  HIP_TRY(ctx, dev_reserve(ctx->out_bytes, sizeof(uint32_t) * std::max(1, ncand)));
  HIP_TRY(ctx, dev_reserve(ctx->dmin, 64));
  const size_t res_bytes = sizeof(uint64_t) * (sr::kResultHeader + static_cast<size_t>(std::max(1, w.max_cand_pods)));
  HIP_TRY(ctx, host_reserve(ctx->h_result, res_bytes));  // mapped: K3 writes the result straight to the host
  HIP_TRY(ctx, host_reserve(ctx->h_early, sizeof(uint64_t) * (static_cast<size_t>(ncand) + na + 1)));
  return SR_OK;
}

// The copies resolve() listed, then ev_upload: kernels queue behind them.
sr_status queue_upload(sr_ctx* ctx, Slot& sl) {
  const char* hs = static_cast<const char*>(sl.h_arena.p);
  char* dv = static_cast<char*>(sl.arena.p);
  for (const sr::ArenaCopy& c : ctx->lists.copies)
    HIP_TRY(ctx, hipMemcpyAsync(dv + c.off, hs + c.off, c.bytes, hipMemcpyHostToDevice, ctx->stream));
  if (!ctx->ev_upload) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_upload, hipEventDisableTiming));
  HIP_TRY(ctx, hipEventRecord(ctx->ev_upload, ctx->stream));
  return SR_OK;
}

// The kernels' view of the prepared workload: pointers into the slot's arena
// by the tick's layout, the lists and switches the tick decided on.
sr_status fill_dev_workload(sr_ctx* ctx, Slot& sl) {
  const sr::Workload& w = sl.wl;
  const sr::TickPlan& p = ctx->plan;
  const sr::ArenaLayout& o = p.at;
  const sr::TickLists& tl = ctx->lists;
  const int32_t na = static_cast<int32_t>(w.pod_src.size());
  const int32_t ncand = static_cast<int32_t>(w.cand_global.size());
  char* base = static_cast<char*>(sl.arena.p);
  auto at = [base](size_t off) { return static_cast<void*>(base + off); };
  const bool dyn = o.dyn, ext = o.ext;
  sr::DevWorkload& d = ctx->dw;
  d = sr::DevWorkload{};
  d.n_spot = w.n_spot;
  d.n_pad = w.n_pad;
  d.Wp = w.Wp;
  d.node_rec = static_cast<const uint64_t*>(at(o.node_rec));
  d.node_free = static_cast<const int64_t*>(at(o.node_free));
  d.n_atoms = w.n_atoms;
  d.atoms = static_cast<const uint64_t*>(at(o.atoms));
  d.cls_prog_off = static_cast<const int32_t*>(at(o.cls_prog_off));
  d.cls_prog = static_cast<const int32_t*>(at(o.cls_prog));
  d.cls_prog8 = static_cast<const int32_t*>(at(o.cls_prog8));
  d.n_classes = w.n_classes;
  d.s_empty_off = w.empty_class >= 0 ? static_cast<uint32_t>(w.empty_class) * static_cast<uint32_t>(w.Wp) : 0xffffffffu;
  d.n_t = static_cast<int32_t>(w.t_dim.size());
  for (int i = 0; i < 5; ++i) d.t_off[i] = w.t_off[i];
  d.t_thr = static_cast<const int64_t*>(at(o.t_thr));
  d.n_pods = na;
  d.pod_rec = static_cast<const uint64_t*>(at(o.pod_rec));
  d.n_cand = ncand;
  d.cand_off = static_cast<const int32_t*>(at(o.cand_off));
  d.cand_global = static_cast<const int32_t*>(at(o.cand_global));
  d.list = static_cast<const int4*>(at(o.list));
  d.n_list = static_cast<int32_t>(w.list.size() / 4);
  d.n_list_head = std::min(d.n_list, sr::kListInline);
  for (int32_t i = 0; i < d.n_list_head; ++i)
    d.list_head[i] = int4{w.list[4 * i], w.list[4 * i + 1], w.list[4 * i + 2], w.list[4 * i + 3]};
  d.max_np = w.max_cand_pods;
  d.dyn_cand = dyn ? static_cast<const int32_t*>(at(o.dyn_cand)) : nullptr;
  d.dyn_pod = dyn ? static_cast<const uint64_t*>(at(o.dyn_pod)) : nullptr;
  d.dk_dom = dyn ? static_cast<const int32_t*>(at(o.dk_dom)) : nullptr;
  d.ds_info = dyn ? static_cast<const int32_t*>(at(o.ds_info)) : nullptr;
  d.sp_tab = dyn ? static_cast<const int32_t*>(at(o.sp_tab)) : nullptr;
  d.n_dk = w.n_dk;
  d.ext_cand = ext ? static_cast<const int32_t*>(at(o.ext_cand)) : nullptr;
  d.pod_ext = ext ? static_cast<const uint64_t*>(at(o.pod_ext)) : nullptr;
  d.list_ext = ext ? static_cast<const int4*>(at(o.list_ext)) : nullptr;
  d.node_scal = ext ? static_cast<const int64_t*>(at(o.node_scal)) : nullptr;
  static_assert(sr::kDevExtU64 == sr::kExtU64, "extension record layout shared by encode.cpp and kernels.hip");
  static_assert(sr::kDevDynU64 == sr::kDynU64 && sr::kDevDomKeys == sr::kDomKeys && sr::kDevDynTerms == sr::kDynTerms &&
                    sr::kDevSpreadSlots == sr::kSpreadSlots,
                "domain-path layout shared by encode.cpp and kernels.hip");
  for (int k = 0; k < sr::kDomKeys; ++k) d.dk_row[k] = w.dk_row[k];
  d.S = static_cast<uint64_t*>(sl.tables.p);
  d.T = d.S + static_cast<size_t>(w.n_classes) * w.Wp;
  d.out_node = static_cast<int32_t*>(ctx->out_node.p);
  d.out_status = static_cast<int32_t*>(ctx->out_status.p);
  d.out_bytes = static_cast<uint32_t*>(ctx->out_bytes.p);
  d.d_min = static_cast<int32_t*>(ctx->dmin.p);
  d.cand_floor = -1;  // a sequence round sets its own
  d.k2_mode = ctx->k2_mode;
  d.k2_narrow = ctx->k2_narrow;
  d.k2_wpb = ctx->k2_wpb;
  d.k2_excl = ctx->k2_excl;
  d.k2_map_regs = ctx->k2_map_regs;
  d.k2_node_kernel = ctx->k2_node_kernel;
  // Wide rows, every candidate on the node-order kernel and every class
  // program in its 8-slot record: K0 writes only the S-row heads, K2
  // evaluates S words beyond them from the programs.
  d.s_head_only = 0;
  if (ctx->s_head_only && w.Wp > 64 && sr::k2_node_launch(dyn, ctx->k2_mode, w.max_cand_pods, ctx->k2_node_kernel)) {
    bool short_programs = true;
    for (int32_t k = 0; k < w.n_classes && short_programs; ++k)
      short_programs = w.cls_prog8[static_cast<size_t>(k) * 8] != -2;
    d.s_head_only = short_programs ? 1 : 0;
  }
  d.swap_mask = w.swap_mask;
  d.rank_next = ~0ull;  // sr_plan_first sets its batch's value
  d.prof = nullptr;
  if (ctx->prof_file) {
    const size_t pbytes = sizeof(uint64_t) * (16 * static_cast<size_t>(std::max(1, ncand)) + 2 * sr::kK0ProfWaves);
    HIP_TRY(ctx, dev_reserve(ctx->prof, pbytes));
    HIP_TRY(ctx, hipMemsetAsync(ctx->prof.p, 0, pbytes, ctx->stream));
    d.prof = static_cast<uint64_t*>(ctx->prof.p);
  }
  void* dres = nullptr;
  HIP_TRY(ctx, hipHostGetDevicePointer(&dres, ctx->h_result.p, 0));
  d.result = static_cast<uint64_t*>(dres);
  HIP_TRY(ctx, hipHostGetDevicePointer(&dres, ctx->h_early.p, 0));
  ctx->d_early = static_cast<uint64_t*>(dres);
  d.res_stat = d.res_map = nullptr;  // set per run
  d.node_patch = p.n_node_patch ? static_cast<const uint64_t*>(at(o.node_patch)) : nullptr;
  d.n_node_patch = p.n_node_patch;
  d.k0_inc = p.k0_inc ? 1 : 0;
  d.n_k0_cols = static_cast<int32_t>(tl.k0_cols.size());
  d.n_k0_rows = static_cast<int32_t>(tl.k0_rows.size());
  d.k0_cols = tl.k0_cols.empty() ? nullptr : static_cast<const int32_t*>(at(o.k0_cols));
  d.k0_rows = tl.k0_rows.empty() ? nullptr : static_cast<const int32_t*>(at(o.k0_rows));
  d.pod_patch = p.n_pod_patch ? static_cast<const uint64_t*>(at(o.pod_patch)) : nullptr;
  d.n_pod_patch = p.n_pod_patch;
  d.k0_skip = p.skip ? 1 : 0;
  // the changed nodes of a K0-less run, one table entry per lane of a K2 wave (DevWorkload::dirty_tab); they
  // are the nodes of node_patch, in its order
  d.n_dirty = p.n_dirty;
  for (int32_t i = 0; i < p.n_dirty; ++i) {
    for (int dm = 0; dm < 3; ++dm) d.dirty_tab[16 * dm + i] = p.dirty_free[i][dm];
    const uint64_t* rec = tl.node_patch.data() + static_cast<size_t>(i) * sr::kNodePatchWords;
    if (p.n_node_patch != p.n_dirty || rec[0] != static_cast<uint64_t>(p.dirty_node[i])) {
      ctx->err = "K0-less run: the node patches are not the changed nodes";
      return SR_ERR_STATE;
    }
    d.dirty_tab[48 + i] = static_cast<int64_t>(static_cast<uint64_t>(static_cast<uint32_t>(p.dirty_node[i])) |
                                                 static_cast<uint64_t>(static_cast<uint32_t>(rec[5])) << 32);
  }
  static_assert(sr::kSkipDirty == 16 && sizeof(d.dirty_tab) == 64 * 8, "kSkipDirty nodes x 4 entries in the kernel arguments");
  d.first_fallback_local = w.first_fallback;
  static_assert(sr::kPodPatchU64 == sr::kPodPatchWords && sr::kNodePatchU64 == sr::kNodePatchWords &&
                    sr::kTPad == sr::kTSpare,
                "patch layout shared with encode.cpp and residency.cpp");
  return SR_OK;
}

// sr_timing of the prepared workload: its dimensions, what the encoder and the
// upload had to do, and K0's algorithmic bytes.
void account_prepare(sr_ctx* ctx, const sr::Workload& w, double ms_pack_host, double ms_upload) {
  const sr::DevWorkload& d = ctx->dw;
  const sr::TickPlan& p = ctx->plan;
  const std::vector<int32_t>& kcols = ctx->lists.k0_cols;
  const std::vector<int32_t>& krows = ctx->lists.k0_rows;
  ctx->t.bytes_uploaded = p.bytes_uploaded;
  const uint64_t row = static_cast<uint64_t>(w.Wp) * 8;
  // K0 algorithmic bytes: every table row written once; every atom row a class
  // program names, the nodes' free capacities and the thresholds read once.
  uint64_t atom_reads = w.cls_prog.size();
  const uint64_t s_row = d.s_head_only ? static_cast<uint64_t>(std::min(w.Wp, 8)) * 8 : row;  // S words K0 writes
  ctx->t.bytes_tables = static_cast<uint64_t>(w.n_classes) * s_row + w.t_dim.size() * row + atom_reads * s_row +
                        3ull * 8 * w.n_pad + 32ull * w.n_classes;
  if (p.k0_inc) {  // the changed columns of every row (S columns inside the written head), the moved rows whole
    const int32_t s_words = d.s_head_only ? std::min(w.Wp, 8) : w.Wp;
    uint64_t s_cols = 0;
    for (int32_t col : kcols) s_cols += col < s_words ? 1 : 0;
    ctx->t.bytes_tables = (static_cast<uint64_t>(w.n_classes) + atom_reads) * 8 * s_cols +
                          (32ull * w.n_classes) * (s_cols > 0 ? 1 : 0) + w.t_dim.size() * 8 * kcols.size() +
                          3ull * 64 * 8 * kcols.size() + krows.size() * (row + 8ull * w.n_pad);
  }
  // K2: counted by the kernel itself per candidate (out_bytes), read back by
  // the next run with status or node_of_pod outputs
  ctx->t.bytes_placement = 0;
  ctx->issued_known = false;
  ctx->issued_checks = 0;
  ctx->t.ms_pack_host = ms_pack_host;
  ctx->t.ms_upload = ms_upload;
  ctx->t.n_pods = d.n_pods;
  ctx->t.n_spot = w.n_spot;
  ctx->t.n_cand = d.n_cand;
  ctx->t.n_words = w.Wp;
  ctx->t.n_rows_static = d.n_classes;
  ctx->t.n_rows_threshold = d.n_t;
  ctx->t.n_classes = w.n_classes;
  ctx->t.enc_new_specs = ctx->enc.last_new_specs;
  ctx->t.enc_static_rebuilt = ctx->enc.last_static_changed;
  ctx->t.enc_state_nodes = ctx->enc.last_state_changed;
  ctx->t.enc_memo_pods = ctx->enc.last_memo_hits;
  ctx->t.enc_reused = ctx->enc.last_reused;
  ctx->t.enc_pod_patches = ctx->enc.last_pod_patches;
  ctx->t.k0_columns = p.skip ? -2 : p.k0_inc ? static_cast<int32_t>(kcols.size()) : -1;
  ctx->t.k0_rows_moved = p.k0_inc ? static_cast<int32_t>(krows.size()) : 0;
  ctx->t.k0_dirty_nodes = p.skip ? static_cast<int32_t>(ctx->lists.node_patch.size() / sr::kNodePatchWords) : 0;
  if (p.skip) ctx->t.bytes_tables = 0;
}

sr_status prepare(sr_ctx* ctx, const sr_snapshot* snap, const sr_cluster* c, const sr_candidates* cands) {
  using ms = std::chrono::duration<double, std::milli>;
  auto t0 = std::chrono::steady_clock::now();
  ctx->prepared = false;
  sr_status st = ctx->shm.host ? check_shm_shards(ctx, cands) : SR_OK;
  if (st != SR_OK) return st;
  Slot& sl = pick_slot(ctx, cands);
  ctx->cur = &sl;
  sr::Workload& w = sl.wl;
  std::string err;
  st = sr::encode_workload(&ctx->enc, snap, c, cands, &w, &err);
  if (st != SR_OK) {
    ctx->err = err;
    sl.res.encode_failed();
    return st;
  }
  const sr::ResidencySwitches sw = switches(ctx);
  sr::TickPlan& p = ctx->plan;
  sl.res.observe(w, ctx->enc, sw, &ctx->lists, &p);

  HIP_TRY(ctx, hipSetDevice(ctx->device));
  st = settle(ctx);
  if (st == SR_OK && p.reorder_due) st = reorder_list(ctx, sl);
  if (st != SR_OK) return st;
  bool moved[3] = {false, false, false};
  st = reserve_buffers(ctx, sl, p.at.bytes, moved);
  if (st != SR_OK) {
    sl.res.moved(moved[0], moved[1], moved[2]);  // (the next prepare must not take a new allocation for the old one)
    return st;
  }
  auto t1 = std::chrono::steady_clock::now();
  sl.res.resolve(w, ctx->enc, sw, moved[0], moved[1], moved[2], p.reorder_due, static_cast<char*>(sl.h_arena.p),
                 &ctx->lists, &p);
  st = queue_upload(ctx, sl);
  if (st != SR_OK) return st;
  sl.res.upload_queued(w, p);
  ctx->t.k2_list_by_cost = sl.res.list_by_cost(w) ? 1 : 0;
  auto t2 = std::chrono::steady_clock::now();
  st = fill_dev_workload(ctx, sl);
  if (st != SR_OK) return st;
  account_prepare(ctx, w, ms(t1 - t0).count(), ms(t2 - t1).count());
  ctx->prepared = true;
  return SR_OK;
}

sr_status flush_timing(sr_ctx* ctx) {
  if (ctx->ev_used == 0) return SR_OK;
  HIP_TRY(ctx, hipEventSynchronize(ctx->ev_end[ctx->ev_used - 1]));
  double* sums[4] = {&ctx->t.ms_tables, &ctx->t.ms_placement, &ctx->t.ms_winner, &ctx->t.ms_collective};
  for (size_t i = 0; i < ctx->ev_used; ++i) {
    float ms = 0;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev_start[i], ctx->ev_end[i]));
    *sums[ctx->ev_kernel[i]] += ms;
  }
  ctx->ev_used = 0;
  return SR_OK;
}

// The end of a single-rank winner-only run (sr::walk_early): K2's words up to the first drainable candidate,
// then its mapping.
sr_status finish_early(sr_ctx* ctx, sr_plan_out* out) {
  const sr::Workload& w = ctx->cur->wl;
  const sr::DevWorkload& d = ctx->dw;
  if (ctx->timing_cur) ctx->t.n_runs += 1;
  const volatile uint64_t* stat = static_cast<const volatile uint64_t*>(ctx->h_early.p);
  ctx->in_flight = true;
  sr::ResultWait wait(sync_stream, ctx);
  const sr::Walk r = sr::walk_early(stat, stat + d.n_cand, cand_view(w), d.seq, wait);
  if (wait.synced()) ctx->in_flight = false;
  if (r.st != sr::kWordsOk) return words_status(ctx, r.st, "K2 result word not written by this run");
  out->first_fallback = w.first_fallback;
  out->first_ok = r.winner >= 0 ? w.cand_global[r.winner] : -1;
  out->winner = (out->first_ok >= 0 && (w.first_fallback < 0 || w.first_fallback > out->first_ok)) ? out->first_ok : -1;
  out->winner_npods = r.np;
  if (out->winner_map) sr::copy_values(r.map, r.np, out->winner_map);
  out->checks_dense = static_cast<uint64_t>(d.n_pods) * static_cast<uint64_t>(w.n_spot);
  out->fallback_pods = w.fallback_pods;
  out->checks = ctx->issued_known ? ctx->issued_checks : 0;
  return SR_OK;
}

// One round of sr_plan_sequence, host side.
struct SeqWalk {
  int32_t floor = -1;     // in: the cursor (candidates at or below it were judged in earlier rounds)
  int32_t winner = -1;    // out: the round's first drainable candidate, in the caller's indices
  int32_t fallback = -1;  // out: the fallback candidate the walk stopped at
  int32_t end = -1;       // out: the last candidate the walk judged (below the fallback it stopped at)
  std::vector<int32_t> map;  // out: the winner's mapping
  // sr_plan_sequence_pdb: the needs and the host's mirror of the device's allowances (null: no limits), and the
  // round's first unrefused fallback candidate above the floor (INT32_MAX: none)
  sr::PdbLedger* pdb = nullptr;
  int32_t stop = INT32_MAX;
};

// The end of a sequence round: K2's words above the floor (sr::walk_sequence), or under disruption budgets the
// ledger step's (sr::walk_ledger: that step runs after the whole of K2, and K2 wrote no other candidate's
// mapping to the host).  The ledger copy may still run when the words are there.
sr_status finish_sequence(sr_ctx* ctx, SeqWalk* sq) {
  const sr::Workload& w = ctx->cur->wl;
  const sr::DevWorkload& d = ctx->dw;
  if (ctx->timing_cur) ctx->t.n_runs += 1;
  const volatile uint64_t* stat = static_cast<const volatile uint64_t*>(ctx->h_early.p);
  const volatile uint64_t* res = static_cast<const volatile uint64_t*>(ctx->h_result.p);
  ctx->in_flight = true;
  sr::ResultWait wait(sync_stream, ctx);
  const sr::Walk r = sq->pdb ? sr::walk_ledger(res, sr::kPdbHeader, cand_view(w), d.seq, sq->floor, sq->stop, wait)
                             : sr::walk_sequence(stat, stat + d.n_cand, cand_view(w), d.seq, sq->floor, wait);
  if (wait.synced()) ctx->in_flight = false;
  sq->winner = r.winner;
  sq->fallback = r.fallback;
  sq->end = r.end;
  if (r.st != sr::kWordsOk)
    return words_status(ctx, r.st, sq->pdb ? "ledger result word not written by this round"
                                           : "K2 result word not written by this run");
  if (r.winner >= 0) {
    sq->map.resize(static_cast<size_t>(r.np));
    sr::copy_values(r.map, r.np, sq->map.data());
  }
  return SR_OK;
}

#define SR_TRY(expr)                   \
  do {                                 \
    sr_status _st = (expr);            \
    if (_st != SR_OK) return _st;      \
  } while (0)

// Timed kernels get an event pair from the pool, recorded by their own
// dispatch (hipExtLaunchKernelGGL); the collective is bracketed with
// plain records.  Events are read back lazily (flush_timing).
// k: 0 = K0, 1 = K2, 2 = K3, 3 = the collective (mask bit 2, with K3);
// both null when the current run does not time kernel k
sr_status event_pair(sr_ctx* ctx, int k, hipEvent_t* a, hipEvent_t* b) {
  *a = *b = nullptr;
  if (!(ctx->timing_cur >> (k == 3 ? 2 : k) & 1)) return SR_OK;
  if (ctx->ev_used == ctx->ev_start.size()) {
    if (ctx->ev_used >= 3072) {  // bounded pool: read back what is pending
      SR_TRY(flush_timing(ctx));
    } else {
      hipEvent_t e0, e1;
      HIP_TRY(ctx, hipEventCreate(&e0));
      HIP_TRY(ctx, hipEventCreate(&e1));
      ctx->ev_start.push_back(e0);
      ctx->ev_end.push_back(e1);
      ctx->ev_kernel.push_back(0);
    }
  }
  const size_t i = ctx->ev_used++;
  ctx->ev_kernel[i] = static_cast<int8_t>(k);
  *a = ctx->ev_start[i];
  *b = ctx->ev_end[i];
  return SR_OK;
}

// K0 (with the slot's commit of what it writes), or on a K0-less run the reset
// of d_min when no K2 of a previous run did it.  forked: K0's dispatch signals
// the split launch's fork event itself (K0 untimed: no marker packet between
// K0 and K2, ~5 us per marker on the split tick).
sr_status queue_tables(sr_ctx* ctx, Slot& sl, bool split, int par, hipEvent_t e0a, hipEvent_t e0b, bool* forked) {
  const sr::DevWorkload& d = ctx->dw;
  *forked = false;
  if (d.k0_skip) {
    if (!ctx->dmin_ready[par])  // no K2 of a previous run reset it: reset here
      HIP_TRY(ctx, hipMemsetAsync(d.d_min, 0xff, sizeof(uint64_t), ctx->stream));
  } else {
    *forked = split && !e0b && ctx->k2_dispatch_events;
    HIP_TRY(ctx, sr::launch_tables(d, sl.wl.first_fallback, ctx->stream, e0a, *forked ? ctx->ev_fork : e0b));
    sl.res.k0_queued(sl.wl);
  }
  ctx->dmin_ready[par] = false;
  ctx->dmin_ready[1 - par] = d.n_list > 0;  // K2's first candidate resets it
  return SR_OK;
}

// K2: one launch, or the split launch (see sr_ctx::k2_split): the node-order
// part on this stream, the general one on stream2 between a fork and a join
// event.
sr_status queue_placement(sr_ctx* ctx, Slot& sl, bool split, bool forked, hipEvent_t e1a, hipEvent_t e1b) {
  const sr::Workload& w = sl.wl;
  sr::DevWorkload& d = ctx->dw;
  hipStream_t s = ctx->stream;
  const int32_t n_node = w.n_list_node;
  ctx->t.k2_launches = d.n_list > 0 ? (split ? 2 : 1) : 0;
  // cooperative blocks for the front of a cost-ordered list, on a node-order
  // launch of four waves per block without extension records
  d.n_coop = 0;
  const bool node_launch = split || sr::k2_node_launch(d.dyn_cand != nullptr, d.k2_mode, d.max_np, d.k2_node_kernel);
  const int32_t len = split ? n_node : d.n_list;
  if (node_launch && sr::k2_waves_per_block(d.k2_wpb, len) == 4 && !d.ext_cand && sl.res.list_by_cost(w))
    d.n_coop = std::min(w.n_coop_front, len);
  ctx->t.k2_coop = d.n_coop;
  if (!split) {
    HIP_TRY(ctx, sr::launch_placement(d, s, e1a, e1b));
    return SR_OK;
  }
  sr::DevWorkload dp = d, dn = d;
  dp.list = d.list + n_node;
  dp.n_list = d.n_list - n_node;
  dp.n_list_head = 0;
  dp.n_coop = 0;  // (the general kernel)
  if (d.list_ext) dp.list_ext = d.list_ext + n_node;
  dn.n_list = n_node;
  dn.n_list_head = std::min(d.n_list_head, n_node);
  dn.max_np = w.max_np_node;
  dn.dyn_cand = nullptr;  // none of its candidates is on the domain path
  if (e1a) HIP_TRY(ctx, hipEventRecord(e1a, s));
  if (!forked) HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, s));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
  // the join is the general kernel's own completion signal
  HIP_TRY(ctx, sr::launch_placement(dp, ctx->stream2, nullptr, ctx->k2_dispatch_events ? ctx->ev_join : nullptr));
  if (!ctx->k2_dispatch_events) HIP_TRY(ctx, hipEventRecord(ctx->ev_join, ctx->stream2));
  HIP_TRY(ctx, sr::launch_placement(dn, s, nullptr, nullptr));
  HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->ev_join, 0));
  if (e1b) HIP_TRY(ctx, hipEventRecord(e1b, s));
  return SR_OK;
}

// A sequence round's ledger kernel after K2 (after the join of a split launch).
sr_status queue_sequence(sr_ctx* ctx, const sr::Workload& w, const SeqWalk& sq) {
  const sr::DevWorkload& d = ctx->dw;
  sr::SeqRound r{};
  r.d_min = d.d_min;
  r.cand_global = d.cand_global;
  r.cand_off = d.cand_off;
  r.out_status = d.out_status;
  r.out_node = d.out_node;
  r.in_off = static_cast<const int32_t*>(ctx->seq_off.p);
  r.n_cand = d.n_cand;
  r.floor = sq.floor;
  r.fb_stop = sr::first_fallback_above(cand_view(w), sq.floor);
  r.seq_status = static_cast<int32_t*>(ctx->seq_status.p);
  r.seq_node = static_cast<int32_t*>(ctx->seq_node.p);
  HIP_TRY(ctx, sr::launch_sequence(r, ctx->stream));
  return SR_OK;
}

// ... under disruption budgets: the step that finds the round's winner itself.
sr_status queue_sequence_pdb(sr_ctx* ctx, const SeqWalk& sq) {
  const sr::DevWorkload& d = ctx->dw;
  const int32_t* need = static_cast<const int32_t*>(ctx->pdb_need.p);
  const size_t n = sq.pdb->need_off.size() - 1, nn = sq.pdb->need_group.size();
  sr::SeqPdbRound p{};
  p.r.d_min = d.d_min;
  p.r.cand_global = d.cand_global;
  p.r.cand_off = d.cand_off;
  p.r.out_status = d.out_status;
  p.r.out_node = d.out_node;
  p.r.in_off = static_cast<const int32_t*>(ctx->seq_off.p);
  p.r.n_cand = d.n_cand;
  p.r.floor = sq.floor;
  p.r.fb_stop = sq.stop;
  p.r.seq_status = static_cast<int32_t*>(ctx->seq_status.p);
  p.r.seq_node = static_cast<int32_t*>(ctx->seq_node.p);
  p.need_off = need;
  p.need_group = need + n + 1;
  p.need_count = need + n + 1 + nn;
  p.remaining = static_cast<int32_t*>(ctx->pdb_remaining.p);
  p.refused = static_cast<uint8_t*>(ctx->pdb_refused.p);
  p.win = static_cast<int32_t*>(ctx->pdb_win.p);
  p.words = d.result;  // (sized by prepare for the longest candidate; a sequence round launches no K3)
  p.seq = d.seq;
  HIP_TRY(ctx, sr::launch_sequence_pdb(p, ctx->stream));
  return SR_OK;
}

// The collective (first ok, first fallback, rank_next) and K3.
sr_status queue_winner(sr_ctx* ctx, bool collective) {
  hipStream_t s = ctx->stream;
  hipEvent_t e2a, e2b, eca, ecb;
  SR_TRY(event_pair(ctx, 2, &e2a, &e2b));
  if (collective) {
    SR_TRY(event_pair(ctx, 3, &eca, &ecb));
    if (eca) HIP_TRY(ctx, hipEventRecord(eca, s));
    SR_TRY(allreduce_min_dev(ctx, ctx->dw.d_min, 3));
    if (ecb) HIP_TRY(ctx, hipEventRecord(ecb, s));
  }
  HIP_TRY(ctx, sr::launch_winner(ctx->dw, s, e2a, e2b));
  return SR_OK;
}

// A full run (or a profiled one): the per-candidate outcomes come down and the
// stream is waited for.
sr_status copy_back(sr_ctx* ctx, bool full) {
  const sr::DevWorkload& d = ctx->dw;
  hipStream_t s = ctx->stream;
  const int32_t na = d.n_pods, ncand = d.n_cand;
  if (full) {
    HIP_TRY(ctx, host_reserve(ctx->h_status, sizeof(int32_t) * std::max(1, ncand)));
    HIP_TRY(ctx, host_reserve(ctx->h_node, sizeof(int32_t) * std::max(1, na)));
    HIP_TRY(ctx, host_reserve(ctx->h_bytes, sizeof(uint32_t) * std::max(1, ncand)));
    if (ncand) {
      HIP_TRY(ctx, hipMemcpyAsync(ctx->h_status.p, d.out_status, sizeof(int32_t) * ncand, hipMemcpyDeviceToHost, s));
      HIP_TRY(ctx, hipMemcpyAsync(ctx->h_bytes.p, d.out_bytes, sizeof(uint32_t) * ncand, hipMemcpyDeviceToHost, s));
    }
    if (na) HIP_TRY(ctx, hipMemcpyAsync(ctx->h_node.p, d.out_node, sizeof(int32_t) * na, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(ctx, hipStreamSynchronize(s));
  ctx->in_flight = false;  // (an earlier winner-only run's K2 has finished too)
  return SR_OK;
}

// A winner-only run that ends with K3: its header, then the winner's mapping, polled instead of waking up on
// stream completion (sr::poll_header; a header still missing after the stream fallback is read_result's error).
sr_status poll_result(sr_ctx* ctx) {
  sr::ResultWait wait(sync_stream, ctx);
  const sr::WordsStatus st = sr::poll_header(static_cast<const volatile uint64_t*>(ctx->h_result.p),
                                             sr::kResultHeader, ctx->dw.seq, wait);
  return words_status(ctx, st, "result header not written by this run");
}

// The shared-memory transport, before K2: this rank's input words and header for the run's tick (its tag is the
// run's), once every rank has finished the tick that used the region before; K2 writes its outcome words there.
sr_status shm_publish(sr_ctx* ctx, int* par) {
  auto& S = ctx->shm;
  sr::DevWorkload& d = ctx->dw;
  const sr::Workload& w = ctx->cur->wl;
  const sr::ShmSeg seg{S.host, S.max_cand, ctx->nranks, ctx->rank, S.session};
  sr::ResultWait wait(sync_stream, ctx);  // (other ranks' words only)
  const sr::ShmPublished pub = sr::shm_publish(seg, ++S.tick, cand_view(w), S.base, w.first_fallback, d.rank_next, wait);
  SR_TRY(words_status(ctx, pub.st, "", wait.silent_rank()));
  ctx->seq = d.seq = pub.tag;
  d.res_stat = S.dev + (pub.stat - S.host);
  d.res_map = ctx->d_early + d.n_cand;
  *par = pub.p;
  return SR_OK;
}

// ... after K2: every rank's outcome words in global order into the result words, as K3 would write them
// (sr::shm_reduce; ms_collective: this host walk).  A winner-only walk returns at the winner: this rank's K2 may
// still plan the candidates after it (res_map in h_early, out_status, out_bytes, out_cycles), as after
// finish_early.  `waited`: copy_back has synchronised the stream.
sr_status walk_shm(sr_ctx* ctx, int shm_par, bool waited) {
  const auto t0 = std::chrono::steady_clock::now();
  const auto& S = ctx->shm;
  const sr::ShmSeg seg{S.host, S.max_cand, ctx->nranks, ctx->rank, S.session};
  if (!waited) ctx->in_flight = true;
  sr::ResultWait wait(sync_stream, ctx);
  const sr::WordsStatus st =
      sr::shm_reduce(seg, shm_par, ctx->dw.seq, cand_view(ctx->cur->wl),
                     static_cast<const volatile uint64_t*>(ctx->h_early.p) + ctx->dw.n_cand,
                     static_cast<volatile uint64_t*>(ctx->h_result.p), sr::kResultHeader, wait);
  if (wait.synced()) ctx->in_flight = false;
  SR_TRY(words_status(ctx, st, "K2 outcome word not written by this run", wait.silent_rank()));
  const auto t1 = std::chrono::steady_clock::now();
  if (ctx->timing_cur & 4) ctx->t.ms_collective += std::chrono::duration<double, std::milli>(t1 - t0).count();
  return SR_OK;
}

// The run's result words (K3's, or the shared-memory walk's) into `out`; a
// full run adds the per-candidate outcomes copy_back brought down.
sr_status read_result(sr_ctx* ctx, sr_plan_out* out, bool full) {
  const sr::Workload& w = ctx->cur->wl;
  const sr::DevWorkload& d = ctx->dw;
  const int32_t na = d.n_pods, ncand = d.n_cand;
  const sr::Header h = sr::read_header(static_cast<const volatile uint64_t*>(ctx->h_result.p), sr::kResultHeader, d.seq);
  SR_TRY(words_status(ctx, h.st, "result header not written by this run"));
  out->first_ok = h.first_ok;
  out->first_fallback = h.first_fallback;
  ctx->last_rank_next = h.rank_next;
  out->winner = (h.first_ok >= 0 && (h.first_fallback < 0 || h.first_fallback > h.first_ok)) ? h.first_ok : -1;
  out->winner_npods = h.np;
  if (out->winner_map) sr::copy_values(h.map, h.np, out->winner_map);
  out->checks_dense = static_cast<uint64_t>(na) * static_cast<uint64_t>(w.n_spot);
  out->fallback_pods = w.fallback_pods;
  if (full) {
    const int32_t* hs = static_cast<const int32_t*>(ctx->h_status.p);
    const int32_t* hn = static_cast<const int32_t*>(ctx->h_node.p);
    const uint32_t* hb = static_cast<const uint32_t*>(ctx->h_bytes.p);
    if (out->status) {
      for (int32_t i = 0; i < w.n_input_cand; ++i) out->status[i] = w.status_host[i];
      for (int32_t k = 0; k < ncand; ++k) out->status[w.cand_src[k]] = hs[k];
    }
    // K2's own byte counts; the reference's CheckPredicates calls for the same
    // plan: findSpotNodeForPod stops at the first fit (position + 1 calls) and
    // scans every spot node for a pod that fits nowhere, where canDrainNode stops
    uint64_t bytes = 0, issued = 0;
    for (int32_t k = 0; k < ncand; ++k) {
      bytes += hb[k];
      const int32_t o = w.cand_off[k], np = w.cand_off[k + 1] - o;
      const int32_t done = hs[k] >= 0 ? std::min(np, hs[k]) : np;
      for (int32_t q = 0; q < done; ++q) issued += static_cast<uint64_t>(hn[o + q]) + 1;
      if (hs[k] >= 0) issued += static_cast<uint64_t>(w.n_spot);
    }
    ctx->t.bytes_placement = bytes;
    ctx->issued_checks = issued;
    ctx->issued_known = true;
    if (out->node_of_pod) {
      for (int32_t i = 0; i < w.n_input_pods; ++i) out->node_of_pod[i] = -1;
      for (int32_t q = 0; q < na; ++q) out->node_of_pod[w.pod_src[q] - w.pod_base] = hn[q];
    }
  }
  out->checks = ctx->issued_known ? ctx->issued_checks : 0;
  return SR_OK;
}

sr_status run(sr_ctx* ctx, sr_plan_out* out, bool full, bool use_comm, SeqWalk* sq = nullptr) {
  if (!ctx->prepared) {
    ctx->err = "sr_plan_run before sr_plan_prepare";
    return SR_ERR_STATE;
  }
  Slot& sl = *ctx->cur;
  const sr::Workload& w = sl.wl;
  sr::DevWorkload& d = ctx->dw;
  hipStream_t s = ctx->stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const bool collective = has_comm(ctx) && use_comm;
  // Single rank, winner only: K2 writes each candidate's outcome to the host
  // and the run returns once the candidates up to the winner are known (no K3)
  const bool early = !collective && !full && (!ctx->prof_file || sq);
  ctx->timing_cur = (ctx->timing_runs++ % ctx->timing_every) == 0 ? ctx->timing : 0;
  do ctx->seq = g_run_seq.fetch_add(1, std::memory_order_relaxed) + 1;
  while (ctx->seq == 0);  // tag 0 is never used: fresh result memory holds zeros
  d.seq = ctx->seq;
  hipEvent_t e0a = nullptr, e0b = nullptr;  // K0's pair only when it is launched (an unrecorded event fails)
  if (!d.k0_skip) SR_TRY(event_pair(ctx, 0, &e0a, &e0b));
  // the first run of a candidate generation records its K2 durations (list_cost)
  const bool want_cost = ctx->list_cost && d.n_list > ctx->list_cost_min && sl.res.want_cost(w);
  d.out_cycles = nullptr;
  if (want_cost) {
    HIP_TRY(ctx, dev_reserve(ctx->out_cycles, sizeof(uint32_t) * static_cast<size_t>(d.n_cand)));
    HIP_TRY(ctx, host_reserve(sl.h_cycles, sizeof(uint32_t) * static_cast<size_t>(d.n_cand)));
    if (!sl.ev_cost) HIP_TRY(ctx, hipEventCreateWithFlags(&sl.ev_cost, hipEventDisableTiming));
    d.out_cycles = static_cast<uint32_t*>(ctx->out_cycles.p);
  }
  // d_min alternates between two buffers: K0 resets this run's, K2 the next's
  const int par = static_cast<int>(ctx->run_count++ & 1);
  d.d_min = static_cast<int32_t*>(ctx->dmin.p) + 8 * par;
  d.d_min_next = static_cast<int32_t*>(ctx->dmin.p) + 8 * (1 - par);
  // the split launch: the encoder put the node-order candidates first
  const bool split = ctx->k2_split && w.n_list_node > 0 && w.n_list_node < d.n_list &&
                     sr::k2_node_launch(false, d.k2_mode, w.max_np_node, d.k2_node_kernel);
  if (split && !ctx->stream2) {
    HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
    HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
  }
  bool forked = false;
  SR_TRY(queue_tables(ctx, sl, split, par, e0a, e0b, &forked));
  hipEvent_t e1a, e1b;
  SR_TRY(event_pair(ctx, 1, &e1a, &e1b));
  const bool shm = collective && ctx->shm.host;  // ranks reduce through host memory: no collective, no K3
  int shm_par = 0;
  if (early) {
    d.res_stat = ctx->d_early;
    d.res_map = ctx->d_early + d.n_cand;
  } else if (shm) {
    SR_TRY(shm_publish(ctx, &shm_par));
  } else {
    d.res_stat = d.res_map = nullptr;
  }
  SR_TRY(queue_placement(ctx, sl, split, forked, e1a, e1b));
  if (want_cost) {  // after K2 in stream order: the next prepare waits for it (ev_cost)
    HIP_TRY(ctx, hipMemcpyAsync(sl.h_cycles.p, d.out_cycles, sizeof(uint32_t) * static_cast<size_t>(d.n_cand),
                                hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipEventRecord(sl.ev_cost, s));
    sl.res.cost_queued(w);
  }
  if (sq) {  // a sequence round: the ledger after K2, then the walk
    SR_TRY(sq->pdb ? queue_sequence_pdb(ctx, *sq) : queue_sequence(ctx, w, *sq));
    return finish_sequence(ctx, sq);
  }
  if (early) return finish_early(ctx, out);
  if (!shm) SR_TRY(queue_winner(ctx, collective));  // the shared-memory transport has neither (walk_shm below)
  if (ctx->timing_cur) ctx->t.n_runs += 1;
  const bool waited = full || ctx->prof_file;
  if (waited) SR_TRY(copy_back(ctx, full));
  else if (!shm) SR_TRY(poll_result(ctx));
  if (shm) SR_TRY(walk_shm(ctx, shm_par, waited));  // (waits for the outcome words it needs)
  if (ctx->prof_file && d.n_cand > 0) {  // diagnostics only (tools/k2_profile.py)
    std::vector<uint64_t> pr(static_cast<size_t>(d.n_cand) * 16 + 2 * sr::kK0ProfWaves);
    HIP_TRY(ctx, hipMemcpy(pr.data(), d.prof, pr.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    const int64_t hdr[2] = {d.n_cand, static_cast<int64_t>(sr::kK0ProfWaves)};
    std::fwrite(hdr, sizeof(hdr), 1, ctx->prof_file);
    std::fwrite(pr.data(), sizeof(uint64_t), pr.size(), ctx->prof_file);
    std::fflush(ctx->prof_file);
  }
  return read_result(ctx, out, full);
}
#undef SR_TRY

}  // namespace

static sr_status plan_first(sr_ctx* ctx, const sr_snapshot* snap, const sr_cluster* c, const sr_candidates* cands,
                            sr_plan_out* out);

extern "C" {

#define SR_STR2(x) #x
#define SR_STR(x) SR_STR2(x)
const char* sr_build_info(void) {
  return "srplanner abi=" SR_STR(SR_ABI_VERSION) " target=gfx950 kernels=K0-tables,K2-placement(fused feasibility),K3-winner";
}

int32_t sr_abi_version(void) { return SR_ABI_VERSION; }

sr_status sr_create(int32_t device, sr_ctx** out) {
  if (!out) return SR_ERR_INVALID_ARG;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return SR_ERR_NO_DEVICE;
  if (device < 0 || device >= count) return SR_ERR_INVALID_ARG;
  auto* ctx = new sr_ctx();
  ctx->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return SR_ERR_HIP;
  }
  ctx->query.device = device;
  ctx->query.stream = ctx->stream;
  ctx->query.err = &ctx->err;
  if (const char* path = std::getenv("SR_K2_PROFILE")) ctx->prof_file = std::fopen(path, "ab");
  if (const char* m = std::getenv("SR_K2_MODE")) ctx->k2_mode = std::atoi(m) == 1 ? 1 : 0;
  if (const char* m = std::getenv("SR_NODE_PATCH")) ctx->node_patch = std::atoi(m) != 0;
  if (const char* m = std::getenv("SR_K2_NARROW")) ctx->k2_narrow = std::atoi(m) != 0;
  if (const char* m = std::getenv("SR_K2_NODE_KERNEL")) ctx->k2_node_kernel = std::atoi(m) != 0;
  if (const char* m = std::getenv("SR_S_HEAD_ONLY")) ctx->s_head_only = std::atoi(m) != 0;
  if (const char* b = std::getenv("SR_PREFIX_BATCH")) ctx->prefix_batch = std::max(1, std::atoi(b));
  if (const char* m = std::getenv("SR_K2_WPB")) ctx->k2_wpb = std::atoi(m);
  if (const char* m = std::getenv("SR_K2_EXCL")) ctx->k2_excl = std::atoi(m) != 0;
  if (const char* m = std::getenv("SR_PLAN_SLOTS")) ctx->n_slots = std::max(1, std::min(16, std::atoi(m)));
  if (const char* m = std::getenv("SR_K0_INCREMENTAL")) ctx->k0_incremental = std::atoi(m) != 0;
  if (const char* m = std::getenv("SR_K0_SKIP")) ctx->k0_skip = std::atoi(m) != 0;
  if (const char* m = std::getenv("SR_K2_SPLIT")) ctx->k2_split = std::atoi(m) != 0;
  if (const char* m = std::getenv("SR_LIST_COST")) ctx->list_cost = std::atoi(m) != 0;
  if (const char* m = std::getenv("SR_LIST_COST_MIN")) ctx->list_cost_min = std::max(0, std::atoi(m));
  if (const char* m = std::getenv("SR_K2_SPLIT_MIN")) ctx->enc.split_min = std::max(0, std::atoi(m));
  if (const char* m = std::getenv("SR_K2_DISPATCH_EVENTS")) ctx->k2_dispatch_events = std::atoi(m) != 0;
  if (const char* m = std::getenv("SR_LIST_HEAD")) ctx->enc.list_head = std::max(0, std::atoi(m));
  if (const char* m = std::getenv("SR_K2_MAP_REGS")) ctx->k2_map_regs = std::atoi(m) != 0;
  if (const char* m = std::getenv("SR_K2_COOP")) ctx->k2_coop = std::max(0, std::atoi(m));
  *out = ctx;
  return SR_OK;
}

void sr_destroy(sr_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->comm) (void)rccl().comm_destroy(ctx->comm);
  if (ctx->shm.host) {
    if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
    (void)hipHostUnregister(ctx->shm.host);
    munmap(ctx->shm.host, ctx->shm.bytes);
    if (ctx->rank == 0) shm_unlink(ctx->shm.name.c_str());  // the ranks keep their mappings
  }
  for (DevBuf* b : {&ctx->out_node, &ctx->out_status, &ctx->out_bytes, &ctx->dmin, &ctx->prof,
                    &ctx->scratch, &ctx->seq_status, &ctx->seq_node, &ctx->seq_off, &ctx->pdb_need, &ctx->pdb_remaining,
                    &ctx->pdb_refused, &ctx->pdb_win, &ctx->query.x_in, &ctx->query.x_out, &ctx->query.x_view,
                    &ctx->query.e_scratch})
    if (b->p) (void)hipFree(b->p);
  if (ctx->ev_upload) (void)hipEventDestroy(ctx->ev_upload);
  if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
  for (hipEvent_t e : {ctx->ev_fork, ctx->ev_join})
    if (e) (void)hipEventDestroy(e);
  if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
  if (ctx->out_cycles.p) (void)hipFree(ctx->out_cycles.p);
  for (HostBuf* b : {&ctx->h_result, &ctx->h_status, &ctx->h_node, &ctx->h_bytes, &ctx->h_early, &ctx->h_comm,
                     &ctx->h_seq_status, &ctx->h_seq_node, &ctx->h_seq_off, &ctx->h_pdb, &ctx->query.hx_in,
                     &ctx->query.hx_out, &ctx->query.hx_view})
    if (b->p) (void)hipHostFree(b->p);
  for (auto& sl : ctx->slots) {
    if (sl->arena.p) (void)hipFree(sl->arena.p);
    if (sl->tables.p) (void)hipFree(sl->tables.p);
    if (sl->h_arena.p) (void)hipHostFree(sl->h_arena.p);
    if (sl->h_cycles.p) (void)hipHostFree(sl->h_cycles.p);
    if (sl->ev_cost) (void)hipEventDestroy(sl->ev_cost);
  }
  for (auto* v : {&ctx->ev_start, &ctx->ev_end})
    for (hipEvent_t e : *v) (void)hipEventDestroy(e);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->prof_file) std::fclose(ctx->prof_file);
  delete ctx;
}

const char* sr_last_error(const sr_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

sr_status sr_plan_first(sr_ctx* ctx, const sr_snapshot* snap, const sr_cluster* cluster, const sr_candidates* cands,
                        sr_plan_out* out) {
  if (!ctx || !snap || !cluster || !cands || !out || cands->n_cand < 0) return SR_ERR_INVALID_ARG;
  return plan_first(ctx, snap, cluster, cands, out);
}

sr_status sr_plan_prepare(sr_ctx* ctx, const sr_snapshot* snap, const sr_cluster* cluster, const sr_candidates* cands) {
  if (!ctx || !snap || !cluster || !cands || cands->n_cand < 0) return SR_ERR_INVALID_ARG;
  return prepare(ctx, snap, cluster, cands);
}

sr_status sr_plan_run(sr_ctx* ctx, sr_plan_out* out) {
  if (!ctx || !out) return SR_ERR_INVALID_ARG;
  return run(ctx, out, out->status != nullptr || out->node_of_pod != nullptr, true);
}

sr_status sr_plan(sr_ctx* ctx, const sr_snapshot* snap, const sr_cluster* cluster, const sr_candidates* cands,
                  sr_plan_out* out) {
  if (!ctx || !snap || !cluster || !cands || !out || cands->n_cand < 0) return SR_ERR_INVALID_ARG;
  sr_status st = prepare(ctx, snap, cluster, cands);
  if (st != SR_OK) return st;
  return run(ctx, out, out->status != nullptr || out->node_of_pod != nullptr, true);
}

// run()'s loop with its break (rescheduler.go:228-287): prefix batches of
// candidates, each encoded and planned on its own, until the first drainable
// candidate is known.  Batch k covers local candidates [lo_k, hi_k) on every
// rank.  The run's collective also reduces the smallest global index some rank
// has not planned yet (rank_next): a drainable candidate below it is the first
// overall, whatever the partition of the global indices over the ranks (with
// contiguous shards, rank 1's early batches hold late indices, and batching
// goes on until rank 0 has planned everything below them).  Every rank sees the
// same reduced values, so all stop after the same batch.
static sr_status plan_first(sr_ctx* ctx, const sr_snapshot* snap, const sr_cluster* c, const sr_candidates* cands,
                            sr_plan_out* out) {
  const int32_t n = cands->n_cand;
  const int32_t* off = cands->cand_pod_off;
  const bool full = out->status != nullptr || out->node_of_pod != nullptr;
  if (out->status)
    for (int32_t i = 0; i < n; ++i) out->status[i] = SR_CAND_SKIPPED;
  if (out->node_of_pod && n > 0)
    for (int32_t i = 0; i < off[n] - off[0]; ++i) out->node_of_pod[i] = -1;
  std::vector<int32_t> glob;
  if (!cands->cand_global) {
    glob.resize(static_cast<size_t>(std::max(0, n)));
    for (int32_t i = 0; i < n; ++i) glob[i] = i;
  }
  const int32_t* G = cands->cand_global ? cands->cand_global : glob.data();
  // suffix minima of the global indices: the smallest one not planned after a batch ending at l
  std::vector<int32_t> next(static_cast<size_t>(std::max(0, n)) + 1, INT32_MAX);
  int32_t maxp = 1;
  for (int32_t i = n - 1; i >= 0; --i) {
    if (G[i] < 0) {
      ctx->err = "cand_global holds a negative index";
      return SR_ERR_INVALID_ARG;
    }
    next[i] = std::min(next[i + 1], G[i]);
    maxp = std::max(maxp, off[i + 1] - off[i]);
  }
  out->winner = out->first_ok = out->first_fallback = -1;
  out->winner_npods = 0;
  out->checks = out->fallback_pods = out->checks_dense = 0;
  std::vector<int32_t> bst, bnode, bmap(out->winner_map ? static_cast<size_t>(maxp) : 0);
  const bool coll = has_comm(ctx);
  int32_t batches = 0;
  for (int32_t lo = 0, B = ctx->prefix_batch;; B = std::min(B * 2, 1 << 20)) {
    const int32_t hi = static_cast<int32_t>(std::min<int64_t>(INT32_MAX, static_cast<int64_t>(lo) + B));
    const int32_t l0 = std::min(lo, n), l1 = std::min(hi, n);
    sr_candidates sub{l1 - l0, off + l0, cands->cand_pods, G + l0};
    sr_plan_out o{};
    o.winner_map = out->winner_map ? bmap.data() : nullptr;
    if (full) {
      bst.assign(static_cast<size_t>(std::max(1, l1 - l0)), 0);
      bnode.assign(static_cast<size_t>(std::max(1, n > 0 ? off[l1] - off[l0] : 0)), -1);
      o.status = bst.data();
      o.node_of_pod = bnode.data();
    }
    sr_status st = prepare(ctx, snap, c, &sub);
    if (st != SR_OK) return st;
    ctx->dw.rank_next = next[l1] == INT32_MAX ? ~0ull : static_cast<uint64_t>(next[l1]);
    st = run(ctx, &o, full, true);
    if (st != SR_OK) return st;
    ++batches;
    if (full) {
      if (out->status) std::copy(bst.begin(), bst.begin() + (l1 - l0), out->status + l0);
      if (out->node_of_pod && n > 0) std::copy(bnode.begin(), bnode.begin() + (off[l1] - off[l0]), out->node_of_pod + (off[l0] - off[0]));
    }
    out->checks += o.checks;
    out->checks_dense += o.checks_dense;
    out->fallback_pods += o.fallback_pods;
    if (o.first_fallback >= 0 && (out->first_fallback < 0 || o.first_fallback < out->first_fallback))
      out->first_fallback = o.first_fallback;
    if (o.first_ok >= 0 && (out->first_ok < 0 || o.first_ok < out->first_ok)) {
      out->first_ok = o.first_ok;
      out->winner_npods = o.winner_npods;  // 0 on the ranks that do not own it
      if (out->winner_map)
        std::copy(bmap.begin(), bmap.begin() + o.winner_npods, out->winner_map);
    }
    // the smallest global index no rank has planned yet (reduced by the run's collective)
    const int64_t bound = coll ? (ctx->last_rank_next < 0 ? INT64_MAX : ctx->last_rank_next)
                               : (next[l1] == INT32_MAX ? INT64_MAX : next[l1]);
    if (bound == INT64_MAX || (out->first_ok >= 0 && out->first_ok < bound)) break;
    lo = hi;
  }
  out->winner = (out->first_ok >= 0 && (out->first_fallback < 0 || out->first_fallback > out->first_ok))
                    ? out->first_ok : -1;
  ctx->t.prefix_batches = batches;
  return SR_OK;
}

// Several consistent drains in one tick: rounds over the whole
// candidate list -- the same cand_pod_off / cand_pods / stamps every round, so
// the encoder's candidate-side reuse applies and a round's prepare re-encodes
// the spot nodes the last commit touched.  A round plans every candidate above
// the cursor from the current snapshot (K2 skips the others: cand_floor); its
// first drainable candidate is the next drain, the candidates between the
// cursor and it failed against the state the serial pass would have shown them.
// With limits (sr_plan_sequence_pdb) a round's refused set is
// fixed by the allowances the last commit left: the host's mirror decides
// which fallback candidate stops the round and whether a round is needed, the
// device's ledger step finds the winner among the unrefused candidates.
static sr_status plan_sequence(sr_ctx* ctx, sr_snapshot* snap, const sr_cluster* cluster, const sr_candidates* cands,
                               const sr_pdb_limits* limits, sr_sequence_out* out) {
  if (!ctx || !snap || !cluster || !cands || !out || cands->n_cand < 0) return SR_ERR_INVALID_ARG;
  const int32_t n = cands->n_cand;
  out->n_drained = out->rounds = out->rounds_k0 = out->rounds_reused = 0;
  out->stop = SR_SEQ_END;
  out->stop_cand = -1;
  if (cands->cand_global) {
    ctx->err = "sr_plan_sequence plans one GPU's whole candidate list: cand_global must be NULL";
    return SR_ERR_INVALID_ARG;
  }
  if (out->max_drains < 1 || out->first_cand < 0 || out->first_cand > n || (n > 0 && !out->drained)) {
    ctx->err = "sr_plan_sequence: max_drains < 1, first_cand out of range or no drained array";
    return SR_ERR_INVALID_ARG;
  }
  if (has_comm(ctx)) {
    ctx->err = "sr_plan_sequence with a communicator attached (single GPU only)";
    return SR_ERR_STATE;
  }
  if (snap->forked) {
    ctx->err = "sr_plan_sequence on a forked snapshot";
    return SR_ERR_STATE;
  }
  const int32_t* off = cands->cand_pod_off;
  const int32_t n_pods = n > 0 ? off[n] - off[0] : 0;
  sr::PdbLedger pdb;
  const bool limited = limits && limits->n_groups != 0;
  if (limited) {
    if (const char* why = sr::pdb_validate(limits->n_groups, limits->allowed, limits->pod_group, n_pods)) {
      ctx->err = why;
      return SR_ERR_INVALID_ARG;
    }
    sr::pdb_build(n, off, limits->n_groups, limits->allowed, limits->pod_group, &pdb);
  }
  // limits->remaining follows the commits, also when a later round fails
  struct Remaining {
    const sr::PdbLedger& l;
    int32_t* out;
    ~Remaining() {
      if (out) std::copy(l.remaining.begin(), l.remaining.end(), out);
    }
  } remaining_out{pdb, limited ? limits->remaining : nullptr};
  const bool want = out->status != nullptr || out->node_of_pod != nullptr;
  // what the host knows of each candidate: 0 not judged, 1 judged on the device (the ledger), 2 no pods, 3 fallback,
  // 4 refused (decided by the host: a fallback candidate, or no round ran)
  std::vector<uint8_t> how(static_cast<size_t>(n), 0);
  int32_t cursor = out->first_cand - 1;
  bool ledger = false;  // the device arrays are sized and cand_pod_off is up
  SeqWalk sq;
  if (limited) sq.pdb = &pdb;
  for (;;) {
    // candidates without pods need no round (rescheduler.go:260-264); no round when nothing else is left
    int32_t next = cursor + 1;
    while (next < n && off[next + 1] == off[next]) how[next++] = 2;
    if (next >= n) break;  // SR_SEQ_END
    sr_status st = prepare(ctx, snap, cluster, cands);
    if (st != SR_OK) return st;
    const sr::Workload& w = ctx->cur->wl;
    sq.floor = cursor;
    bool any_active = !w.cand_src.empty() && w.cand_src.back() > cursor;
    if (limited) {  // no round when every candidate with pods below the stop is refused or host-decided
      sq.stop = sr::pdb_first_stop(pdb, cursor, n, [&](int32_t i) { return w.status_host[i] == SR_CAND_FALLBACK; });
      any_active = false;
      for (auto k = std::upper_bound(w.cand_src.begin(), w.cand_src.end(), cursor);
           k != w.cand_src.end() && *k < sq.stop && !any_active; ++k)
        any_active = !pdb.refused(*k);
    }
    const bool in_round = any_active;
    if (any_active) {
      if (!ledger) {  // (after prepare's settle: no earlier kernel reads them)
        HIP_TRY(ctx, dev_reserve(ctx->seq_status, sizeof(int32_t) * static_cast<size_t>(n)));
        HIP_TRY(ctx, dev_reserve(ctx->seq_node, sizeof(int32_t) * static_cast<size_t>(std::max(1, n_pods))));
        HIP_TRY(ctx, dev_reserve(ctx->seq_off, sizeof(int32_t) * (static_cast<size_t>(n) + 1)));
        HIP_TRY(ctx, host_reserve(ctx->h_seq_off, sizeof(int32_t) * (static_cast<size_t>(n) + 1)));
        std::memcpy(ctx->h_seq_off.p, off, sizeof(int32_t) * (static_cast<size_t>(n) + 1));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->seq_off.p, ctx->h_seq_off.p, sizeof(int32_t) * (static_cast<size_t>(n) + 1),
                                    hipMemcpyHostToDevice, ctx->stream));
        if (limited) {  // the needs and the allowances go up once per call; the device commits by itself
          const size_t nn = pdb.need_group.size(), ng = pdb.remaining.size();
          const size_t need_words = static_cast<size_t>(n) + 1 + 2 * nn;
          HIP_TRY(ctx, dev_reserve(ctx->pdb_need, sizeof(int32_t) * need_words));
          HIP_TRY(ctx, dev_reserve(ctx->pdb_remaining, sizeof(int32_t) * ng));
          HIP_TRY(ctx, dev_reserve(ctx->pdb_refused, static_cast<size_t>(n)));
          HIP_TRY(ctx, dev_reserve(ctx->pdb_win, 2 * sizeof(int32_t)));
          HIP_TRY(ctx, host_reserve(ctx->h_pdb, sizeof(int32_t) * (need_words + ng)));
          int32_t* up = static_cast<int32_t*>(ctx->h_pdb.p);
          std::copy(pdb.need_off.begin(), pdb.need_off.end(), up);
          std::copy(pdb.need_group.begin(), pdb.need_group.end(), up + n + 1);
          std::copy(pdb.need_count.begin(), pdb.need_count.end(), up + n + 1 + nn);
          std::copy(pdb.remaining.begin(), pdb.remaining.end(), up + need_words);
          HIP_TRY(ctx, hipMemcpyAsync(ctx->pdb_need.p, up, sizeof(int32_t) * need_words, hipMemcpyHostToDevice,
                                      ctx->stream));
          HIP_TRY(ctx, hipMemcpyAsync(ctx->pdb_remaining.p, up + need_words, sizeof(int32_t) * ng,
                                      hipMemcpyHostToDevice, ctx->stream));
        }
        ledger = true;
      }
      ctx->dw.cand_floor = cursor;
      ctx->dw.prof = nullptr;  // (SR_K2_PROFILE records whole runs)
      sr_plan_out o{};
      st = run(ctx, &o, false, false, &sq);
      ctx->dw.cand_floor = -1;  // (the launches hold their copy: a later sr_plan_run of this workload plans everything)
      if (st != SR_OK) return st;
      out->rounds += 1;
      out->rounds_k0 += ctx->dw.k0_skip ? 0 : 1;
      out->rounds_reused += ctx->t.enc_reused ? 1 : 0;
    } else {  // every candidate above the cursor is decided by the host
      sq.winner = sq.fallback = -1;
      sq.end = n - 1;
      const int32_t fb = limited ? sq.stop : sr::first_fallback_above(cand_view(w), cursor);
      if (fb != INT32_MAX) sq.fallback = fb, sq.end = fb - 1;
    }
    for (int32_t i = cursor + 1; i <= sq.end; ++i) {
      how[i] = w.status_host[i] == SR_CAND_EMPTY ? 2 : 1;
      // a refused candidate the round's K2 planned is in the ledger as refused (the allowances are still the round's)
      if (limited && how[i] == 1 && pdb.refused(i) &&
          !(in_round && std::binary_search(w.cand_src.begin(), w.cand_src.end(), i)))
        how[i] = 4;
    }
    if (sq.winner < 0) {
      if (sq.fallback >= 0) {
        how[sq.fallback] = 3;
        out->stop = SR_SEQ_FALLBACK;
        out->stop_cand = sq.fallback;
      }
      break;
    }
    // the commit: the winner's pods stay on their planned nodes (rescheduler.go:366)
    const int32_t c = sq.winner, np = off[c + 1] - off[c];
    if (static_cast<int32_t>(sq.map.size()) != np) {
      ctx->err = "sr_plan_sequence: the winner's mapping does not cover its pods";
      return SR_ERR_HIP;
    }
    for (int32_t q = 0; q < np; ++q) {
      if (sq.map[q] < 0 || sq.map[q] >= sr_snapshot_num_nodes(snap)) {
        ctx->err = "sr_plan_sequence: the winner's mapping names no spot node";
        return SR_ERR_HIP;
      }
    }
    for (int32_t q = 0; q < np; ++q) sr::snapshot_add_pod(snap, cluster, cands->cand_pods[off[c] + q], sq.map[q]);
    out->drained[out->n_drained++] = c;
    if (limited) pdb.commit(c);
    cursor = c;
    if (out->n_drained == out->max_drains) {
      out->stop = SR_SEQ_BUDGET;
      break;
    }
  }
  if (want) {
    const int32_t* hs = nullptr;
    const int32_t* hn = nullptr;
    if (ledger) {  // the one copy of the sequence (waits for the last round's K2 and ledger kernel)
      HIP_TRY(ctx, host_reserve(ctx->h_seq_status, sizeof(int32_t) * static_cast<size_t>(n)));
      HIP_TRY(ctx, host_reserve(ctx->h_seq_node, sizeof(int32_t) * static_cast<size_t>(std::max(1, n_pods))));
      HIP_TRY(ctx, hipMemcpyAsync(ctx->h_seq_status.p, ctx->seq_status.p, sizeof(int32_t) * static_cast<size_t>(n),
                                  hipMemcpyDeviceToHost, ctx->stream));
      if (n_pods > 0)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_seq_node.p, ctx->seq_node.p, sizeof(int32_t) * static_cast<size_t>(n_pods),
                                    hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      ctx->in_flight = false;
      hs = static_cast<const int32_t*>(ctx->h_seq_status.p);
      hn = static_cast<const int32_t*>(ctx->h_seq_node.p);
    }
    for (int32_t i = 0; i < n; ++i) {
      const bool dev = how[i] == 1;
      if (out->status)
        out->status[i] = dev ? hs[i] : how[i] == 2 ? SR_CAND_EMPTY : how[i] == 3 ? SR_CAND_FALLBACK
                                   : how[i] == 4 ? SR_CAND_PDB : SR_CAND_SKIPPED;
      if (out->node_of_pod)
        for (int32_t q = off[i] - off[0]; q < off[i + 1] - off[0]; ++q) out->node_of_pod[q] = dev ? hn[q] : -1;
    }
  }
  return SR_OK;
}

sr_status sr_plan_sequence(sr_ctx* ctx, sr_snapshot* snap, const sr_cluster* cluster, const sr_candidates* cands,
                           sr_sequence_out* out) {
  return plan_sequence(ctx, snap, cluster, cands, nullptr, out);
}

sr_status sr_plan_sequence_pdb(sr_ctx* ctx, sr_snapshot* snap, const sr_cluster* cluster, const sr_candidates* cands,
                               const sr_pdb_limits* limits, sr_sequence_out* out) {
  return plan_sequence(ctx, snap, cluster, cands, limits, out);
}

// Single-process helpers (no collective): findSpotNodeForPod / canDrainNode.
static sr_status plan_local(sr_ctx* ctx, const sr_snapshot* snap, const sr_cluster* cluster,
                            const sr_candidates* cands, sr_plan_out* out) {
  sr_status st = prepare(ctx, snap, cluster, cands);
  if (st != SR_OK) return st;
  return run(ctx, out, true, false);
}

sr_status sr_find_spot_nodes(sr_ctx* ctx, const sr_snapshot* snap, const sr_cluster* cluster, const int32_t* pods,
                             int32_t n, int32_t* out_spot_pos, uint8_t* out_fallback) {
  if (!ctx || !snap || !cluster || n < 0 || (n > 0 && (!pods || !out_spot_pos))) return SR_ERR_INVALID_ARG;
  if (n == 0) return SR_OK;
  std::vector<int32_t> off(static_cast<size_t>(n) + 1), status(n);
  for (int32_t i = 0; i <= n; ++i) off[i] = i;
  sr_candidates c{n, off.data(), pods, nullptr};
  sr_plan_out o{};
  o.status = status.data();
  o.node_of_pod = out_spot_pos;
  sr_status st = plan_local(ctx, snap, cluster, &c, &o);
  if (st != SR_OK) return st;
  if (out_fallback)
    for (int32_t i = 0; i < n; ++i) out_fallback[i] = status[i] == SR_CAND_FALLBACK ? 1 : 0;
  return SR_OK;
}

sr_status sr_can_drain_node(sr_ctx* ctx, sr_snapshot* snap, const sr_cluster* cluster, const int32_t* pods,
                            int32_t n, int32_t* out_node_of_pod, int32_t* out_fail_pod, uint8_t* out_fallback) {
  if (!ctx || !snap || !cluster || n < 0 || (n > 0 && !pods) || !out_fail_pod) return SR_ERR_INVALID_ARG;
  std::vector<int32_t> map(static_cast<size_t>(std::max(1, n)), -1);
  int32_t off[2] = {0, n}, status = SR_CAND_EMPTY;
  if (out_fallback) *out_fallback = 0;
  *out_fail_pod = -1;
  if (n > 0) {
    sr_candidates c{1, off, pods, nullptr};
    sr_plan_out o{};
    o.status = &status;
    o.node_of_pod = map.data();
    sr_status st = plan_local(ctx, snap, cluster, &c, &o);
    if (st != SR_OK) return st;
    if (status == SR_CAND_FALLBACK) {
      if (out_fallback) *out_fallback = 1;
      if (out_node_of_pod)
        for (int32_t i = 0; i < n; ++i) out_node_of_pod[i] = -1;
      return SR_OK;
    }
    *out_fail_pod = status >= 0 ? status : -1;
    // Side effect of the reference: every placed pod is added to the snapshot
    // (rescheduler.go:366), also those before a failing pod.
    for (int32_t i = 0; i < n; ++i)
      if (map[i] >= 0) sr::snapshot_add_pod(snap, cluster, pods[i], map[i]);
  }
  if (out_node_of_pod)
    for (int32_t i = 0; i < n; ++i) out_node_of_pod[i] = map[i];
  return SR_OK;
}

sr_status sr_set_timing(sr_ctx* ctx, int32_t mask) {
  if (!ctx) return SR_ERR_INVALID_ARG;
  sr_status st = flush_timing(ctx);
  if (st != SR_OK) return st;
  ctx->timing = mask & 7;
  ctx->timing_every = std::max(1, (mask >> 8) & 0xffff);
  ctx->timing_runs = 0;
  ctx->t.n_runs = 0;
  ctx->t.ms_tables = ctx->t.ms_placement = ctx->t.ms_winner = ctx->t.ms_collective = 0;
  return SR_OK;
}

sr_status sr_get_timing(sr_ctx* ctx, sr_timing* out) {
  if (!ctx || !out) return SR_ERR_INVALID_ARG;
  sr_status st = flush_timing(ctx);
  if (st != SR_OK) return st;
  *out = ctx->t;
  return SR_OK;
}

sr_status sr_comm_unique_id(uint8_t out[SR_UNIQUE_ID_BYTES]) {
  if (!out) return SR_ERR_INVALID_ARG;
  ncclUniqueId id;
  static_assert(sizeof(id) == SR_UNIQUE_ID_BYTES, "ncclUniqueId size");
  if (!rccl().ok || rccl().get_unique_id(&id) != ncclSuccess) return SR_ERR_RCCL;
  std::memcpy(out, &id, sizeof(id));
  return SR_OK;
}

sr_status sr_comm_init_shm(sr_ctx* ctx, const char* name, uint32_t session, int32_t nranks, int32_t rank,
                           int32_t max_cand) {
  if (!ctx || !name || name[0] != '/' || nranks < 1 || rank < 0 || rank >= nranks || max_cand < 1 ||
      max_cand > (1 << 28) || has_comm(ctx))
    return SR_ERR_INVALID_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) return SR_ERR_HIP;
  const size_t words = static_cast<size_t>(nranks) * 2 * sr::shm_region_words(max_cand);
  const size_t bytes = (words * sizeof(uint64_t) + 4095) & ~size_t(4095);
  const int fd = shm_open(name, O_CREAT | O_RDWR, 0600);
  if (fd < 0) {
    ctx->err = std::string("shm_open(") + name + "): " + std::strerror(errno);
    return SR_ERR_RCCL;
  }
  struct stat sb;
  if (fstat(fd, &sb) != 0 || (sb.st_size != 0 && static_cast<size_t>(sb.st_size) != bytes) ||
      (sb.st_size == 0 && ftruncate(fd, static_cast<off_t>(bytes)) != 0)) {  // every rank sizes it alike
    ctx->err = std::string("shared segment ") + name + ": size mismatch or " + std::strerror(errno) +
               " (every rank passes the same nranks and max_cand)";
    close(fd);
    return SR_ERR_RCCL;
  }
  void* p = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  close(fd);
  if (p == MAP_FAILED) {
    ctx->err = std::string("mmap: ") + std::strerror(errno);
    return SR_ERR_RCCL;
  }
  void* dp = nullptr;
  hipError_t e = hipHostRegister(p, bytes, hipHostRegisterMapped);
  if (e == hipSuccess) e = hipHostGetDevicePointer(&dp, p, 0);
  if (e != hipSuccess) {
    munmap(p, bytes);
    return hip_fail(ctx, e, "hipHostRegister(shared segment)");
  }
  auto& S = ctx->shm;
  S.host = static_cast<uint64_t*>(p);
  S.dev = static_cast<uint64_t*>(dp);
  S.bytes = bytes;
  S.max_cand = max_cand;
  S.session = session;
  S.tick = 0;
  S.name = name;
  ctx->nranks = nranks;
  ctx->rank = rank;
  return SR_OK;
}

sr_status sr_comm_init_host(sr_ctx* ctx, int32_t nranks, int32_t rank, sr_allreduce_min_fn fn, void* user) {
  if (!ctx || !fn || nranks < 1 || rank < 0 || rank >= nranks || has_comm(ctx)) return SR_ERR_INVALID_ARG;
  ctx->host_fn = fn;
  ctx->host_user = user;
  ctx->nranks = nranks;
  ctx->rank = rank;
  return SR_OK;
}

sr_status sr_comm_init(sr_ctx* ctx, const uint8_t id[SR_UNIQUE_ID_BYTES], int32_t nranks, int32_t rank) {
  if (!ctx || !id || nranks < 1 || rank < 0 || rank >= nranks || has_comm(ctx)) return SR_ERR_INVALID_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess) return SR_ERR_HIP;
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  if (!rccl().ok) {
    ctx->err = "RCCL (librccl.so) could not be loaded";
    return SR_ERR_RCCL;
  }
  ncclResult_t r = rccl().comm_init_rank(&ctx->comm, nranks, uid, rank);
  if (r != ncclSuccess) {
    ctx->err = std::string("ncclCommInitRank: ") + rccl().error_string(r);
    ctx->comm = nullptr;
    return SR_ERR_RCCL;
  }
  ctx->nranks = nranks;
  ctx->rank = rank;
  return SR_OK;
}

}  // extern "C"
