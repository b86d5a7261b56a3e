// residency.hpp — what a workload slot's staging arena, device arena and
// tables still hold from earlier ticks, and how little a tick has to send up.
// Plain host arithmetic (no HIP): the planner hands in three booleans (did the
// staging, arena or tables allocation move) and executes the copies this unit
// lists; tools/encode_stats' `residency` mode checks it on the CPU.
#pragma once

#include <cstring>
#include <vector>

#include "host.hpp"
#include "launch_shape.hpp"

namespace sr {

constexpr size_t kDirtyMax = 64;       // changed nodes tracked since the last K0 run (more: the list is dropped)
constexpr size_t kSkipDirty = 16;      // ... a K0-less run carries (DevWorkload::dirty_tab)
constexpr size_t kPatchNodes = 16;     // ... sent as node patches instead of the whole node section
constexpr size_t kAtomsLogMax = 256;   // atom rows logged since the version both copies may lag to
constexpr size_t kK0ColsMax = 32;      // word columns / T rows of an incremental K0 (more: every row)
constexpr size_t kK0RowsMax = 256;
constexpr size_t kAtomRowCopies = 32;  // atom rows copied one by one (more: the atoms whole)
constexpr int kNodePatchWords = 12;    // {node, node_rec[8], node_free[3]} (kernels.hpp kNodePatchU64)

// Packs host vectors into one contiguous staging buffer (256-B aligned
// sections) so the whole workload goes up in a single copy.
class Packer {
 public:
  template <class T>
  size_t add(const std::vector<T>& v) {
    size_t off = (size_ + 255) & ~size_t(255);
    items_.push_back({off, v.data(), v.size() * sizeof(T)});
    size_ = off + v.size() * sizeof(T);
    return off;
  }
  size_t size() const { return (size_ + 255) & ~size_t(255); }
  void copy_to(char* dst, size_t from = 0) const {  // the sections at or after `from`
    for (const auto& it : items_)
      if (it.bytes && it.off >= from) std::memcpy(dst + it.off, it.src, it.bytes);
  }
  void clear() { items_.clear(), size_ = 0; }

 private:
  struct Item {
    size_t off;
    const void* src;
    size_t bytes;
  };
  std::vector<Item> items_;
  size_t size_ = 0;
};

// Arena: the node section (spot nodes' records and free values), the
// candidate section (class programs, pod records, candidate lists, domain
// path and extension records: one candidate generation, w.cand_gen), then
// this call's tick section (atoms, thresholds, patches).  Sections the
// device already holds are not copied again.
struct ArenaLayout {
  size_t node_rec = 0, node_free = 0;
  size_t node_bytes = 0;  // end of the node section
  size_t cls_prog_off = 0, cls_prog = 0, cls_prog8 = 0, pod_rec = 0, cand_off = 0, cand_global = 0, list = 0;
  bool dyn = false, ext = false;  // the call has domain-path candidates / extension records (else their offsets are 0)
  size_t dyn_cand = 0, dyn_pod = 0, ds_info = 0;
  size_t ext_cand = 0, pod_ext = 0, list_ext = 0;
  // the tick section: the atoms (rows a reuse encode changed go up alone),
  // then what follows the spot nodes' state every tick
  size_t atoms = 0;
  size_t tick_rest = 0;  // end of the atoms
  size_t node_scal = 0;  // the spot nodes' scalar usage
  size_t sp_tab = 0;     // the domain path's base counts
  size_t dk_dom = 0;     // ... and node domains (the spot order may move)
  size_t t_thr = 0;
  size_t node_patch = 0, pod_patch = 0, k0_cols = 0, k0_rows = 0;  // this call's lists (0: empty)
  size_t bytes = 0;
};

// One host-to-device copy of the arena (the same range of staging and device).
struct ArenaCopy {
  size_t off, bytes;
  bool counted;  // in sr_timing::bytes_uploaded (the copies of a reordered work list are not)
};

// This call's lists; the storage is the context's, reused tick after tick.
struct TickLists {
  Packer pk;
  std::vector<uint64_t> node_patch;   // {node, node_rec[8], node_free[3]} of the changed nodes
  std::vector<uint64_t> pod_patch;    // {pod, pod_rec[4], pod_rec[5]} of every pod re-pointed since the last K0 run
  std::vector<int32_t> k0_cols, k0_rows;  // incremental K0: the word columns and T rows to rewrite
  std::vector<ArenaCopy> copies;      // at most kAtomRowCopies row copies and a handful of sections
};

// The environment switches the decisions read (sr_ctx).
struct ResidencySwitches {
  int32_t k0_skip = 1, k0_incremental = 1, node_patch = 1, list_cost = 1, k2_mode = 0;
};

// The decisions of one tick: observe() fills the layout and what the slot's
// history allows, resolve() the rest once the allocations are known.
struct TickPlan {
  ArenaLayout at;
  bool reorder_due = false;    // the work list is to be reordered by cost before resolve()
  bool k0_skip_ok = false;     // the history allows a K0-less run
  bool k0_inc = false;         // K0 rewrites only k0_cols / k0_rows
  bool nodes_resident = false; // the device node section is current
  bool nodes_patch = false;    // ... or a few nodes behind: K0 applies their records from this call's copy
  bool cand_resident = false;  // the device candidate section is this candidate generation's
  bool skip = false;           // no K0 this run
  bool list_moved = false;     // the work list was reordered for this call
  int32_t n_node_patch = 0;    // node patches the kernels get (K0 writes them; K0-less: K2 reads them)
  int32_t n_pod_patch = 0;     // pod patches K0 gets
  int32_t n_dirty = 0;         // K0-less: the changed nodes in the kernel arguments
  int32_t dirty_node[kSkipDirty];
  int64_t dirty_free[kSkipDirty][3];
  uint64_t bytes_uploaded = 0; // the counted copies
};

// The bookkeeping of one workload slot.
struct Residency {
  uint64_t dev_state_gen = ~0ull;   // encoder state whose node records the device arena holds
  uint64_t host_state_gen = ~0ull;  // ... and the pinned staging arena
  uint64_t dev_cand_gen = ~0ull;    // candidate generation (Workload::cand_gen) the device arena holds (its
                                    //   pod records as of the last K0 run plus none of the pending patches)
  uint64_t host_cand_gen = ~0ull;   // ... and the staging arena (every patch applied)
  uint64_t tables_cand_gen = ~0ull; // candidate generation, encoder state, thresholds and atoms of the last K0
  uint64_t tables_state_gen = ~0ull;  //   run on the tables (incremental K0 / K0-less runs: what changed since)
  std::vector<int64_t> tables_thr;
  uint64_t tables_atoms_ver = ~0ull;   // Workload::atoms_ver of the last K0 run
  std::vector<int32_t> atom_cols;      // inter-pod / spread atom words changed since (reuse encodes)
  // atom rows changed since version atoms_log_ver (reuse encodes of one
  // candidate generation): the staging and device copies of an older version
  // that is atoms_log_ver take only those rows
  uint64_t atoms_log_ver = ~0ull, last_atoms_ver = ~0ull;
  std::vector<int32_t> atoms_log;
  uint64_t host_atoms_ver = ~0ull, dev_atoms_ver = ~0ull;
  // the work list by cost (sr_ctx::list_cost): the candidate generation whose
  // K2 durations were copied back (h_cycles, complete at ev_cost), and the one
  // the list was reordered for
  uint64_t cost_gen = ~0ull, list_sorted_gen = ~0ull;
  // spot nodes changed since tables_state_gen (valid: every state step since was one the encoder patched)
  std::vector<int32_t> dirty;
  bool dirty_valid = false;
  uint64_t seen_gen = ~0ull;        // encoder state at the slot's last prepare
  std::vector<int32_t> pending;     // pods re-pointed since the last K0 run (their device records are older)
  std::vector<uint8_t> pending_mark;
  bool class_flip = false;          // ... some of them to or from the empty class
  // what the next K0 launch of this slot brings the tables and the node section to (k0_queued commits it)
  bool commit_k0 = false;
  bool need_k0 = true;              // the device records name rows no K0 run has written yet

  // The encode failed: the encoder may have moved on, upload the node records again.
  void encode_failed() { dev_state_gen = ~0ull; }

  // A new allocation holds nothing.  resolve() takes the same three flags; the
  // planner calls this itself only when it gives up between the allocations.
  void moved(bool staging, bool arena, bool tables);

  // Phase one, observe and size: folds the encoded workload into the atoms
  // log, atom_cols, the dirty list and the pending pods, builds this call's
  // lists and lays the arena out.
  void observe(const Workload& w, const EncoderCache& E, const ResidencySwitches& sw, TickLists* tl, TickPlan* p);

  // Phase two, resolve: what is resident, which K0 runs, which lists the
  // kernels get; brings `staging` (p->at.bytes long) up to date and lists the
  // copies to the device in tl->copies.
  void resolve(const Workload& w, const EncoderCache& E, const ResidencySwitches& sw, bool staging_moved,
               bool arena_moved, bool tables_moved, bool list_moved, char* staging, TickLists* tl, TickPlan* p);

  // The copies of resolve() are queued.
  void upload_queued(const Workload& w, const TickPlan& p);

  // A K0 launch of the prepared workload is queued: it wrote the node and pod
  // patches and brought the rows to this workload (a rerun: idempotent).
  void k0_queued(const Workload& w);

  // The work list by cost: the first run of a candidate generation records its
  // K2 durations, a later prepare reorders the list by them.
  bool list_by_cost(const Workload& w) const { return list_sorted_gen == w.cand_gen; }
  bool want_cost(const Workload& w) const { return list_sorted_gen != w.cand_gen && cost_gen != w.cand_gen; }
  void cost_queued(const Workload& w) { cost_gen = w.cand_gen; }

 private:
  const std::vector<int32_t>* log_rows(uint64_t have) const {  // the rows a copy of version `have` lacks (null: all)
    return atoms_log_ver != ~0ull && have == atoms_log_ver ? &atoms_log : nullptr;
  }
  void clear_pending();
};

}  // namespace sr
