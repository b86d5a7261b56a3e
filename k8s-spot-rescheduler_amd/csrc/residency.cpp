// residency.cpp — the slot bookkeeping behind a tick's upload and K0 decisions
// (residency.hpp; DESIGN.md §5 lists the copies and the fields tracking them).
#include "residency.hpp"

#include <algorithm>

namespace sr {

void Residency::moved(bool staging, bool arena, bool tables) {
  if (staging) host_state_gen = host_cand_gen = host_atoms_ver = ~0ull;  // holds none
  if (arena) dev_atoms_ver = ~0ull;  // (resolve() takes the node and candidate sections as gone too)
  if (tables) tables_cand_gen = ~0ull;  // a new allocation holds no rows
}

void Residency::clear_pending() {
  pending.clear();
  std::fill(pending_mark.begin(), pending_mark.end(), 0);
  class_flip = false;
}

void Residency::observe(const Workload& w, const EncoderCache& E, const ResidencySwitches& sw, TickLists* tl,
                        TickPlan* p) {
  *p = TickPlan{};
  ArenaLayout& at = p->at;
  Packer& pk = tl->pk;
  pk.clear();
  const int32_t na = static_cast<int32_t>(w.pod_src.size());
  const int32_t ncand = static_cast<int32_t>(w.cand_global.size());
  at.node_rec = pk.add(E.node_rec);
  at.node_free = pk.add(E.node_free);
  at.node_bytes = pk.size();
  at.cls_prog_off = pk.add(w.cls_prog_off), at.cls_prog = pk.add(w.cls_prog), at.cls_prog8 = pk.add(w.cls_prog8);
  at.pod_rec = pk.add(w.pod_rec);
  at.cand_off = pk.add(w.cand_off), at.cand_global = pk.add(w.cand_global);
  at.list = pk.add(w.list);
  const bool dyn = at.dyn = !w.dyn_cand.empty();
  if (dyn) at.dyn_cand = pk.add(w.dyn_cand), at.dyn_pod = pk.add(w.dyn_pod), at.ds_info = pk.add(w.ds_info);
  const bool ext = at.ext = !w.ext_cand.empty();
  if (ext) at.ext_cand = pk.add(w.ext_cand), at.pod_ext = pk.add(w.pod_ext), at.list_ext = pk.add(w.list_ext);
  at.atoms = pk.add(w.atoms);
  at.tick_rest = pk.size();
  if (ext) at.node_scal = pk.add(w.node_scal);
  if (dyn) at.sp_tab = pk.add(w.sp_tab), at.dk_dom = pk.add(w.dk_dom);
  at.t_thr = pk.add(w.t_thr);
  // the atom-row log
  if (w.atoms_ver != last_atoms_ver) {
    const bool follows = w.reused && !w.atom_rows_all && w.atoms_prev_ver == last_atoms_ver;
    if (follows && atoms_log_ver != ~0ull) {
      atoms_log.insert(atoms_log.end(), w.atom_rows.begin(), w.atom_rows.end());
    } else if (follows) {
      atoms_log_ver = last_atoms_ver;
      atoms_log = w.atom_rows;
    } else {
      atoms_log_ver = ~0ull;
      atoms_log.clear();
    }
    if (atoms_log.size() > kAtomsLogMax) {
      atoms_log_ver = ~0ull;
      atoms_log.clear();
    }
    last_atoms_ver = w.atoms_ver;
  }
  const bool same_cand = w.reused && dev_cand_gen == w.cand_gen;  // a reuse encode of the generation on the device
  if (!same_cand) atom_cols.clear();
  else atom_cols.insert(atom_cols.end(), w.atom_cols.begin(), w.atom_cols.end());
  // ---- the slot's device state against this call.  Spot nodes changed since
  // the slot's tables were written, accumulated over K0-less runs:
  if (w.state_gen != seen_gen) {
    if (dirty_valid && E.patched_from != ~0ull && E.patched_from == seen_gen && E.state_gen == w.state_gen) {
      for (int32_t i : E.patched_nodes)
        if (std::find(dirty.begin(), dirty.end(), i) == dirty.end()) dirty.push_back(i);
    } else {
      dirty_valid = false;
    }
    seen_gen = w.state_gen;
  }
  if (dirty.size() > kDirtyMax) dirty_valid = false;
  // pods the encoder re-pointed since the last K0 run of this candidate generation
  if (!same_cand) {
    pending.clear();
    pending_mark.assign(static_cast<size_t>(na), 0);
    class_flip = false;
  } else {
    if (pending_mark.size() != static_cast<size_t>(na)) pending_mark.assign(static_cast<size_t>(na), 0);
    for (size_t i = 0; i < w.pod_patch.size(); i += kPodPatchWords) {
      const int32_t q = static_cast<int32_t>(w.pod_patch[i]);
      if (!pending_mark[q]) {
        pending_mark[q] = 1;
        pending.push_back(q);
      }
    }
    class_flip = class_flip || w.class_flip;
  }
  const bool tables_cur = same_cand && tables_cand_gen == w.cand_gen && tables_thr.size() == w.t_thr.size() && dirty_valid;
  // A K0-less run: the tables stand for every node but the changed ones, whose
  // records and T bits K2 takes from the node patches; the atoms (S rows) must
  // be the tables' and no pod may have left the empty class (K2's dead-pod
  // shortcut reads the device records).  Node-order candidates only (on
  // either kernel: the SR_K2_NODE_KERNEL switch does not matter here).
  p->k0_skip_ok = sw.k0_skip && ncand > 0 && tables_cur && dirty.size() <= kSkipDirty && !class_flip &&
                  k2_node_launch(dyn, sw.k2_mode, w.max_cand_pods, 1) && tables_atoms_ver == w.atoms_ver;
  // node patches {node, node_rec[8], node_free[3]}: the changed nodes' records
  // ride in the call's copy; K0 writes them into the node section (or K2 reads
  // them, K0-less)
  std::vector<uint64_t>& patch = tl->node_patch;
  patch.clear();
  if (dirty_valid && !dirty.empty() && dirty.size() <= kPatchNodes) {  // a superset of the nodes the device
                                                                       // section lacks
    const size_t NP = static_cast<size_t>(w.n_pad);
    for (int32_t i : dirty) {
      patch.push_back(static_cast<uint64_t>(i));
      for (size_t j = 0; j < 8; ++j) patch.push_back(E.node_rec[static_cast<size_t>(i) * 8 + j]);
      for (size_t dm = 0; dm < 3; ++dm) patch.push_back(static_cast<uint64_t>(E.node_free[dm * NP + i]));
    }
  }
  if (!patch.empty()) at.node_patch = pk.add(patch);
  // pod patches of a K0 run: every pod re-pointed since the last one
  std::vector<uint64_t>& ppatch = tl->pod_patch;
  ppatch.clear();
  if (same_cand)  // (unused if the run turns out K0-less)
    for (int32_t q : pending)
      ppatch.insert(ppatch.end(), {static_cast<uint64_t>(q), w.pod_rec[static_cast<size_t>(q) * 6 + 4],
                                   w.pod_rec[static_cast<size_t>(q) * 6 + 5]});
  if (!ppatch.empty()) at.pod_patch = pk.add(ppatch);
  // Incremental K0: the tables hold this candidate generation: the word
  // columns of the changed nodes and the T rows whose threshold moved are
  // rewritten; anything else rewrites every row.
  std::vector<int32_t>& kcols = tl->k0_cols;
  std::vector<int32_t>& krows = tl->k0_rows;
  kcols.clear();
  krows.clear();
  p->k0_inc = sw.k0_incremental && tables_cur;  // (unused if the run turns out K0-less)
  if (p->k0_inc) {
    for (int32_t i : dirty) kcols.push_back(i >> 6);
    kcols.insert(kcols.end(), atom_cols.begin(), atom_cols.end());
    std::sort(kcols.begin(), kcols.end());
    kcols.erase(std::unique(kcols.begin(), kcols.end()), kcols.end());
    for (size_t r = 0; r < w.t_thr.size(); ++r)
      if (w.t_thr[r] != tables_thr[r] && w.t_thr[r] != kTSpare) krows.push_back(static_cast<int32_t>(r));
    if (kcols.size() > kK0ColsMax || krows.size() > kK0RowsMax) p->k0_inc = false;
  }
  if (!p->k0_inc) kcols.clear(), krows.clear();
  if (!kcols.empty()) at.k0_cols = pk.add(kcols);
  if (!krows.empty()) at.k0_rows = pk.add(krows);
  at.bytes = pk.size();
  // a reused workload's list in the order of its last run's K2 durations
  // (list_sorted_gen is set once the reordered list's copies are queued: a
  // prepare failing in between reorders and uploads it again next time)
  p->reorder_due = sw.list_cost && w.reused && cost_gen == w.cand_gen && list_sorted_gen != w.cand_gen;
}

void Residency::resolve(const Workload& w, const EncoderCache& E, const ResidencySwitches& sw, bool staging_moved,
                        bool arena_moved, bool tables_moved, bool list_moved, char* hs, TickLists* tl, TickPlan* p) {
  const ArenaLayout& at = p->at;
  moved(staging_moved, arena_moved, tables_moved);
  p->list_moved = list_moved;
  p->nodes_resident = !arena_moved && dev_state_gen == w.state_gen;
  // a reuse encode's candidate section is on the device: K0 re-points the
  // records that moved (a K0-less run reads them as they are)
  p->cand_resident = w.reused && !arena_moved && dev_cand_gen == w.cand_gen;
  p->skip = p->k0_skip_ok && p->cand_resident && !need_k0 && !tables_moved;
  // a few nodes changed since the generation on the device: K0 applies their
  // records from this call's copy (K0-less: K2 reads them there)
  p->nodes_patch = !p->nodes_resident && !arena_moved && !tl->node_patch.empty() && sw.node_patch;
  if (tables_moved || p->skip) {  // every row / no row
    p->k0_inc = false;
    if (tables_moved) tl->k0_cols.clear(), tl->k0_rows.clear();
  }
  const size_t from = p->nodes_resident || p->nodes_patch ? at.node_bytes : 0;
  // The staging arena keeps the node section of the generation it last held:
  // when that is the current one, or the one the encoder patched a few nodes
  // on, only those nodes' records are rewritten (no copy of the whole section).
  const size_t NP = static_cast<size_t>(w.n_pad);
  if (host_state_gen == w.state_gen) {
    // current
  } else if (E.patched_from != ~0ull && host_state_gen == E.patched_from && E.state_gen == w.state_gen &&
             !E.patched_nodes.empty()) {
    for (int32_t i : E.patched_nodes) {
      std::memcpy(hs + at.node_rec + static_cast<size_t>(i) * 64, &E.node_rec[static_cast<size_t>(i) * 8], 64);
      for (size_t dm = 0; dm < 3; ++dm)
        std::memcpy(hs + at.node_free + (dm * NP + static_cast<size_t>(i)) * 8, &E.node_free[dm * NP + i], 8);
    }
  } else {
    std::memcpy(hs + at.node_rec, E.node_rec.data(), E.node_rec.size() * sizeof(uint64_t));
    std::memcpy(hs + at.node_free, E.node_free.data(), E.node_free.size() * sizeof(int64_t));
  }
  host_state_gen = w.state_gen;
  // the candidate section: kept in staging across a reuse encode (its pod
  // patches applied there too), packed again otherwise
  const size_t row_bytes = static_cast<size_t>(w.Wp) * sizeof(uint64_t);
  const size_t list_bytes = w.list.size() * sizeof(int32_t), list_ext_bytes = w.list_ext.size() * sizeof(int32_t);
  if (w.reused && host_cand_gen == w.cand_gen) {
    for (size_t i = 0; i < w.pod_patch.size(); i += kPodPatchWords)
      std::memcpy(hs + at.pod_rec + (static_cast<size_t>(w.pod_patch[i]) * 6 + 4) * 8, &w.pod_patch[i + 1], 16);
    if (host_atoms_ver != w.atoms_ver) {
      const std::vector<int32_t>* rows = log_rows(host_atoms_ver);
      if (rows) {
        for (int32_t r : *rows)
          std::memcpy(hs + at.atoms + static_cast<size_t>(r) * row_bytes, w.atoms.data() + static_cast<size_t>(r) * w.Wp,
                      row_bytes);
      } else {
        std::memcpy(hs + at.atoms, w.atoms.data(), w.atoms.size() * sizeof(uint64_t));
      }
    }
    if (list_moved) {
      std::memcpy(hs + at.list, w.list.data(), list_bytes);
      if (at.ext) std::memcpy(hs + at.list_ext, w.list_ext.data(), list_ext_bytes);
    }
    tl->pk.copy_to(hs, at.tick_rest);
  } else {
    tl->pk.copy_to(hs, at.node_bytes);
  }
  host_cand_gen = w.cand_gen;
  host_atoms_ver = w.atoms_ver;
  if (!p->cand_resident) {  // the records go up whole, current: nothing pending, but rows to write
    clear_pending();
    need_k0 = true;
  }
  // the copies to the device, in the order they are queued
  std::vector<ArenaCopy>& cp = tl->copies;
  cp.clear();
  if (!p->cand_resident) {
    cp.push_back({from, at.bytes - from, true});
  } else {
    if (from < at.node_bytes) cp.push_back({0, at.node_bytes, true});
    // the atoms: current, a few rows behind (each row alone), or whole
    if (dev_atoms_ver != w.atoms_ver) {
      const std::vector<int32_t>* rows = log_rows(dev_atoms_ver);
      if (rows && rows->size() <= kAtomRowCopies)
        for (int32_t r : *rows) cp.push_back({at.atoms + static_cast<size_t>(r) * row_bytes, row_bytes, true});
      else cp.push_back({at.atoms, at.tick_rest - at.atoms, true});
    }
    cp.push_back({at.tick_rest, at.bytes - at.tick_rest, true});
    if (list_moved) {  // the reordered work list into the resident candidate section
      cp.push_back({at.list, list_bytes, false});
      if (at.ext) cp.push_back({at.list_ext, list_ext_bytes, false});
    }
  }
  p->bytes_uploaded = 0;
  for (const ArenaCopy& c : cp) p->bytes_uploaded += c.counted ? c.bytes : 0;
  // K0 writes the patches into the node section; a K0-less run's K2 reads them
  // (every changed node, whether or not the section went up whole)
  const bool use_patch = p->skip ? !tl->node_patch.empty() : p->nodes_patch;
  p->n_node_patch = use_patch ? static_cast<int32_t>(tl->node_patch.size() / kNodePatchWords) : 0;
  const bool pods_patch = !p->skip && p->cand_resident && !tl->pod_patch.empty();
  p->n_pod_patch = pods_patch ? static_cast<int32_t>(tl->pod_patch.size() / kPodPatchWords) : 0;
  p->n_dirty = 0;
  if (p->skip)  // the changed nodes in the kernel arguments (<= kSkipDirty)
    for (int32_t i : dirty) {
      p->dirty_node[p->n_dirty] = i;
      for (size_t dm = 0; dm < 3; ++dm) p->dirty_free[p->n_dirty][dm] = E.node_free[dm * NP + static_cast<size_t>(i)];
      ++p->n_dirty;
    }
}

void Residency::upload_queued(const Workload& w, const TickPlan& p) {
  dev_atoms_ver = w.atoms_ver;
  if (host_atoms_ver == w.atoms_ver) {  // both copies current: the log starts again here
    atoms_log_ver = w.atoms_ver;
    atoms_log.clear();
  }
  if (!p.nodes_patch) dev_state_gen = w.state_gen;  // the section went up whole (or was current)
  dev_cand_gen = w.cand_gen;
  if (p.list_moved) list_sorted_gen = w.cand_gen;
  commit_k0 = !p.skip;
}

void Residency::k0_queued(const Workload& w) {
  if (!commit_k0) return;
  commit_k0 = false;
  tables_cand_gen = w.cand_gen;
  tables_state_gen = dev_state_gen = w.state_gen;
  if (tables_thr != w.t_thr) tables_thr = w.t_thr;
  tables_atoms_ver = w.atoms_ver;
  atom_cols.clear();
  dirty.clear();
  dirty_valid = true;
  seen_gen = w.state_gen;
  for (int32_t q : pending) pending_mark[q] = 0;
  pending.clear();
  class_flip = false;
  need_k0 = false;
}

}  // namespace sr
