// evacuate.hpp — what a spot reclaim strands (sr_evacuate_plan), host side.
//
// HIP-free.  Scenario s loses a set of spot positions and moves a list of pods; its answer is
// sr_blockers_plan's loop over those pods against S', the snapshot built without the lost positions
// (sr_planner.h).  No S' is built.  A scenario is JUDGED when the standing snapshot provably says about every
// surviving node what S' says and its pods meet each other through nothing but arithmetic:
// evacuate_ways decides that from the sr_cluster tables and the snapshot alone.  Such a scenario is planned
// against the encode of the standing snapshot with the lost positions masked out as targets; its own
// placements are dense per-node deltas (used[3][n_pad], added[n_pad]) that the scenario restores to zero by
// walking its own node_of_pod, so the pod count has no limit.  evacuate_scenario is that loop on the host, the
// statement the kernel of evacuate.hip follows, a block of waves a scenario.  EvacuateStage lays out, packs
// and unpacks the two buffers of a pass, which query.cpp owns (GroupStage of blockers.hpp with the lost lists).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "blockers.hpp"

struct sr_snapshot;

namespace sr {

// The launch shape: waves a block (any number from 1 to kEvacMaxWaves) and blocks (1 to kEvacMaxGrid: the
// scratch grows by 28 bytes a node with every block, and 2,048 blocks of the default shape are all a device of
// 256 compute units can hold at once).  The defaults and their reason: DESIGN.md 4.1.
constexpr int kEvacWaves = 4, kEvacMaxWaves = 16;
constexpr int kEvacGrid = 512, kEvacMaxGrid = 2048;
// The lost set is a bitmask of Wp words in the block's LDS: the row words a pass may have.
constexpr int kEvacMaxWp = 4096;

// Checks the arguments (SR_ERR_INVALID_ARG: a CSR that decreases or starts below 0, a lost position outside
// [0, n_spot) or repeated within a scenario, a pod index out of range) and decides every scenario: how[s]
// SR_EVAC_JUDGED or SR_EVAC_NOT_PLAIN, `judged` ascending.  Nothing is modified.
struct EvacuateWays {
  std::vector<uint8_t> how;
  std::vector<int32_t> judged;
};
sr_status evacuate_ways(const sr_snapshot* snap, const sr_cluster* c, const sr_candidates* scen, const int32_t* lost_off,
                        const int32_t* lost_pos, EvacuateWays* out);

// The pods of the scenarios `ids`, flattened in that order: what a pass encodes as single-pod candidates.
void evacuate_flat(const sr_candidates* scen, const std::vector<int32_t>& ids, std::vector<int32_t>* pods);

// The dense context of one scenario at a time: zero between scenarios.
struct EvacuateDeltas {
  std::vector<int64_t> used;   // [3][n_pad]
  std::vector<int32_t> added;  // [n_pad]
  void size(int32_t n_pad) {
    used.assign(3 * static_cast<size_t>(n_pad), 0);
    added.assign(static_cast<size_t>(n_pad), 0);
  }
};

// The loop for one JUDGED scenario: blockers_candidate with a lost set (`lost`: Wp words, bit = position) and
// the dense deltas in place of the sorted list.  A lost or padded node is never a target and is counted in no
// row.  `d` is all zero on entry and on return (restored by walking node_of_pod).  node_of_pod [n]; counts
// [n][SR_WHY_COUNT] or nullptr: a stranded pod's row is written, every other row left as it is.  Returns the
// stranded pods, *first the first one's index (-1: none).
int32_t evacuate_scenario(const ExplainPrograms& x, const BlockerPod* pods, int32_t n, const uint64_t* atoms, int32_t Wp,
                          const int64_t* node_free, int32_t n_pad, int32_t n_spot, const int32_t* slack,
                          const uint64_t* lost, EvacuateDeltas* d, int32_t* node_of_pod, int32_t* counts, int32_t* first);

// What k_evacuate takes (by value).  x.pods, x.sums, x.node_mask and x.pod0 are not used.
struct EvacuateArgs {
  ExplainArgs x;
  const BlockerPod* pods;    // [x.n_pods] scenario after scenario
  const int32_t* scen_off;   // [n_scen + 1] into pods
  const int32_t* lost_off;   // [n_scen + 1] into lost_pos
  const int32_t* lost_pos;   // positions in [0, x.n_spot), distinct within a scenario
  const int64_t* node_left;  // [n_pad] allowed pods - pods (node_left), pads 0
  int32_t n_scen;
  int32_t waves;             // waves a block of this launch
  int64_t* used;             // scratch [blocks][3][n_pad], zero before the launch and after it
  int32_t* added;            // scratch [blocks][n_pad], likewise
  int32_t* counts;           // [x.n_pods][SR_WHY_COUNT], zeroed on the stream before the launch; nullptr: not wanted
  int32_t* node_of_pod;      // [x.n_pods]
  int32_t* stranded;         // [n_scen]
  int32_t* first;            // [n_scen]
};

// A pass's input: the common parts, scen_off, lost_off, lost_pos, node_left
enum EvacuateIn { EIN_SOFF = GIN_OFF, EIN_LOFF, EIN_LPOS, EIN_LEFT, EIN_PARTS };
using EvacuateLayout = GroupLayout;

// The scratch of a launch of `blocks` blocks: used at 0, added behind it.
struct EvacuateScratch {
  size_t used = 0, added = 0, bytes = 0;
};
EvacuateScratch evacuate_scratch(int32_t n_pad, int32_t blocks);

// The launch shape of a pass over n_scen scenarios: the defaults, or what SR_EVAC_GRID / SR_EVAC_WAVES ask
// for (`grid_env`, `waves_env`: the variables' values, nullptr: unset), clamped to what the kernel takes.
void evacuate_shape(int32_t n_scen, const char* grid_env, const char* waves_env, int32_t* blocks, int32_t* waves);

// Every output of scenario s as "not judged": stranded / first -1, its pods -1, zero rows, how as given.
void evacuate_clear(const sr_candidates* scen, int32_t s, uint8_t how, sr_evacuate_out* out);

// The staging of one pass.  Valid while the workload, node_free and the arguments given to plan() stand.
class EvacuateStage : public GroupStage {
 public:
  // `w`: the encode (tags on) of evacuate_flat(ids)'s pods as single-pod candidates.  A scenario one of whose
  // pods that encode handed back as fallback (or left inactive) is not planned: it is appended to *fell.
  // SR_ERR_STATE with *err set when the workload holds something the kernel would index out of bounds with.
  sr_status plan(const Workload& w, const std::vector<int64_t>& node_free, const sr_snapshot* snap, const sr_cluster* c,
                 const sr_candidates* scen, const int32_t* lost_off, const int32_t* lost_pos,
                 const std::vector<int32_t>& ids, bool want_counts, std::vector<int32_t>* fell, std::string* err);
  int32_t n_scen() const { return n_groups(); }  // scenarios the kernel plans
  int32_t n_pad() const;
  // `scratch`: evacuate_scratch(n_pad(), blocks) bytes, zero
  void args(const char* in, char* out, char* scratch, int32_t blocks, int32_t waves, EvacuateArgs* a) const;
  // the first at().out_bytes of the output buffer into the caller's arrays; how[s] becomes SR_EVAC_JUDGED
  void unpack(const char* image, const sr_candidates* scen, sr_evacuate_out* out) const;

 private:
  std::vector<int32_t> loff_, lpos_;  // the kept scenarios' lost lists
};

}  // namespace sr
