// explain.hpp — which scheduler filter refuses a pod on a node (sr_explain_pods), host side.
//
// HIP-free.  The encoder folds every filter into one S row and three T rows
// per pod, which is what the planning kernels want and what
// loses the reason.  With EncoderCache::want_why set it also tags what it
// emits: a reason per atom row (Workload::atom_why), a reason per class
// program operation (Workload::cls_why), the taint atoms behind every
// composite atom and each pod's class before the dead check.  build_explain
// turns those into one explain program per class, whose operations keep the
// filters apart; explain_node evaluates a program for one node on the host
// (tools/explain_check.cpp), the kernel of explain.hip for 64 nodes a wave.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/sr_planner.h"

namespace sr {

struct Workload;

// Reason indices: bit r of a node's mask is SR_WHY_* 1 << r.
enum Why : uint8_t {
  WHY_UNSCHEDULABLE = 0,
  WHY_TAINT = 1,
  WHY_NODE_AFFINITY = 2,
  WHY_PODS = 3,
  WHY_CPU = 4,
  WHY_MEMORY = 5,
  WHY_EPHEMERAL = 6,
  WHY_SCALAR = 7,
  WHY_PORTS = 8,
  WHY_INTER_POD = 9,
  WHY_SPREAD = 10,
  WHY_VOLUMES = 11,
  // tags of the encoder that are no reason of their own:
  WHY_NONE = 0x40,       // a row no class program names (domain-path rows)
  WHY_COMPOSITE = 0x41,  // pod count AND NOT an untolerated-taint set: expanded (Workload::comp_taint_off)
  WHY_DECIDED = 0x80     // | set of WHY_DEC_*: the `atom 0 AND NOT atom 0` of a class decided without rows
};
enum : uint8_t { WHY_DEC_NODE_AFFINITY = 1, WHY_DEC_VOLUMES = 2, WHY_DEC_INTER_POD = 4 };
static_assert(SR_WHY_COUNT == 12 && (1u << WHY_VOLUMES) == SR_WHY_VOLUMES && (1u << WHY_PODS) == SR_WHY_PODS &&
                  (1u << WHY_CPU) == SR_WHY_CPU && (1u << WHY_INTER_POD) == SR_WHY_INTER_POD,
              "reason indices follow sr_planner.h");

// Explain program operations: atom << 8 | reason << 3 | kind.
enum : int32_t {
  X_AND = 0,         // the node refuses for `reason` unless its bit is set in the atom row
  X_ANDNOT = 1,      // ... if its bit is set
  X_TERM_START = 2,  // opens an ORed term (closes the one before): the group refuses when no term holds
  X_TERM_AND = 3,    // ANDs into the open term
  X_ALL = 4          // every node refuses for `reason` (decided by the encoder without rows)
};
inline int32_t x_op(int32_t atom, int32_t why, int32_t kind) { return atom << 8 | why << 3 | kind; }
constexpr int32_t kMaxExplainAtoms = 1 << 23;

struct ExplainPrograms {
  std::vector<int32_t> off;  // [n_classes + 1]
  std::vector<int32_t> ops;
};

// One program per class of `w` (encoded with want_why).  False: the workload
// carries no tags, or names more atoms than an operation can hold.
bool build_explain(const Workload& w, ExplainPrograms* out);

// The queried pod of active pod q: {class before the dead check, 1: NodeResourcesFit compares cpu / memory /
// ephemeral (0: the all-zero shortcut), requests}
struct ExplainPod {
  int32_t cls;
  int32_t resources;
  int64_t req[3];
};
void explain_pods(const Workload& w, std::vector<ExplainPod>* out);

// The mask of one node: the program over the atom rows, then fitsRequest's
// compares of the requests against the node's free values (free = allocatable
// - requested, so request > free is allocatable < request + requested).
uint32_t explain_node(const ExplainPrograms& x, const ExplainPod& p, const uint64_t* atoms, int32_t Wp,
                      const int64_t* node_free, int32_t n_pad, int32_t node);

}  // namespace sr
