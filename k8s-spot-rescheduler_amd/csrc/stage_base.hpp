// stage_base.hpp — what the staging units of the query calls share (explain_stage.hpp, blockers.hpp,
// evacuate.hpp): a buffer as a table of parts, the check of the encoded explain workload every plan() starts
// with, and the kernel arguments every query kernel takes first.
//
// HIP-free.  The non-template functions are defined in explain_stage.cpp.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "explain_args.hpp"

namespace sr {

struct Workload;

// A part of a staged buffer.  A part starts at the 8-byte boundary after the part before it; an absent part has
// no bytes.
struct StagePart {
  size_t off = 0, bytes = 0;
  size_t elem = 8;  // size of the part's element type (what its offset must be a multiple of)
};

// Every input buffer starts with these, in this order; a unit's own parts follow from IN_COMMON on.
enum StageCommonIn {
  IN_ATOMS,  // uint64 [n_atoms][Wp]
  IN_FREE,   // int64 [3][n_pad]
  IN_XOFF,   // int32 [n_classes + 1]
  IN_XOPS,   // int32
  IN_PODS,   // the unit's pod records [n_pods]
  IN_COMMON
};

inline size_t up8(size_t b) { return (b + 7) & ~size_t(7); }

// Offsets from the sizes: every part at the 8-byte boundary after the one before.  Returns the last part's end.
inline size_t place(StagePart* parts, int n) {
  size_t end = 0;
  for (int i = 0; i < n; ++i) {
    parts[i].off = up8(end);
    end = parts[i].off + parts[i].bytes;
  }
  return end;
}

template <class T>
void part_of(StagePart* p, const void** src, const T* data, size_t count) {
  p->bytes = count * sizeof(T);
  p->elem = sizeof(T) > 8 ? 8 : sizeof(T);  // (the records are 8-byte aligned structs)
  if (src) *src = data;
}

template <class T>
T* at_part(char* base, const StagePart& p) {
  return reinterpret_cast<T*>(base + p.off);
}
template <class T>
const T* at_part(const char* base, const StagePart& p) {
  return reinterpret_cast<const T*>(base + p.off);
}

// The input image: every part with bytes copied from its source.
void pack_parts(char* in, const StagePart* parts, const void* const* src, int n);

// What every plan() starts with: the explain programs of the encoded workload `w` into *prog, and everything
// the kernels index with checked (`node_free`: EncoderCache::node_free of its encode).  `more_ok`: further size
// conditions of the caller's, reported as the same defect.  SR_ERR_STATE with *err = "<who>: ..." otherwise.
// Sets the parts IN_ATOMS .. IN_XOPS of `in` and their sources.
sr_status stage_workload(const char* who, const Workload& w, const std::vector<int64_t>& node_free, bool more_ok,
                         ExplainPrograms* prog, StagePart* in, const void** src, std::string* err);

// The arguments every query kernel takes first, over the input buffer `in` laid out as `parts`: n_spot, n_pad,
// Wp, n_pods, atoms, node_free, xoff, xops.  The rest of *a is left as it is.
void stage_args(const Workload& w, int32_t n_pods, const char* in, const StagePart* parts, ExplainArgs* a);

}  // namespace sr
