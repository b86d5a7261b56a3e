// node_view.cpp — rows between their column-major device layout and the caller's arrays (node_view.hpp).
#include "node_view.hpp"

#include <algorithm>

namespace sr {

NodeViewRow node_view_load(const uint64_t* min, const int32_t* cnt, const int32_t* at, size_t stride, size_t node) {
  NodeViewRow r;
  r.admits = cnt[kNodeViewAdmits * stride + node];
  r.near = cnt[kNodeViewNear * stride + node];
  for (size_t k = 0; k < SR_WHY_COUNT; ++k) {
    r.refuses[k] = cnt[(kNodeViewRefuses + k) * stride + node];
    r.sole[k] = cnt[(kNodeViewSole + k) * stride + node];
  }
  for (size_t d = 0; d < SR_SHORT_COUNT; ++d) {
    r.min[d] = min[d * stride + node];
    r.at[d] = at[d * stride + node];
  }
  return r;
}

void node_view_store(const NodeViewRow& r, uint64_t* min, int32_t* cnt, int32_t* at, size_t stride, size_t node) {
  cnt[kNodeViewAdmits * stride + node] = r.admits;
  cnt[kNodeViewNear * stride + node] = r.near;
  for (size_t k = 0; k < SR_WHY_COUNT; ++k) {
    cnt[(kNodeViewRefuses + k) * stride + node] = r.refuses[k];
    cnt[(kNodeViewSole + k) * stride + node] = r.sole[k];
  }
  for (size_t d = 0; d < SR_SHORT_COUNT; ++d) {
    min[d * stride + node] = r.min[d];
    at[d * stride + node] = r.at[d];
  }
}

void node_view_clear(sr_node_view_out* out, size_t ns) {
  *out->judged = 0;
  std::fill_n(out->admits, ns, 0);
  std::fill_n(out->near, ns, 0);
  std::fill_n(out->refuses, ns * SR_WHY_COUNT, 0);
  std::fill_n(out->sole, ns * SR_WHY_COUNT, 0);
  std::fill_n(out->sole_min, ns * SR_SHORT_COUNT, int64_t(0));
  std::fill_n(out->sole_at, ns * SR_SHORT_COUNT, -1);
}

void node_view_unpack(const char* image, size_t stride, size_t ns, sr_node_view_out* out) {
  const NodeViewLayout l = node_view_layout(stride, 1);
  const uint64_t* min = reinterpret_cast<const uint64_t*>(image + l.min);
  const int32_t* cnt = reinterpret_cast<const int32_t*>(image + l.cnt);
  const int32_t* at = reinterpret_cast<const int32_t*>(image + l.at);
  for (size_t node = 0; node < ns; ++node) {
    const NodeViewRow r = node_view_load(min, cnt, at, stride, node);
    out->admits[node] = r.admits;
    out->near[node] = r.near;
    std::copy_n(r.refuses, SR_WHY_COUNT, out->refuses + node * SR_WHY_COUNT);
    std::copy_n(r.sole, SR_WHY_COUNT, out->sole + node * SR_WHY_COUNT);
    for (size_t d = 0; d < SR_SHORT_COUNT; ++d) {
      out->sole_min[node * SR_SHORT_COUNT + d] = r.at[d] ? static_cast<int64_t>(r.min[d]) : 0;
      out->sole_at[node * SR_SHORT_COUNT + d] = r.at[d] - 1;
    }
  }
}

}  // namespace sr
