// node_view.hpp — what each spot node refuses (sr_node_view_pods, sr_node_view_plan), host side.
//
// HIP-free.  The explain / shortfall kernels reduce a query's masks over the nodes; these calls reduce along the
// other axis, a node's masks over the queries.  node_view_fold is one query folded into one node's row and
// node_view_merge two rows into one: the statements the kernels of node_view.hip follow.  The unit also says
// where a row's values lie on the device (NodeViewLayout) and how many chunks of queries a launch is cut into
// (node_view_chunks); tools/node_view_check.cpp follows the kernels on the host through both.
#pragma once

#include <cstddef>
#include <cstdint>

#include "explain_args.hpp"

namespace sr {

// One node's row.  at[d] is the slot + 1 of the query attaining min[d], 0: none (min[d] then means nothing), so
// a zeroed row is the row of no query.
struct NodeViewRow {
  int32_t admits = 0, near = 0;
  int32_t refuses[SR_WHY_COUNT] = {}, sole[SR_WHY_COUNT] = {};
  uint64_t min[SR_SHORT_COUNT] = {};
  int32_t at[SR_SHORT_COUNT] = {};
};

// The bit of dimension d (SR_SHORT_*) and the four together (R of sr_planner.h).
constexpr uint32_t node_view_bit(int d) { return d < 3 ? 1u << (WHY_CPU + d) : 1u << WHY_PODS; }
constexpr uint32_t kNodeViewR = 1u << WHY_PODS | 1u << WHY_CPU | 1u << WHY_MEMORY | 1u << WHY_EPHEMERAL;

// (shortfall a, slot + 1 a) before (shortfall b, slot + 1 b); "none" (at 0) is after everything
inline bool node_view_before(uint64_t min_a, int32_t at_a, uint64_t min_b, int32_t at_b) {
  return at_a != 0 && (at_b == 0 || min_a < min_b || (min_a == min_b && at_a < at_b));
}

// One judged query into a node's row: `mask` is explain_node_ctx's, `sf` shortfall_node's, `slot` the query's.
inline void node_view_fold(uint32_t mask, const int64_t sf[SR_SHORT_COUNT], int32_t slot, NodeViewRow* row) {
  row->admits += mask == 0;
  row->near += mask != 0 && (mask & ~kNodeViewR) == 0;
  for (int r = 0; r < SR_WHY_COUNT; ++r) {
    row->refuses[r] += (mask >> r & 1) != 0;
    row->sole[r] += mask == 1u << r;
  }
  for (int d = 0; d < SR_SHORT_COUNT; ++d)
    if (mask == node_view_bit(d) && node_view_before(static_cast<uint64_t>(sf[d]), slot + 1, row->min[d], row->at[d])) {
      row->min[d] = static_cast<uint64_t>(sf[d]);
      row->at[d] = slot + 1;
    }
}

// Two rows of disjoint sets of queries into one: sums, and the lexicographic minimum of (shortfall, slot).
inline void node_view_merge(NodeViewRow* into, const NodeViewRow& part) {
  into->admits += part.admits;
  into->near += part.near;
  for (int r = 0; r < SR_WHY_COUNT; ++r) {
    into->refuses[r] += part.refuses[r];
    into->sole[r] += part.sole[r];
  }
  for (int d = 0; d < SR_SHORT_COUNT; ++d)
    if (node_view_before(part.min[d], part.at[d], into->min[d], into->at[d])) {
      into->min[d] = part.min[d];
      into->at[d] = part.at[d];
    }
}

// Rows on the device: column-major, [cols][stride] per value so that the 64 lanes of a wave (64 consecutive
// nodes) store 64 consecutive words of a column.  A block of `chunks` row sets lies as min [chunks][4][stride]
// (uint64), then cnt [chunks][kNodeViewCnt][stride], then at [chunks][4][stride] (int32).
constexpr int kNodeViewAdmits = 0, kNodeViewNear = 1, kNodeViewRefuses = 2, kNodeViewSole = 2 + SR_WHY_COUNT;
constexpr int kNodeViewCnt = 2 + 2 * SR_WHY_COUNT;
constexpr size_t kNodeViewRowBytes = 8 * SR_SHORT_COUNT + 4 * kNodeViewCnt + 4 * SR_SHORT_COUNT;  // 152

struct NodeViewLayout {
  size_t min = 0, cnt = 0, at = 0, bytes = 0;  // offsets of the three arrays, and the end
};
inline NodeViewLayout node_view_layout(size_t stride, size_t chunks) {
  NodeViewLayout l;
  l.cnt = l.min + 8 * SR_SHORT_COUNT * stride * chunks;
  l.at = l.cnt + 4 * kNodeViewCnt * stride * chunks;
  l.bytes = l.at + 4 * SR_SHORT_COUNT * stride * chunks;
  return l;
}
// The stride of the call's totals: the spot nodes up to a whole row word (whatever the encode pads its rows to).
inline int32_t node_view_stride(int32_t n_spot) { return (n_spot + 63) & ~63; }

// How a launch over `n_queries` active queries and Wp row words is cut: a block takes four row words and a chunk
// of `per` consecutive queries, and leaves one partial row per node and chunk.  ceil(Wp / 4) blocks alone fill
// the device only on the largest pools, so the queries are cut until about kNodeViewBlocks blocks run (two a
// compute unit of a 256-unit device); a chunk is never empty.  The partials therefore hold at most
//   (kNodeViewBlocks + ceil(Wp / 4)) * 256 nodes * kNodeViewRowBytes  <  20 MiB + 152 B * n_pad
// whatever the number of queries.  `override_per` > 0 (SR_NODE_VIEW_CHUNK) sets the queries a chunk instead;
// it is raised where the grid's second dimension (65,535) would not hold the chunks.
constexpr int32_t kNodeViewBlocks = 512, kNodeViewMaxChunks = 65535;
struct NodeViewChunks {
  int32_t per = 1, chunks = 0;
};
inline NodeViewChunks node_view_chunks(int32_t Wp, int32_t n_queries, int32_t override_per = 0) {
  NodeViewChunks c;
  if (n_queries <= 0) return c;
  if (override_per > 0) {
    c.per = override_per;
  } else {
    const int32_t gx = shortfall_blocks(Wp) > 0 ? shortfall_blocks(Wp) : 1;
    int32_t want = (kNodeViewBlocks + gx - 1) / gx;  // chunks * gx <= kNodeViewBlocks + gx
    if (want > n_queries) want = n_queries;
    c.per = (n_queries + want - 1) / want;
  }
  const int32_t least = (n_queries + kNodeViewMaxChunks - 1) / kNodeViewMaxChunks;
  if (c.per < least) c.per = least;
  c.chunks = (n_queries + c.per - 1) / c.per;
  return c;
}

// What the kernels of node_view.hip take beside ExplainPlanArgs (whose per-query outputs they do not write).
struct NodeViewArgs {
  const int64_t* node_left;  // [n_pad] as ShortfallArgs::node_left
  const int32_t* slot;       // [n_pods] the slot of active query q
  int32_t per, chunks;       // node_view_chunks
  int32_t lists;             // 1: the queries carry context lists (sr_node_view_plan's batched pass)
  int32_t tot_stride;        // node_view_stride(n_spot)
  uint64_t* part_min;        // the partials: node_view_layout(n_pad, chunks); rows of nodes >= n_spot are not written
  int32_t* part_cnt;
  int32_t* part_at;
  uint64_t* tot_min;         // the call's totals: node_view_layout(tot_stride, 1), zeroed once a call; k_node_view_close
  int32_t* tot_cnt;          //   merges a launch's partials into them
  int32_t* tot_at;
};

// One column-major row set <-> a row (host side: the check tool and the unpacking).
NodeViewRow node_view_load(const uint64_t* min, const int32_t* cnt, const int32_t* at, size_t stride, size_t node);
void node_view_store(const NodeViewRow& row, uint64_t* min, int32_t* cnt, int32_t* at, size_t stride, size_t node);

// The caller's arrays with no judged query in them (fallback is the call's to fill).
void node_view_clear(sr_node_view_out* out, size_t n_spot);
// The downloaded totals (node_view_layout(stride, 1) at `image`) into the caller's arrays.
void node_view_unpack(const char* image, size_t stride, size_t n_spot, sr_node_view_out* out);

}  // namespace sr
