// explain_stage.cpp — layout, packing and unpacking of an explain / shortfall call's buffers.
#include "explain_stage.hpp"

#include <algorithm>
#include <cstring>

#include "host.hpp"

namespace sr {

void active_lists(const Workload& w, const PlanQueries& pq, std::vector<PlanCtxEntry>* entries,
                  std::vector<int32_t>* off) {
  off->assign(1, 0);
  entries->clear();
  for (int32_t src : w.pod_src) {
    const int32_t i = src - w.pod_base;
    const auto e0 = pq.entries.begin();
    entries->insert(entries->end(), e0 + pq.off[i], e0 + pq.off[i + 1]);
    off->push_back(static_cast<int32_t>(entries->size()));
  }
}

void clear_slot(sr_explain_out* out, sr_shortfall_out* sh, size_t o, size_t ns, uint8_t fallback) {
  out->feasible[o] = out->first[o] = -1;
  std::fill_n(out->counts + o * SR_WHY_COUNT, SR_WHY_COUNT, 0);
  if (out->node_mask) std::fill_n(out->node_mask + o * ns, ns, uint16_t(0));
  if (out->fallback) out->fallback[o] = fallback;
  if (!sh) return;
  sh->near[o] = -1;
  std::fill_n(sh->only_nodes + o * SR_SHORT_COUNT, SR_SHORT_COUNT, 0);
  std::fill_n(sh->only_min + o * SR_SHORT_COUNT, SR_SHORT_COUNT, int64_t(0));
  std::fill_n(sh->only_at + o * SR_SHORT_COUNT, SR_SHORT_COUNT, -1);
  if (sh->node_short) std::fill_n(sh->node_short + o * ns * SR_SHORT_COUNT, ns * SR_SHORT_COUNT, int64_t(0));
}

void pack_parts(char* in, const StagePart* parts, const void* const* src, int n) {
  for (int i = 0; i < n; ++i)
    if (parts[i].bytes) std::memcpy(in + parts[i].off, src[i], parts[i].bytes);
}

sr_status stage_workload(const char* who, const Workload& w, const std::vector<int64_t>& node_free, bool more_ok,
                         ExplainPrograms* prog, StagePart* in, const void** src, std::string* err) {
  const size_t n_pad = static_cast<size_t>(w.n_pad);
  if (!build_explain(w, prog) || w.pod_cls.size() != w.pod_src.size() || w.n_pad != w.Wp * 64 ||
      node_free.size() < 3 * n_pad || !more_ok) {
    *err = std::string(who) + ": the encoder left no reasons";
    return SR_ERR_STATE;
  }
  for (int32_t op : prog->ops)  // what the kernel indexes with
    if ((op >> 8) < 0 || (op >> 8) >= w.n_atoms || (op >> 3 & 31) >= SR_WHY_COUNT || (op & 7) > X_ALL) {
      *err = std::string(who) + ": malformed program";
      return SR_ERR_STATE;
    }
  part_of(&in[IN_ATOMS], &src[IN_ATOMS], w.atoms.data(), w.atoms.size());
  part_of(&in[IN_FREE], &src[IN_FREE], node_free.data(), 3 * n_pad);
  part_of(&in[IN_XOFF], &src[IN_XOFF], prog->off.data(), prog->off.size());
  part_of(&in[IN_XOPS], &src[IN_XOPS], prog->ops.data(), prog->ops.size());
  return SR_OK;
}

void stage_args(const Workload& w, int32_t n_pods, const char* in, const StagePart* parts, ExplainArgs* a) {
  a->n_spot = w.n_spot;
  a->n_pad = w.n_pad;
  a->Wp = w.Wp;
  a->n_pods = n_pods;
  a->atoms = at_part<uint64_t>(in, parts[IN_ATOMS]);
  a->node_free = at_part<int64_t>(in, parts[IN_FREE]);
  a->xoff = at_part<int32_t>(in, parts[IN_XOFF]);
  a->xops = at_part<int32_t>(in, parts[IN_XOPS]);
}

sr_status ExplainStage::plan(const Workload& w, const std::vector<int64_t>& node_free, const sr_snapshot* snap,
                             const PlanQueries* pq, bool want_shortfall, bool node_mask, bool node_short,
                             std::string* err, const NodeViewAsk* view) {
  if (view) {
    want_shortfall = true;
    node_mask = node_short = false;
  }
  const size_t na = w.pod_src.size(), ns = static_cast<size_t>(w.n_spot), n_pad = static_cast<size_t>(w.n_pad);
  at_ = StageLayout{};
  const sr_status st = stage_workload("explain", w, node_free, true, &prog_, at_.in, src_, err);
  if (st != SR_OK) return st;
  explain_pods(w, &pods_);
  for (const ExplainPod& p : pods_)
    if (p.cls < 0 || p.cls >= w.n_classes) {
      *err = "explain: pod class out of range";
      return SR_ERR_STATE;
    }
  if (pq) {
    active_lists(w, *pq, &centries_, &coff_);
    for (const PlanCtxEntry& e : centries_)  // what the kernel indexes with
      if (e.node < 0 || e.node >= w.n_spot) {
        *err = "explain: context node out of range";
        return SR_ERR_STATE;
      }
    if (!want_shortfall) node_slack(snap, w.n_pad, &slack_);
  }
  if (want_shortfall) node_left(snap, w.n_pad, &left_);
  w_ = &w;
  n_pods_ = static_cast<int32_t>(na);
  blocks_ = shortfall_blocks(w.Wp);
  lists_ = pq != nullptr;
  shortfall_ = want_shortfall;
  want_mask_ = node_mask;
  want_short_ = want_shortfall && node_short;
  view_ = view != nullptr;
  chunks_ = NodeViewChunks{};
  slots_.clear();
  if (view_) {
    chunks_ = node_view_chunks(w.Wp, n_pods_, view->per);
    for (int32_t src : w.pod_src) slots_.push_back(view->slot ? view->slot[src - w.pod_base] : src - w.pod_base);
  }

  part_of(&at_.in[IN_PODS], &src_[IN_PODS], pods_.data(), na);
  part_of(&at_.in[IN_CTX], &src_[IN_CTX], centries_.data(), lists_ ? centries_.size() : 0);
  part_of(&at_.in[IN_COFF], &src_[IN_COFF], coff_.data(), lists_ ? coff_.size() : 0);
  if (shortfall_) part_of(&at_.in[IN_SLACK], &src_[IN_SLACK], left_.data(), left_.size());
  else part_of(&at_.in[IN_SLACK], &src_[IN_SLACK], slack_.data(), lists_ ? slack_.size() : 0);
  at_.in_bytes = up8(place(at_.in, IN_PARTS));
  if (view_) {  // behind the parts every call has: their layout is what it is without the switch
    part_of(&at_.view_slot, nullptr, slots_.data(), slots_.size());
    at_.view_slot.off = at_.in_bytes;
    at_.in_bytes = up8(at_.view_slot.off + at_.view_slot.bytes);
  }

  const size_t sf = shortfall_ && !view_ ? na : 0, dims = SR_SHORT_COUNT;
  part_of<int32_t>(&at_.out[OUT_SUMS], nullptr, nullptr, view_ ? 0 : na * kExplainSums);
  part_of<int32_t>(&at_.out[OUT_SSUMS], nullptr, nullptr, sf * kShortSums);
  part_of<int64_t>(&at_.out[OUT_OMIN], nullptr, nullptr, sf * dims);
  part_of<int32_t>(&at_.out[OUT_OAT], nullptr, nullptr, sf * dims);
  part_of<int64_t>(&at_.out[OUT_NSHORT], nullptr, nullptr, want_short_ ? na * ns * dims : 0);
  part_of<uint16_t>(&at_.out[OUT_MASKS], nullptr, nullptr, want_mask_ ? na * ns : 0);
  part_of<uint64_t>(&at_.out[OUT_PMIN], nullptr, nullptr, sf * blocks_ * dims);
  part_of<int32_t>(&at_.out[OUT_PAT], nullptr, nullptr, sf * blocks_ * dims);
  const size_t end = place(at_.out, OUT_PARTS);
  at_.zero_bytes = at_.out[OUT_OMIN].off;
  at_.out_bytes = at_.out[OUT_MASKS].off + at_.out[OUT_MASKS].bytes;
  at_.dev_out_bytes = shortfall_ ? end : at_.out_bytes;
  if (view_) {  // every per-query part is absent (end == 0): the partials are the buffer
    part_of<uint64_t>(&at_.view_part, nullptr, nullptr,
                      node_view_layout(n_pad, static_cast<size_t>(chunks_.chunks)).bytes / 8);
    at_.view_part.off = up8(end);
    at_.dev_out_bytes = at_.view_part.off + at_.view_part.bytes;
  }
  return SR_OK;
}

void ExplainStage::pack(char* in) const {
  pack_parts(in, at_.in, src_, IN_PARTS);
  if (at_.view_slot.bytes) std::memcpy(in + at_.view_slot.off, slots_.data(), at_.view_slot.bytes);
}

void ExplainStage::args(const char* in, char* out, ExplainPlanArgs* pa, ShortfallArgs* sa) const {
  *pa = ExplainPlanArgs{};
  *sa = ShortfallArgs{};
  ExplainArgs& a = pa->x;
  stage_args(*w_, n_pods_, in, at_.in, &a);
  a.pods = at_part<ExplainPod>(in, at_.in[IN_PODS]);
  a.sums = at_part<int32_t>(out, at_.out[OUT_SUMS]);
  a.node_mask = want_mask_ ? at_part<uint16_t>(out, at_.out[OUT_MASKS]) : nullptr;
  if (lists_) {
    pa->ctx = at_part<PlanCtxEntry>(in, at_.in[IN_CTX]);
    pa->ctx_off = at_part<int32_t>(in, at_.in[IN_COFF]);
    pa->node_slack = shortfall_ ? nullptr : at_part<int32_t>(in, at_.in[IN_SLACK]);
  }
  if (shortfall_) {
    sa->node_left = at_part<int64_t>(in, at_.in[IN_SLACK]);
    sa->sums = at_part<int32_t>(out, at_.out[OUT_SSUMS]);
    sa->part_min = at_part<uint64_t>(out, at_.out[OUT_PMIN]);
    sa->part_at = at_part<int32_t>(out, at_.out[OUT_PAT]);
    sa->blocks = blocks_;
    sa->only_min = at_part<int64_t>(out, at_.out[OUT_OMIN]);
    sa->only_at = at_part<int32_t>(out, at_.out[OUT_OAT]);
    sa->node_short = want_short_ ? at_part<int64_t>(out, at_.out[OUT_NSHORT]) : nullptr;
  }
}

void ExplainStage::view_args(const char* in, char* out, char* totals, ExplainPlanArgs* pa, NodeViewArgs* na) const {
  ShortfallArgs sa;
  args(in, out, pa, &sa);
  pa->x.sums = nullptr;  // (no per-query output is laid out)
  *na = NodeViewArgs{};
  na->node_left = at_part<int64_t>(in, at_.in[IN_SLACK]);
  na->slot = at_part<int32_t>(in, at_.view_slot);
  na->per = chunks_.per;
  na->chunks = chunks_.chunks;
  na->lists = lists_ ? 1 : 0;
  na->tot_stride = node_view_stride(w_->n_spot);
  const NodeViewLayout pl = node_view_layout(static_cast<size_t>(w_->n_pad), static_cast<size_t>(chunks_.chunks));
  char* part = out + at_.view_part.off;
  na->part_min = reinterpret_cast<uint64_t*>(part + pl.min);
  na->part_cnt = reinterpret_cast<int32_t*>(part + pl.cnt);
  na->part_at = reinterpret_cast<int32_t*>(part + pl.at);
  const NodeViewLayout tl = node_view_layout(static_cast<size_t>(na->tot_stride), 1);
  na->tot_min = reinterpret_cast<uint64_t*>(totals + tl.min);
  na->tot_cnt = reinterpret_cast<int32_t*>(totals + tl.cnt);
  na->tot_at = reinterpret_cast<int32_t*>(totals + tl.at);
}

void ExplainStage::unpack(const char* image, const int32_t* slot, sr_explain_out* out, sr_shortfall_out* sh) const {
  const size_t ns = static_cast<size_t>(w_->n_spot), dims = SR_SHORT_COUNT;
  const int32_t* sums = at_part<int32_t>(image, at_.out[OUT_SUMS]);
  const uint16_t* masks = at_part<uint16_t>(image, at_.out[OUT_MASKS]);
  const int32_t* ssums = at_part<int32_t>(image, at_.out[OUT_SSUMS]);
  const int64_t* omin = at_part<int64_t>(image, at_.out[OUT_OMIN]);
  const int32_t* oat = at_part<int32_t>(image, at_.out[OUT_OAT]);
  const int64_t* nshort = at_part<int64_t>(image, at_.out[OUT_NSHORT]);
  for (size_t q = 0; q < static_cast<size_t>(n_pods_); ++q) {
    const int32_t src = w_->pod_src[q] - w_->pod_base;
    const size_t i = static_cast<size_t>(slot ? slot[src] : src);
    const int32_t* s = sums + q * kExplainSums;
    std::copy_n(s, SR_WHY_COUNT, out->counts + i * SR_WHY_COUNT);
    out->feasible[i] = s[kExplainFeasible];
    out->first[i] = s[kExplainFirst] > 0 ? w_->n_pad - s[kExplainFirst] : -1;
    if (want_mask_) std::copy_n(masks + q * ns, ns, out->node_mask + i * ns);
    if (!shortfall_) continue;
    sh->near[i] = ssums[q * kShortSums];
    std::copy_n(ssums + q * kShortSums + 1, dims, sh->only_nodes + i * dims);
    std::copy_n(omin + q * dims, dims, sh->only_min + i * dims);
    std::copy_n(oat + q * dims, dims, sh->only_at + i * dims);
    if (want_short_) std::copy_n(nshort + q * ns * dims, ns * dims, sh->node_short + i * ns * dims);
  }
}

}  // namespace sr
