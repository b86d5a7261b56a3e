// explain.cpp — explain programs from a tagged workload, and their host evaluation.
#include "explain.hpp"

#include "host.hpp"

namespace sr {

bool build_explain(const Workload& w, ExplainPrograms* out) {
  out->off.assign(1, 0);
  out->ops.clear();
  if (w.cls_why.size() != w.cls_prog.size() || w.atom_why.size() != static_cast<size_t>(w.n_atoms) ||
      w.n_atoms >= kMaxExplainAtoms)
    return false;
  for (int32_t k = 0; k < w.n_classes; ++k) {
    for (int32_t i = w.cls_prog_off[k]; i < w.cls_prog_off[k + 1]; ++i) {
      const int32_t atom = w.cls_prog[i] >> 2, kind = w.cls_prog[i] & 3;
      const uint8_t why = w.cls_why[i];
      if (why & WHY_DECIDED) {  // the class is refused everywhere, for each group that decided it
        if (why & WHY_DEC_NODE_AFFINITY) out->ops.push_back(x_op(0, WHY_NODE_AFFINITY, X_ALL));
        if (why & WHY_DEC_VOLUMES) out->ops.push_back(x_op(0, WHY_VOLUMES, X_ALL));
        if (why & WHY_DEC_INTER_POD) out->ops.push_back(x_op(0, WHY_INTER_POD, X_ALL));
      } else if (why == WHY_COMPOSITE) {  // atom 0, then one AND-NOT per untolerated taint of the set
        const int32_t c = atom - w.comp_first;
        out->ops.push_back(x_op(0, WHY_PODS, X_AND));
        for (int32_t j = w.comp_taint_off[c]; j < w.comp_taint_off[c + 1]; ++j) {
          const int32_t ta = w.comp_taint_atom[j];
          out->ops.push_back(x_op(ta, w.atom_why[ta], X_ANDNOT));
        }
      } else if (why < SR_WHY_COUNT) {
        out->ops.push_back(x_op(atom, why, kind));  // PROG_* and X_* kinds agree
      } else if (why == WHY_NONE) {
        // the closing operation of the empty class: no pod is explained from it (Workload::pod_cls)
      } else {
        return false;  // an operation the encoder did not tag
      }
    }
    out->off.push_back(static_cast<int32_t>(out->ops.size()));
  }
  static_assert(int(PROG_AND) == int(X_AND) && int(PROG_ANDNOT) == int(X_ANDNOT) &&
                    int(PROG_TERM_START) == int(X_TERM_START) && int(PROG_TERM_AND) == int(X_TERM_AND),
                "operation kinds shared with the class programs");
  return true;
}

void explain_pods(const Workload& w, std::vector<ExplainPod>* out) {
  const size_t na = w.pod_src.size();
  out->resize(na);
  for (size_t q = 0; q < na; ++q) {
    ExplainPod& p = (*out)[q];
    p.cls = w.pod_cls[q];
    for (int d = 0; d < 3; ++d) p.req[d] = static_cast<int64_t>(w.pod_rec[q * 6 + d]);
    // an active pod with an all-zero request lists no scalar resource (the
    // encoder sends such a pod to the reference path): fitsRequest returns
    // after the pod count
    p.resources = (p.req[0] | p.req[1] | p.req[2]) != 0 ? 1 : 0;
  }
}

uint32_t explain_node(const ExplainPrograms& x, const ExplainPod& p, const uint64_t* atoms, int32_t Wp,
                      const int64_t* node_free, int32_t n_pad, int32_t node) {
  uint32_t mask = 0;
  bool in_terms = false, any = false, term = false;
  auto bit = [&](int32_t atom) { return (atoms[static_cast<size_t>(atom) * Wp + (node >> 6)] >> (node & 63) & 1) != 0; };
  for (int32_t i = x.off[p.cls]; i < x.off[p.cls + 1]; ++i) {
    const int32_t op = x.ops[i], atom = op >> 8, why = op >> 3 & 31, kind = op & 7;
    switch (kind) {
      case X_AND:
        if (!bit(atom)) mask |= 1u << why;
        break;
      case X_ANDNOT:
        if (bit(atom)) mask |= 1u << why;
        break;
      case X_TERM_START:
        any = any || (in_terms && term);
        in_terms = true;
        term = bit(atom);
        break;
      case X_TERM_AND:
        term = term && bit(atom);
        break;
      default:
        mask |= 1u << why;
    }
  }
  if (in_terms && !(any || term)) mask |= 1u << WHY_NODE_AFFINITY;
  if (p.resources)
    for (int d = 0; d < 3; ++d)
      if (p.req[d] > node_free[static_cast<size_t>(d) * n_pad + node]) mask |= 1u << (WHY_CPU + d);
  return mask;
}

}  // namespace sr
