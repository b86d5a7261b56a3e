"""Reference for sr_node_view_pods / sr_node_view_plan: `fold` computes every output array from per-query masks
and shortfalls in plain Python integers -- the one reference of the node-view tests.  Where the per-query arrays
come from (the oracle-checked host view on the CPU, the sibling calls sr_shortfall_* on the GPU, hand-written
cases) is the caller's.  The host view's two node-view exports (tools/explain_plan_view.cpp) are bound here."""
from __future__ import annotations

import ctypes

import numpy as np

from explain_ref import RESOURCE_BITS
from shortfall_ref import DIM_BITS, _bound_view, _view_snapshot
from spotplanner import capi

FIELDS = ("judged", "admits", "near", "refuses", "sole", "sole_min", "sole_at")


def fold(masks, shorts, slots, n_spot):
    """masks[q][node], shorts[q][node][4] and slots[q] of the judged queries (asked, not fallback), in any order:
    dict(judged, admits[n_spot], near[n_spot], refuses[n_spot][12], sole[n_spot][12], sole_min[n_spot][4],
    sole_at[n_spot][4]).  sole_min / sole_at is the lexicographic minimum of (shortfall, slot)."""
    W, D = capi.SR_WHY_COUNT, capi.SR_SHORT_COUNT
    out = dict(judged=len(masks), admits=[0] * n_spot, near=[0] * n_spot, refuses=[[0] * W for _ in range(n_spot)],
               sole=[[0] * W for _ in range(n_spot)], sole_min=[[0] * D for _ in range(n_spot)],
               sole_at=[[-1] * D for _ in range(n_spot)])
    assert len(masks) == len(shorts) == len(slots) and len(set(int(s) for s in slots)) == len(slots)
    best = [[None] * D for _ in range(n_spot)]
    for row, sf, slot in zip(masks, shorts, slots):
        assert len(row) == n_spot
        for j in range(n_spot):
            m = int(row[j])
            out["admits"][j] += m == 0
            out["near"][j] += m != 0 and m & ~RESOURCE_BITS == 0
            for r in range(W):
                out["refuses"][j][r] += m >> r & 1
                out["sole"][j][r] += m == 1 << r
            for d, bit in enumerate(DIM_BITS):
                if m == bit:
                    key = (int(sf[j][d]), int(slot))
                    if best[j][d] is None or key < best[j][d]:
                        best[j][d] = key
    for j in range(n_spot):
        for d in range(D):
            if best[j][d] is not None:
                out["sole_min"][j][d], out["sole_at"][j][d] = best[j][d]
    return out


def as_dict(res):
    """A rescheduler.NodeViewResult as `fold` returns it."""
    return dict(judged=int(res.judged), admits=[int(x) for x in res.admits], near=[int(x) for x in res.near],
                refuses=[[int(x) for x in r] for r in res.refuses], sole=[[int(x) for x in r] for r in res.sole],
                sole_min=[[int(x) for x in r] for r in res.sole_min], sole_at=[[int(x) for x in r] for r in res.sole_at])


def same(got, want, what=""):
    """Two fold dicts, field for field (the first node that differs is named)."""
    for f in FIELDS:
        if got[f] != want[f]:
            if f == "judged":
                raise AssertionError((what, f, got[f], want[f]))
            j = next(j for j in range(len(want[f])) if got[f][j] != want[f][j])
            raise AssertionError((what, f, "node", j, got[f][j], want[f][j]))


def fold_pods(why, short, n_spot):
    """`fold` of sr_shortfall_pods' per-query arrays (rescheduler.shortfall_arrays with node_mask and node_short):
    the fallback pods left out, a query's slot its asked index."""
    q = [i for i in range(len(why.fallback)) if not why.fallback[i]]
    return fold([why.node_mask[i] for i in q], [short.node_short[i] for i in q], q, n_spot)


def fold_plan(why, short, at_pod, n_spot):
    """`fold` of sr_shortfall_plan's per-query arrays: the candidates asked and not fallback, slot = candidate."""
    q = [c for c in range(len(at_pod)) if at_pod[c] >= 0 and not why.fallback[c]]
    return fold([why.node_mask[c] for c in q], [short.node_short[c] for c in q], q, n_spot)


# ---- the host view (lib/libsrexplainview.so): sr_node_view_pods_view, sr_node_view_plan_view
def _bound():
    lib = _bound_view()
    if getattr(lib.sr_node_view_pods_view, "argtypes", None) is None:
        PC, VP, PO = ctypes.POINTER(capi.sr_cluster), ctypes.c_void_p, ctypes.POINTER(capi.sr_node_view_out)
        lib.sr_node_view_pods_view.argtypes = [PC, VP, capi.P32, ctypes.c_int32, PO]
        lib.sr_node_view_pods_view.restype = ctypes.c_int32
        lib.sr_node_view_plan_view.argtypes = [PC, VP, ctypes.POINTER(capi.sr_candidates), capi.P32, capi.P32, capi.PU8, PO]
        lib.sr_node_view_plan_view.restype = ctypes.c_int32
    return lib


def _out(n, n_spot):
    from spotplanner.rescheduler import _node_view_out
    return _node_view_out(n, n_spot)


def view_pods(sc, pods):
    """(fold dict, fallback [n]) of cluster pods `pods` by the host statement (node_view_fold)."""
    lib = _bound()
    pods = np.ascontiguousarray(pods, np.int32)
    o, result = _out(len(pods), len(sc.spot))
    with _view_snapshot(lib, sc) as h:
        st = lib.sr_node_view_pods_view(sc.ptr, h, capi.ptr(pods, capi.P32), len(pods), ctypes.byref(o))
    assert st == capi.SR_OK, st
    res = result()
    return as_dict(res), res.fallback


def view_plan(sc, cand_off, cand_pods, at_pod, node_of_pod):
    """(fold dict over the batched candidates, fallback [n], how [n]) by the host statement."""
    lib = _bound()
    cand_off = np.ascontiguousarray(cand_off, np.int32)
    cand_pods = np.ascontiguousarray(cand_pods, np.int32)
    at_pod = np.ascontiguousarray(at_pod, np.int32)
    node_of_pod = np.ascontiguousarray(node_of_pod, np.int32)
    n = len(cand_off) - 1
    how = np.zeros(max(n, 1), np.uint8)
    c = capi.sr_candidates(n, capi.ptr(cand_off, capi.P32), capi.ptr(cand_pods, capi.P32), None)
    o, result = _out(n, len(sc.spot))
    with _view_snapshot(lib, sc) as h:
        st = lib.sr_node_view_plan_view(sc.ptr, h, ctypes.byref(c), capi.ptr(at_pod, capi.P32),
                                        capi.ptr(node_of_pod, capi.P32), capi.ptr(how, capi.PU8), ctypes.byref(o))
    assert st == capi.SR_OK, st
    res = result()
    return as_dict(res), res.fallback, how[:n]
