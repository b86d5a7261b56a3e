"""Reference for sr_shortfall_pods / sr_shortfall_plan, from the CPU oracle alone.

The masks are sr_explain_pods' and sr_explain_plan's, checked against the
oracle as explain_ref.Reference and explain_plan_cases.oracle_in_context do
it.  Every expected number is fitsRequest's arithmetic [upstream k8s v1.19.2
noderesources/fit.go] on the oracle's own node state
(oracle_snapshot_node_state) and the cluster arrays:

  cpu / memory / ephemeral   request + requested - allocatable   where the mask holds the bit, else 0
  pods                       len(pods) + 1 - allowed pods        where the mask holds PODS, else 0 (at most 2^63 - 1)

and the reductions follow from the masks and those numbers (`reduce_row`).  A
context is the oracle snapshot forked and filled with the candidate's earlier
pods (`context`).  The host view (tools/explain_plan_view.cpp) is bound here
for the CPU tests."""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np

from explain_ref import CPU, EPHEMERAL, MEMORY, PODS, RESOURCE_BITS, Reference
from oracle_lib import load_oracle
from spotplanner import capi

INT64_MAX = (1 << 63) - 1
DIM_BITS = (CPU, MEMORY, EPHEMERAL, PODS)  # capi.SR_SHORT_* order
assert [capi.SR_SHORT_CPU, capi.SR_SHORT_MEMORY, capi.SR_SHORT_EPHEMERAL, capi.SR_SHORT_PODS] == [0, 1, 2, 3]


def node_shortfalls(mask, req, requested, alloc, num_pods, alloc_pods):
    """The four shortfalls of one node whose mask is `mask` (Python integers: nothing wraps)."""
    out = [0, 0, 0, 0]
    for d in range(3):
        if mask & DIM_BITS[d]:
            out[d] = int(req[d]) + int(requested[d]) - int(alloc[d])
    if mask & PODS:
        out[3] = min(int(num_pods) + 1 - int(alloc_pods), INT64_MAX)
    return out


def reduce_row(masks, shorts):
    """(near, only_nodes[4], only_min[4], only_at[4]) of one query from its nodes' masks and shortfalls."""
    near = sum(1 for m in masks if int(m) != 0 and int(m) & ~RESOURCE_BITS == 0)
    only_nodes, only_min, only_at = [0] * 4, [0] * 4, [-1] * 4
    for d, bit in enumerate(DIM_BITS):
        at = [j for j, m in enumerate(masks) if int(m) == bit]
        only_nodes[d] = len(at)
        if at:
            only_min[d] = min(int(shorts[j][d]) for j in at)
            only_at[d] = next(j for j in at if int(shorts[j][d]) == only_min[d])
            assert only_min[d] >= 1
    return near, only_nodes, only_min, only_at


def node_states(osnap, n_spot):
    """([n_spot][3] requested, [n_spot] pods) of the oracle snapshot as it stands."""
    st = [osnap.node_state(j) for j in range(n_spot)]
    return [s[0] for s in st], [s[1] for s in st]


def expected_shorts(sc, pod, masks, requested, num_pods):
    """[n_spot][4] for cluster pod `pod` whose nodes' masks are `masks`, on the given oracle state."""
    A = sc.enc.a
    req = (int(A["req_cpu"][pod]), int(A["req_mem"][pod]), int(A["req_eph"][pod]))
    return [node_shortfalls(int(masks[j]), req, requested[j],
                            (A["alloc_cpu"][j], A["alloc_mem"][j], A["alloc_eph"][j]), num_pods[j], A["alloc_pods"][j])
            for j in range(len(masks))]


def resource_bits(sc, pod, requested, num_pods):
    """fitsRequest's PODS / CPU / MEMORY / EPHEMERAL bits of cluster pod `pod` on every node of the given state."""
    A = sc.enc.a
    req = (int(A["req_cpu"][pod]), int(A["req_mem"][pod]), int(A["req_eph"][pod]))
    lists_scalar = A["pod_scalar_off"][pod + 1] > A["pod_scalar_off"][pod]
    alloc = (A["alloc_cpu"], A["alloc_mem"], A["alloc_eph"])
    out = []
    for j in range(len(requested)):
        m = PODS if num_pods[j] + 1 > int(A["alloc_pods"][j]) else 0
        if any(req) or lists_scalar:
            for d in range(3):
                if int(alloc[d][j]) < req[d] + requested[j][d]:
                    m |= DIM_BITS[d]
        out.append(m)
    return out


@contextlib.contextmanager
def context(sc, osnap, pods, mapping, k):
    """The oracle snapshot forked and filled the way canDrainNode fills it (pods[:k] at mapping[:k]); reverted."""
    ora = load_oracle()
    assert ora.oracle_snapshot_fork(osnap.h) == 0
    try:
        for q in range(k):
            ora.oracle_snapshot_add_pod(osnap.h, sc.ptr, int(pods[q]), int(mapping[q]))
        yield
    finally:
        ora.oracle_snapshot_revert(osnap.h)


def check_query(sc, osnap, pod, masks, shorts, n_spot, what=""):
    """One judged query against the oracle snapshot as it stands (inside `context` for a plan query): the masks'
    yes / no and resource bits, then every node's shortfalls.  Returns the expected reductions."""
    ora = load_oracle()
    requested, num_pods = node_states(osnap, n_spot)
    fits = [ora.oracle_check_predicates(osnap.h, sc.ptr, int(pod), j) for j in range(n_spot)]
    assert [int(int(m) == 0) for m in masks] == fits, what
    assert [int(m) & RESOURCE_BITS for m in masks] == resource_bits(sc, int(pod), requested, num_pods), what
    want = expected_shorts(sc, int(pod), masks, requested, num_pods)
    got = [[int(x) for x in row] for row in shorts]
    assert got == want, (what, [(j, got[j], want[j]) for j in range(n_spot) if got[j] != want[j]][:4])
    return reduce_row(masks, want)


def check_reduced(short, i, want, what=""):
    """Entry i of a ShortfallResult equals the reductions `want` (reduce_row's tuple)."""
    near, only_nodes, only_min, only_at = want
    assert int(short.near[i]) == near, (what, i, int(short.near[i]), near)
    assert [int(x) for x in short.only_nodes[i]] == only_nodes, (what, i)
    assert [int(x) for x in short.only_min[i]] == only_min, (what, i, list(short.only_min[i]), only_min)
    assert [int(x) for x in short.only_at[i]] == only_at, (what, i, list(short.only_at[i]), only_at)


def check_none(short, i, what=""):
    """A fallback pod, or a candidate that was not asked."""
    assert short.near[i] == -1, (what, i)
    assert not short.only_nodes[i].any() and not short.only_min[i].any() and (short.only_at[i] == -1).all(), (what, i)
    if short.node_short is not None:
        assert not short.node_short[i].any(), (what, i)


class ShortfallReference(Reference):
    """explain_ref.Reference (one random scenario, its candidate pods as queries, the oracle's answers computed
    once) with the shortfalls: `check` takes node_mask [n][n_spot], node_short [n][n_spot][4] and fallback [n] of
    pod_indices() and returns the expected reductions per pod (None for a fallback pod)."""

    def check(self, node_mask, node_short, fallback):
        out = []
        requested, num_pods = self.requested, self.num_pods
        for i in range(self.n):
            assert int(fallback[i]) == int(self.fallback[i]), i
            if self.fallback[i]:
                assert not np.asarray(node_mask[i]).any() and not np.asarray(node_short[i]).any(), i
                out.append(None)
                continue
            row = node_mask[i]
            for j in range(self.n_spot):
                m = int(row[j])
                assert (m == 0) == (self.fits[i][j] == 1), (self.pods[i].name, j, hex(m))
                assert m & RESOURCE_BITS == self.resource_mask(i, j), (self.pods[i].name, j, hex(m))
            want = expected_shorts(self.sc, self.sc.qidx(i), row, requested, num_pods)
            got = [[int(x) for x in r] for r in node_short[i]]
            assert got == want, (i, [(j, got[j], want[j]) for j in range(self.n_spot) if got[j] != want[j]][:4])
            out.append(reduce_row(row, want))
        return out


# ---- the host view (lib/libsrexplainview.so): sr_shortfall_pods_view, sr_shortfall_plan_view
def _bound_view():
    from test_explain_plan_reference import load_view
    lib = load_view()
    if getattr(lib.sr_shortfall_pods_view, "argtypes", None) is None:
        PC, VP = ctypes.POINTER(capi.sr_cluster), ctypes.c_void_p
        lib.sr_shortfall_pods_view.argtypes = [PC, VP, capi.P32, ctypes.c_int32, capi.PU16, capi.P64, capi.PU8]
        lib.sr_shortfall_pods_view.restype = ctypes.c_int32
        lib.sr_shortfall_plan_view.argtypes = [PC, VP, ctypes.POINTER(capi.sr_candidates), capi.P32, capi.P32, capi.PU8,
                                               capi.PU16, capi.P64, capi.PU8]
        lib.sr_shortfall_plan_view.restype = ctypes.c_int32
    return lib


@contextlib.contextmanager
def _view_snapshot(lib, sc):
    h = ctypes.c_void_p()
    assert lib.sr_snapshot_create(sc.ptr, capi.ptr(sc.spot, capi.P32), len(sc.spot), capi.ptr(sc.node_pod_off, capi.P32),
                                  capi.ptr(sc.node_pod_idx, capi.P32), ctypes.byref(h)) == capi.SR_OK
    try:
        yield h
    finally:
        lib.sr_snapshot_destroy(h)


def view_pods(sc, pods):
    """dict(masks [n][n_spot], shorts [n][n_spot][4], fallback [n]) of cluster pods `pods`, by the host statements."""
    lib = _bound_view()
    pods = np.ascontiguousarray(pods, np.int32)
    n, n_spot = len(pods), len(sc.spot)
    masks = np.zeros((max(n, 1), n_spot), np.uint16)
    shorts = np.zeros((max(n, 1), n_spot, 4), np.int64)
    fb = np.zeros(max(n, 1), np.uint8)
    with _view_snapshot(lib, sc) as h:
        st = lib.sr_shortfall_pods_view(sc.ptr, h, capi.ptr(pods, capi.P32), n, capi.ptr(masks, capi.PU16),
                                        capi.ptr(shorts, capi.P64), capi.ptr(fb, capi.PU8))
    assert st == capi.SR_OK, st
    return dict(masks=masks[:n], shorts=shorts[:n], fallback=fb[:n])


def view_plan(sc, cand_off, cand_pods, at_pod, node_of_pod):
    """dict(how [n], masks, shorts, fallback) of the batched candidates (others: zeros), by the host statements."""
    lib = _bound_view()
    cand_off = np.ascontiguousarray(cand_off, np.int32)
    cand_pods = np.ascontiguousarray(cand_pods, np.int32)
    at_pod = np.ascontiguousarray(at_pod, np.int32)
    node_of_pod = np.ascontiguousarray(node_of_pod, np.int32)
    n, n_spot = len(cand_off) - 1, len(sc.spot)
    how, fb = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
    masks = np.zeros((max(n, 1), n_spot), np.uint16)
    shorts = np.zeros((max(n, 1), n_spot, 4), np.int64)
    c = capi.sr_candidates(n, capi.ptr(cand_off, capi.P32), capi.ptr(cand_pods, capi.P32), None)
    with _view_snapshot(lib, sc) as h:
        st = lib.sr_shortfall_plan_view(sc.ptr, h, ctypes.byref(c), capi.ptr(at_pod, capi.P32),
                                        capi.ptr(node_of_pod, capi.P32), capi.ptr(how, capi.PU8),
                                        capi.ptr(masks, capi.PU16), capi.ptr(shorts, capi.P64), capi.ptr(fb, capi.PU8))
    assert st == capi.SR_OK, st
    return dict(how=how[:n], masks=masks[:n], shorts=shorts[:n], fallback=fb[:n])
