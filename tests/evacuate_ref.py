"""The contract of sr_evacuate_plan over the CPU oracle.  The reference REALLY removes the nodes: scenario s is
answered by the oracle's snapshot built from the spot list without lost[s],

    OracleSnapshot(cluster, spot without lost[s], node_pod_off, node_pod_idx)

by the loop of tests/blockers_ref.py over the scenario's pods, its positions mapped back to the original list.
`masked_blockers` is the other thing one could do -- keep the standing snapshot and merely never choose a lost
position -- which is what the product does where its rule proves the two equal; the hand cases use it to show
that outside the rule they really differ.

Shared by tests/test_evacuate_reference.py (CPU) and the GPU tests of the entry point."""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from blockers_ref import RefBlockers, oracle_blockers
from oracle_lib import OracleSnapshot, load_oracle


def surviving(n_spot: int, lost: Sequence[int]) -> List[int]:
    gone = {int(j) for j in lost}
    return [j for j in range(n_spot) if j not in gone]


def reduced_oracle(sc, lost):
    """(the oracle's snapshot without the lost positions, surviving positions in the original list)."""
    keep = surviving(len(sc.spot), lost)
    return OracleSnapshot(sc.ptr, sc.spot[keep], sc.node_pod_off, sc.node_pod_idx), keep


def reduced_product(sc, lost):
    """(a product snapshot handle built without the lost positions -- the caller destroys it --, surviving
    positions)."""
    import ctypes

    from spotplanner import capi
    keep = surviving(len(sc.spot), lost)
    spot = np.ascontiguousarray(sc.spot[keep], np.int32)
    lib = capi.load_planner()
    h = ctypes.c_void_p()
    st = lib.sr_snapshot_create(sc.ptr, capi.ptr(spot, capi.P32), len(spot), capi.ptr(sc.node_pod_off, capi.P32),
                                capi.ptr(sc.node_pod_idx, capi.P32), ctypes.byref(h))
    assert st == capi.SR_OK
    return h, keep


def oracle_evacuate(sc, pods, lost) -> RefBlockers:
    """One scenario on the really reduced snapshot; node_of_pod in positions of the original list."""
    osnap, keep = reduced_oracle(sc, lost)
    try:
        r = oracle_blockers(sc, osnap, pods, len(keep))
    finally:
        osnap.close()
    return RefBlockers(r.blockers, r.first, [keep[j] if j >= 0 else -1 for j in r.node_of_pod], r.fallback)


def oracle_evacuate_plan(sc, scen_off, scen_pods, lost_off, lost_pos):
    """Every scenario: dict(stranded, first, node_of_pod, fallback), node_of_pod relative to scen_off[0]."""
    n = len(scen_off) - 1
    base = int(scen_off[0])
    stranded, first = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    mapping = np.full(int(scen_off[n]) - base, -1, np.int32)
    fallback = np.zeros(n, np.uint8)
    for s in range(n):
        lo, hi = int(scen_off[s]), int(scen_off[s + 1])
        r = oracle_evacuate(sc, scen_pods[lo:hi], lost_pos[int(lost_off[s]):int(lost_off[s + 1])])
        stranded[s], first[s], fallback[s] = r.blockers, r.first, r.fallback
        mapping[lo - base:hi - base] = r.node_of_pod
    return dict(stranded=stranded, first=first, node_of_pod=mapping, fallback=fallback)


def masked_blockers(sc, osnap, pods, lost) -> List[int]:
    """The loop on the STANDING snapshot with the lost positions merely never chosen (reverted afterwards)."""
    ora = load_oracle()
    keep = surviving(len(sc.spot), lost)
    mapping = []
    assert ora.oracle_snapshot_fork(osnap.h) == 0
    try:
        for p in (int(p) for p in pods):
            at = next((j for j in keep if ora.oracle_check_predicates(osnap.h, sc.ptr, p, j)), -1)
            mapping.append(at)
            if at >= 0:
                ora.oracle_snapshot_add_pod(osnap.h, sc.ptr, p, at)
    finally:
        ora.oracle_snapshot_revert(osnap.h)
    return mapping


def first_fit_standing(sc, osnap, pod) -> int:
    """findSpotNodeForPod on the standing snapshot as it is."""
    ora = load_oracle()
    return next((j for j in range(len(sc.spot)) if ora.oracle_check_predicates(osnap.h, sc.ptr, int(pod), j)), -1)


def node_pods(sc, pos) -> List[int]:
    """The cluster pod indices the snapshot holds on spot position `pos`, in order."""
    node = int(sc.spot[pos])
    return [int(p) for p in sc.node_pod_idx[int(sc.node_pod_off[node]):int(sc.node_pod_off[node + 1])]]


def scenarios(sc, lost_sets, moved=None):
    """(scen_off, scen_pods, lost_off, lost_pos) for the lost sets; a scenario moves `moved[s]` or, by default, the
    pods of its lost nodes in NodeInfoArray order."""
    scen_off, scen_pods, lost_off, lost_pos = [0], [], [0], []
    for s, lost in enumerate(lost_sets):
        pods = moved[s] if moved is not None else [p for j in sorted(lost) for p in node_pods(sc, j)]
        scen_pods.extend(int(p) for p in pods)
        scen_off.append(len(scen_pods))
        lost_pos.extend(int(j) for j in lost)
        lost_off.append(len(lost_pos))
    return (np.array(scen_off, np.int32), np.array(scen_pods, np.int32), np.array(lost_off, np.int32),
            np.array(lost_pos, np.int32))


def n_minus_one(n_spot):
    return [[j] for j in range(n_spot)]


def pools(n_spot, k):
    """k pools: position j belongs to pool j % k."""
    return [[j for j in range(n_spot) if j % k == r] for r in range(k)]


def compacted(pods, mapping, k):
    """Stranded pod k's context as sr_explain_candidate takes it on the REDUCED snapshot: the scenario's list with
    the stranded pods before k removed -- (pods, their ORIGINAL positions, k's place in that list)."""
    keep = [q for q in range(k) if mapping[q] >= 0]
    return ([int(pods[q]) for q in keep] + [int(pods[k])], [int(mapping[q]) for q in keep] + [-1], len(keep))


def reduced_in_context(sc, osnap, keep, pods, mapping, k):
    """explain_plan_cases.oracle_in_context on a reduced snapshot (`osnap`, `keep` from reduced_oracle): forked
    and filled with pods[:k] at the ORIGINAL positions mapping[:k]; the oracle's yes / no for pods[k] on every
    surviving node and fitsRequest's PODS / CPU / MEMORY / EPHEMERAL bits from its node state after the fill;
    reverted."""
    from explain_cases import CPU, EPHEMERAL, MEMORY, PODS
    ora = load_oracle()
    A = sc.enc.a
    pod = int(pods[k])
    req = (int(A["req_cpu"][pod]), int(A["req_mem"][pod]), int(A["req_eph"][pod]))
    lists_scalar = A["pod_scalar_off"][pod + 1] > A["pod_scalar_off"][pod]
    alloc = (A["alloc_cpu"], A["alloc_mem"], A["alloc_eph"])
    back = {j: i for i, j in enumerate(keep)}
    assert ora.oracle_snapshot_fork(osnap.h) == 0
    try:
        for q in range(k):
            ora.oracle_snapshot_add_pod(osnap.h, sc.ptr, int(pods[q]), back[int(mapping[q])])
        fits = [ora.oracle_check_predicates(osnap.h, sc.ptr, pod, i) for i in range(len(keep))]
        bits = []
        for i, j in enumerate(keep):
            node = int(sc.spot[j])
            requested, num_pods = osnap.node_state(i)
            m = PODS if num_pods + 1 > int(A["alloc_pods"][node]) else 0
            if any(req) or lists_scalar:
                for d, bit in enumerate((CPU, MEMORY, EPHEMERAL)):
                    if int(alloc[d][node]) < req[d] + requested[d]:
                        m |= bit
            bits.append(m)
    finally:
        ora.oracle_snapshot_revert(osnap.h)
    return fits, bits
