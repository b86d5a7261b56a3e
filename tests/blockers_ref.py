"""The contract of sr_blockers_plan over the CPU oracle: canDrainNode's loop with the `return err` at the
first unplaceable pod replaced by "note the pod and go on, state unchanged".

    Fork
    for k in 0..n:
        j = first spot position whose predicates pass for p[k]
        j found:  node_of_pod[k] = j; AddPod(p[k], j)
        none:     node_of_pod[k] = -1; p[k] is a blocker
    Revert

Shared by tests/test_blockers_reference.py (CPU) and the GPU tests of the entry point."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import numpy as np

from oracle_lib import load_oracle


@dataclass
class RefBlockers:
    blockers: int            # -1: a pod of the candidate lies outside the encoded set
    first: int
    node_of_pod: List[int]
    fallback: int


def oracle_blockers(sc, osnap, pods, n_spot) -> RefBlockers:
    """The loop for one candidate (`pods`: cluster pod indices); the oracle's snapshot is reverted."""
    ora = load_oracle()
    pods = [int(p) for p in pods]
    if any(ora.oracle_pod_needs_fallback(osnap.h, sc.ptr, p) for p in pods):
        return RefBlockers(-1, -1, [-1] * len(pods), 1)
    mapping = []
    assert ora.oracle_snapshot_fork(osnap.h) == 0
    try:
        for p in pods:
            at = next((j for j in range(n_spot) if ora.oracle_check_predicates(osnap.h, sc.ptr, p, j)), -1)
            mapping.append(at)
            if at >= 0:
                ora.oracle_snapshot_add_pod(osnap.h, sc.ptr, p, at)
    finally:
        ora.oracle_snapshot_revert(osnap.h)
    stuck = [k for k, j in enumerate(mapping) if j < 0]
    return RefBlockers(len(stuck), stuck[0] if stuck else -1, mapping, 0)


def oracle_blockers_plan(sc, osnap, cand_off, cand_pods, ask, n_spot):
    """Every asked candidate (ask[c] >= 0) by the loop: dict(blockers, first, node_of_pod, fallback) as
    sr_blockers_out holds them, node_of_pod relative to cand_off[0]."""
    n = len(cand_off) - 1
    base = int(cand_off[0])
    blockers, first = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    mapping = np.full(int(cand_off[n]) - base, -1, np.int32)
    fallback = np.zeros(n, np.uint8)
    for c in range(n):
        if ask[c] < 0:
            continue
        lo, hi = int(cand_off[c]), int(cand_off[c + 1])
        r = oracle_blockers(sc, osnap, cand_pods[lo:hi], n_spot)
        blockers[c], first[c], fallback[c] = r.blockers, r.first, r.fallback
        mapping[lo - base:hi - base] = r.node_of_pod
    return dict(blockers=blockers, first=first, node_of_pod=mapping, fallback=fallback)


def compacted(pods, mapping, k):
    """Blocker k's context as sr_explain_candidate takes it: the candidate's list with the blockers before k
    removed -- (pods, their positions, k's place in that list)."""
    keep = [q for q in range(k) if mapping[q] >= 0]
    return ([int(pods[q]) for q in keep] + [int(pods[k])], [int(mapping[q]) for q in keep] + [-1], len(keep))
