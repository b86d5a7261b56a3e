"""The reference pass of sr_plan_sequence_pdb on the CPU oracle, and the
disruption groups the limited-sequence tests share.

The pass is sequence_ref.reference_sequence with one check added before
anything else is asked of a candidate with pods: a candidate whose pods in
some group outnumber what the group still allows gets SR_CAND_PDB and is
passed over, whether it would have drained, failed or belonged to the
reference path; a drain spends its pods' allowances.  Fork, canDrainNode,
Revert and AddPod are the oracle's own.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np

from oracle_lib import OracleSnapshot, load_oracle
from sequence_ref import EMPTY, FB, OK, SKIPPED, RefSequence, SeqInput, reference_sequence
from spotplanner import capi

PDB = capi.SR_CAND_PDB


@dataclass
class RefPdbSequence(RefSequence):
    remaining: np.ndarray = None
    # refused candidate -> what canDrainNode says from the state the pass met it in (OK, a failing pod, FB);
    # filled when the pass is run with probe=True (the probe is reverted: the pass is not changed by it)
    would: Dict[int, int] = field(default_factory=dict)


def needs_of(cand_off, pod_group, n_groups, c):
    base = int(cand_off[0])
    g = np.asarray(pod_group[int(cand_off[c]) - base:int(cand_off[c + 1]) - base])
    return np.bincount(g[g >= 0], minlength=n_groups)


def reference_sequence_pdb(osnap: OracleSnapshot, cluster_ptr, cand_off, cand_pods, allowed, pod_group,
                           max_drains: Optional[int] = None, first_cand: int = 0,
                           probe: bool = False) -> RefPdbSequence:
    lib = load_oracle()
    cand_off = np.ascontiguousarray(cand_off, np.int32)
    cand_pods = np.ascontiguousarray(cand_pods, np.int32)
    remaining = np.array(allowed, np.int64)
    n = len(cand_off) - 1
    base = int(cand_off[0]) if n > 0 else 0
    status = np.full(n, SKIPPED, np.int32)
    node = np.full(int(cand_off[-1]) - base if n > 0 else 0, -1, np.int32)
    drained, stop, stop_cand, would = [], capi.SR_SEQ_END, -1, {}

    def can_drain(b, e):
        pods = np.ascontiguousarray(cand_pods[b:e])
        omap = np.full(e - b, -1, np.int32)
        assert lib.oracle_snapshot_fork(osnap.h) == 0
        r = lib.oracle_can_drain_node(osnap.h, cluster_ptr, capi.ptr(pods, capi.P32), e - b, capi.ptr(omap, capi.P32))
        assert lib.oracle_snapshot_revert(osnap.h) == 0
        return r, pods, omap

    for c in range(first_cand, n):
        b, e = int(cand_off[c]), int(cand_off[c + 1])
        if e == b:
            status[c] = EMPTY
            continue
        need = needs_of(cand_off, pod_group, len(remaining), c)
        if np.any(need > remaining):
            status[c] = PDB
            if probe:
                r = can_drain(b, e)[0]
                would[c] = FB if r == -2 else OK if r < 0 else r
            continue
        r, pods, omap = can_drain(b, e)
        if r == -2:
            status[c] = FB
            stop, stop_cand = capi.SR_SEQ_FALLBACK, c
            break
        node[b - base:e - base] = omap
        if r >= 0:
            status[c] = r
            continue
        status[c] = OK
        for k in range(e - b):
            lib.oracle_snapshot_add_pod(osnap.h, cluster_ptr, int(pods[k]), int(omap[k]))
        remaining -= need
        drained.append(c)
        if max_drains is not None and len(drained) == max_drains:
            stop = capi.SR_SEQ_BUDGET
            break
    return RefPdbSequence(np.array(drained, np.int32), stop, stop_cand, status, node,
                          remaining.astype(np.int32), would)


def pdb_reference(inp: SeqInput, key, allowed, pod_group, max_drains=None, first_cand=0, probe=False):
    """The limited pass from the base snapshot, computed once per (key, arguments) and never changed.  Returns
    (RefPdbSequence, node states)."""
    k = ("pdb", key, max_drains, first_cand, probe)
    if k not in inp._ref:
        osnap = inp.oracle_snapshot()
        r = reference_sequence_pdb(osnap, inp.ptr, inp.cand_off, inp.cand_pods, allowed, pod_group, max_drains,
                                   first_cand, probe)
        inp._ref[k] = (r, [osnap.node_state(i) for i in range(len(inp.spot))])
        osnap.close()
    return inp._ref[k]


def groups_for(inp: SeqInput, seed: int):
    """3 to 40 groups with allowances of 0 to 6.  Most pods of a candidate share a group (replicas of one
    workload land together), some belong to another, about a quarter to none."""
    n = len(inp.cand_off) - 1
    r = np.random.RandomState((zlib.crc32(b"pdb-groups") ^ seed ^ (7919 * int(inp.cand_off[-1]))) & 0x7fffffff)
    n_groups = int(r.randint(3, 41))
    allowed = r.randint(0, 7, n_groups).astype(np.int32)
    pod_group = np.full(int(inp.cand_off[-1] - inp.cand_off[0]) if n else 0, -1, np.int32)
    off = inp.cand_off - inp.cand_off[0]
    for c in range(n):
        home = int(r.randint(0, n_groups))
        for q in range(int(off[c]), int(off[c + 1])):
            u = r.random_sample()
            pod_group[q] = -1 if u < 0.25 else home if u < 0.8 else int(r.randint(0, n_groups))
    return allowed, pod_group


# The random inputs of the limited-sequence tests and the seed of each one's groups, chosen on the oracle so
# that the facts test_sequence_pdb_reference.py asserts hold (pdb_facts).
RANDOM_INPUTS = {
    "plain-4": 0,
    "features-11": 4,
    "c5": 0,
    "vol-11": 0,
    "spread-22": 0,
    "realistic-80": 0,
    "c3-tight": 0,
}


def pdb_facts(inp: SeqInput, allowed, pod_group):
    """(refused candidates, refused candidates the oracle finds drainable from the state the pass met them in
    that lie below a later drain, drained candidates whose mapping differs from the unlimited pass's, drains
    after the first refusal)."""
    ref, _ = pdb_reference(inp, "facts-%d" % zlib.crc32(np.asarray(pod_group).tobytes() + np.asarray(allowed).tobytes()),
                           allowed, pod_group, probe=True)
    plain, _ = inp.reference()
    off = inp.cand_off - inp.cand_off[0]
    refused = [c for c in range(len(ref.status)) if ref.status[c] == PDB]
    last = int(ref.drained[-1]) if len(ref.drained) else -1
    masked = [c for c in refused if ref.would[c] == OK and c < last]
    moved = [c for c in ref.drained
             if not np.array_equal(ref.node_of_pod[off[c]:off[c + 1]], plain.node_of_pod[off[c]:off[c + 1]])]
    after = [c for c in ref.drained if refused and c > refused[0]]
    return len(refused), len(masked), len(moved), len(after)


def masking_groups(inp: SeqInput):
    """One group holding every pod of the unlimited pass's first drain, allowing one eviction fewer than it
    needs: that candidate is refused, drainable, and the first drainable candidate K2 sees in round one."""
    plain, _ = inp.reference()
    c = int(plain.drained[0])
    off = inp.cand_off - inp.cand_off[0]
    pod_group = np.full(int(off[-1]), -1, np.int32)
    pod_group[off[c]:off[c + 1]] = 0
    return c, np.array([off[c + 1] - off[c] - 1], np.int32), pod_group
