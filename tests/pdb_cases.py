"""Hand-derived cases of sr_plan_sequence_pdb: two spot nodes of 1000 mCPU with
no pods, candidates of a few pods that differ in CPU only, first fit in node
order.  Every expectation below was worked out by hand from the pass in
include/sr_planner.h; test_sequence_pdb_reference.py holds the oracle to them
and test_gpu_sequence_pdb.py the planner."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np

from sequence_ref import SeqInput, from_scenario
from spotplanner import capi
from spotplanner.model import Container, Node, Pod

OK, FB, SKIPPED, PDB = capi.SR_CAND_OK, capi.SR_CAND_FALLBACK, capi.SR_CAND_SKIPPED, capi.SR_CAND_PDB
END, BUDGET, FALLBACK = capi.SR_SEQ_END, capi.SR_SEQ_BUDGET, capi.SR_SEQ_FALLBACK


@dataclass
class PdbCase:
    # candidates: lists of (mCPU, group) pods; a negative mCPU marks a pod outside the encoded predicate set
    cands: List[List[tuple]]
    allowed: List[int]
    drained: List[int]
    status: List[int]
    node_of_pod: List[int]
    remaining: List[int]
    stop: int = END
    stop_cand: int = -1
    max_drains: Optional[int] = None
    rounds: Optional[int] = None  # device rounds, where the case fixes them
    equals_plain: bool = False    # the allowances never bind: sr_plan_sequence's result


CASES: Dict[str, PdbCase] = {
    # (a) allowances that never bind.  c0 -> n0, c1 does not fit beside it -> n1, c2 fits nowhere
    "a-never-binds": PdbCase([[(600, 0)], [(600, 0)], [(600, 0)]], [10],
                             drained=[0, 1], status=[OK, OK, 0], node_of_pod=[0, 1, -1], remaining=[8],
                             equals_plain=True),
    # (b) c0 fits (both pods on n0) but needs 2 of a group allowing 1; c1 then takes n0, where it would not
    # have fitted beside c0's 600
    "b-refused-though-fits": PdbCase([[(300, 0), (300, 0)], [(700, -1)]], [1],
                                     drained=[1], status=[PDB, OK], node_of_pod=[-1, -1, 0], remaining=[1]),
    # (c) c0 spends group 0's last allowance; c1 of the same group is refused although it fits; c2 of group 1
    "c-last-allowance": PdbCase([[(400, 0)], [(100, 0)], [(100, 1)]], [1, 1],
                                drained=[0, 2], status=[OK, PDB, OK], node_of_pod=[0, -1, 0], remaining=[0, 0]),
    # (d) a refused candidate that fits nowhere: SR_CAND_PDB, not failing pod 0
    "d-refused-would-fail": PdbCase([[(5000, 0)], [(100, -1)]], [0],
                                    drained=[1], status=[PDB, OK], node_of_pod=[-1, 0], remaining=[0]),
    # (e) c0 is outside the encoded set and refused: passed over.  c2 is outside it and not refused: the stop
    "e-fallbacks": PdbCase([[(-1, 0)], [(100, 1)], [(-1, 1)], [(100, -1)]], [0, 5],
                           drained=[1], status=[PDB, OK, FB, SKIPPED], node_of_pod=[-1, 0, -1, -1],
                           remaining=[0, 4], stop=FALLBACK, stop_cand=2),
    # (f) a group allowing nothing touches every candidate: no drain and no device round
    "f-nothing-allowed": PdbCase([[(100, 0)], [(100, -1), (100, 0)], [(100, 0), (100, 0)]], [0],
                                 drained=[], status=[PDB, PDB, PDB], node_of_pod=[-1] * 5, remaining=[0], rounds=0),
    # (g) pods of no group beside limited ones: only the limited ones count
    "g-ungrouped-pods": PdbCase([[(200, 0), (200, -1), (200, 0)], [(100, -1), (100, 0)], [(100, -1), (100, -1)]],
                                [2], drained=[0, 2], status=[OK, PDB, OK], node_of_pod=[0, 0, 0, -1, -1, 0, 0],
                                remaining=[0]),
    # (h) the uninterrupted pass of the resume test: c0, c1 (group 0 spent), c2 refused, c3 (500 does not fit
    # beside 600 on n0), c4 refused
    "h-uninterrupted": PdbCase([[(300, 0)], [(300, 0)], [(300, 0)], [(500, 1)], [(300, 0)]], [2, 1],
                               drained=[0, 1, 3], status=[OK, OK, PDB, OK, PDB], node_of_pod=[0, 0, -1, 1, -1],
                               remaining=[0, 0]),
    # ... stopped by max_drains = 1 with allowances left; test_*_resume goes on from first_cand = 1 with
    # allowed = remaining and must arrive at h-uninterrupted
    "h-budget-one": PdbCase([[(300, 0)], [(300, 0)], [(300, 0)], [(500, 1)], [(300, 0)]], [2, 1],
                            drained=[0], status=[OK, SKIPPED, SKIPPED, SKIPPED, SKIPPED],
                            node_of_pod=[0, -1, -1, -1, -1], remaining=[1, 1], stop=BUDGET, max_drains=1),
}

_inputs: Dict[str, SeqInput] = {}


def case_input(name: str) -> SeqInput:
    """The case's cluster, built once per process."""
    if name not in _inputs:
        case = CASES[name]
        nodes = [Node("s%d" % i, cpu_milli=1000) for i in range(2)]
        cands = [[Pod("c%d-%d" % (c, k), containers=[Container(cpu_milli=max(cpu, 0))], has_pvc=cpu < 0)
                  for k, (cpu, _) in enumerate(ps)] for c, ps in enumerate(case.cands)]
        _inputs[name] = from_scenario(nodes, [[] for _ in nodes], cands)
    return _inputs[name]


def case_limits(name: str):
    case = CASES[name]
    return (np.array(case.allowed, np.int32), np.array([g for ps in case.cands for _, g in ps], np.int32))
