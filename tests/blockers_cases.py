"""Hand cases for sr_blockers_plan: candidates with the answer of canDrainNode's loop without its early return
worked out by hand -- where every pod goes (-1: a blocker), the way the candidate must go (`how`) and, for the
blockers the case pins, the spot nodes refusing per reason in the blocker's own context.

tests/test_blockers_reference.py proves the cases on the CPU (the oracle loop of tests/blockers_ref.py and the
host view), tests/test_gpu_blockers.py runs them through the C ABI."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

from explain_cases import CPU, INTER_POD, PODS, PORTS, SCALAR, SPREAD
from explain_plan_cases import BATCHED, NONE, SINGLE, pool
from known_answer import P, used
from spotplanner.model import (Container, ContainerPort, LabelSelector, Pod, PodAffinityTerm, TopologySpreadConstraint,
                               VolumeWorld)


@dataclass
class BCand:
    pods: List[Pod]
    how: int
    node_of_pod: List[int]                 # the answer; every entry -1 when not asked or fallback
    ask: int = 0                           # >= 0: asked
    counts: Dict[int, Dict[int, int]] = field(default_factory=dict)  # blocker index -> {SR_WHY_* bit: nodes}
    fallback: int = 0

    @property
    def blockers(self) -> int:
        if self.ask < 0 or self.fallback:
            return -1
        return sum(1 for j in self.node_of_pod if j < 0)

    @property
    def first(self) -> int:
        if self.ask < 0 or self.fallback:
            return -1
        return next((k for k, j in enumerate(self.node_of_pod) if j < 0), -1)


@dataclass
class BCase:
    name: str
    nodes: list
    base: list
    cands: List[BCand]
    world: Optional[VolumeWorld] = None


def _hp(name, port, cpu=10):
    return Pod(name, containers=[Container(cpu_milli=cpu, ports=[ContainerPort(port)])])


def _empty(n):
    return [[] for _ in range(n)]


def _batched():
    # ---- three 1000m nodes: a blocker first, in the middle and last; none; every pod; not asked; no pods
    n = 3
    yield BCase("blocker_first_middle_last", pool(n), _empty(n), [
        BCand([P("a0", cpu=1001), P("a1", cpu=600), P("a2", cpu=600)], BATCHED, [-1, 0, 1], counts={0: {CPU: 3}}),
        BCand([P("b0", cpu=600), P("b1", cpu=1001), P("b2", cpu=600)], BATCHED, [0, -1, 1], counts={1: {CPU: 3}}),
        BCand([P("c0", cpu=600), P("c1", cpu=600), P("c2", cpu=1001)], BATCHED, [0, 1, -1], counts={2: {CPU: 3}}),
        BCand([P("d0", cpu=600), P("d1", cpu=600)], BATCHED, [0, 1]),
        BCand([P("e0", cpu=1001), P("e1", cpu=1002), P("e2", cpu=1003)], BATCHED, [-1, -1, -1],
              counts={0: {CPU: 3}, 1: {CPU: 3}, 2: {CPU: 3}}),
        BCand([P("f0", cpu=1001), P("f1", cpu=10)], NONE, [-1, -1], ask=-1),
        BCand([], BATCHED, []),
        BCand([P("g0", cpu=1001)], NONE, [-1], ask=-3),
    ])
    # ---- two blockers with placed pods between and behind them: two nodes, 400m left on each after a0 / a1; a2
    # fits neither; a3 takes node 0 down to 100m; a4 (500m) fits neither; a5 (400m) fills node 1
    n = 2
    yield BCase("two_blockers_placed_between", pool(n), _empty(n), [
        BCand([P("a0", cpu=600), P("a1", cpu=600), P("a2", cpu=600), P("a3", cpu=300), P("a4", cpu=500),
               P("a5", cpu=400)], BATCHED, [0, 1, -1, 0, -1, 1], counts={2: {CPU: 2}, 4: {CPU: 2}}),
    ])
    # ---- one node filled by arithmetic alone: 300 + 300 + 300 fit, 200 more overflows, 100 fits again
    n = 1
    yield BCase("node_filled_by_arithmetic", pool(n), _empty(n), [
        BCand([P("a0", cpu=300), P("a1", cpu=300), P("a2", cpu=300), P("a3", cpu=200), P("a4", cpu=100)], BATCHED,
              [0, 0, 0, -1, 0], counts={3: {CPU: 1}}),
        BCand([P("b0", cpu=300), P("b1", cpu=300), P("b2", cpu=300), P("b3", cpu=101), P("b4", cpu=100)], BATCHED,
              [0, 0, 0, -1, 0], counts={3: {CPU: 1}}),
        BCand([P("c0", cpu=300), P("c1", cpu=300), P("c2", cpu=300), P("c3", cpu=100), P("c4", cpu=1)], BATCHED,
              [0, 0, 0, 0, -1], counts={4: {CPU: 1}}),
    ])
    # ---- accounting apart from the fit request: the init container asks 800m, AddPod accounts the 100m container,
    # so 900m still fit behind it and 1m more does not; were acc the request, a1 would be the blocker
    ic = Pod("a0", containers=[Container(cpu_milli=100)], init_containers=[Container(cpu_milli=800)])
    yield BCase("init_container_accounts_less", pool(n), _empty(n), [
        BCand([ic, P("a1", cpu=900), P("a2", cpu=1)], BATCHED, [0, 0, -1], counts={2: {CPU: 1}}),
    ])
    # ---- the pod count reached through the candidate's own pods: node 1 allows 3 pods and holds 1; node 0 is full
    # in pods and cpu from the start.  The zero-request pod behind is refused for the count alone
    n = 2
    base = [[used(cpu=1000)], [used(cpu=10)]]
    yield BCase("pod_count_through_own_pods", pool(n, over={0: dict(pods=1), 1: dict(pods=3)}), base, [
        BCand([P("a0", cpu=10), P("a1", cpu=10), P("a2", cpu=10), P("a3", cpu=0)], BATCHED, [1, 1, -1, -1],
              counts={2: {CPU: 1, PODS: 2}, 3: {PODS: 2}}),
    ])


def _single():
    # ---- two pods with host ports: node 1 is full, so the second meets the first's port on node 0
    n = 2
    base = [[], [used(cpu=1000)]]
    yield BCase("two_port_pods", pool(n), base, [
        BCand([_hp("a0", 80), _hp("a1", 80), P("a2", cpu=10)], SINGLE, [0, -1, 0], counts={1: {PORTS: 1, CPU: 1}}),
        BCand([_hp("b0", 80), P("b1", cpu=10)], BATCHED, [0, 0]),  # one port pod: plain
    ])
    H = "kubernetes.io/hostname"
    n = 5
    nodes = pool(n)
    for i, nd in enumerate(nodes):
        nd.labels = {H: nd.name, "zone": "a" if i < 3 else "b"}
    web, db = {"app": "web"}, {"app": "db"}

    def lp(name, labels, anti=None, cpu=10):
        return Pod(name, namespace="default", labels=labels, containers=[Container(cpu_milli=cpu)], pod_anti_affinity=anti)
    # ---- an anti-affinity pod: it avoids the node the candidate's first pod took
    yield BCase("anti_affinity_pod", nodes, _empty(n), [
        BCand([lp("a0", db), lp("a1", web, [PodAffinityTerm(H, LabelSelector(db))]), lp("a2", db)], SINGLE, [0, 1, 0]),
        # on the whole zone: zone a is gone, and a pod too large for anything blocks in between
        BCand([lp("b0", db), lp("b1", web, cpu=1001), lp("b2", web, [PodAffinityTerm("zone", LabelSelector(db))])],
              SINGLE, [0, -1, 3], counts={1: {CPU: 5}}),
        BCand([lp("c0", web, [PodAffinityTerm(H, LabelSelector(db))])], SINGLE, [0]),  # conservative: any such pod
    ])
    # ---- spread on a later pod: zone a counts the two earlier pods, zone b none
    sp = Pod("a2", namespace="default", labels=web, containers=[Container(cpu_milli=10)],
             topology_spread=[TopologySpreadConstraint(1, "zone", label_selector=LabelSelector(web))])
    yield BCase("spread_on_a_later_pod", nodes, _empty(n), [
        BCand([lp("a0", web), lp("a1", web), sp], SINGLE, [0, 0, 3]),
    ])
    # ---- two scalar pods: node 1 has one unit, node 2 two
    G = "nvidia.com/gpu"

    def gpu(name, k=1):
        return Pod(name, containers=[Container(cpu_milli=10, scalar={G: k})])
    gnodes = pool(n)
    gnodes[1].scalar = {G: 1}
    gnodes[2].scalar = {G: 2}
    yield BCase("two_scalar_pods", gnodes, _empty(n), [
        BCand([gpu("a0"), gpu("a1"), gpu("a2"), gpu("a3"), P("a4", cpu=10)], SINGLE, [1, 2, 2, -1, 0],
              counts={3: {SCALAR: 5}}),
        BCand([P("b0", cpu=10), gpu("b1")], BATCHED, [0, 1]),  # one scalar pod: plain
    ])
    # ---- a pod outside the encoded predicate set: nothing is reported for its candidate
    yield BCase("fallback_pod", pool(n), _empty(n), [
        BCand([P("a0", cpu=100), Pod("pvc", containers=[Container(cpu_milli=10)], has_pvc=True), P("a2", cpu=1001)],
              SINGLE, [-1, -1, -1], fallback=1),
        BCand([P("b0", cpu=600), P("b1", cpu=1001)], BATCHED, [0, -1], counts={1: {CPU: 5}}),
    ])


def cases() -> List[BCase]:
    out = list(_batched()) + list(_single())
    names = [c.name for c in out]
    assert len(names) == len(set(names))
    return out


def why_row(counts: Dict[int, int]) -> List[int]:
    """{SR_WHY_* bit: nodes} as a counts row."""
    from spotplanner import capi
    row = [0] * capi.SR_WHY_COUNT
    for bit, v in counts.items():
        row[bit.bit_length() - 1] = v
    return row


class Built:
    """A case as one cluster: the scenario, the candidate arrays, ask, and the expected outputs."""

    def __init__(self, case: BCase):
        import numpy as np
        from helpers import Scenario
        from spotplanner import capi
        self.case = case
        flat = [p for cd in case.cands for p in cd.pods]
        self.sc = Scenario(case.nodes, case.base, flat, volumes=case.world)
        self.cand_off = np.zeros(len(case.cands) + 1, np.int32)
        self.cand_off[1:] = np.cumsum([len(cd.pods) for cd in case.cands])
        self.cand_pods = np.array([self.sc.qidx(i) for i in range(len(flat))], np.int32)
        self.ask = np.array([cd.ask for cd in case.cands], np.int32)
        self.n_spot = len(case.nodes)
        self.node_of_pod = np.array([x for cd in case.cands for x in cd.node_of_pod], np.int32)
        assert len(self.node_of_pod) == len(flat)
        self.blockers = np.array([cd.blockers for cd in case.cands], np.int32)
        self.first = np.array([cd.first for cd in case.cands], np.int32)
        self.fallback = np.array([cd.fallback for cd in case.cands], np.uint8)
        self.how = np.array([cd.how for cd in case.cands], np.uint8)
        self.pinned = {}  # flat pod index -> counts row
        for c, cd in enumerate(case.cands):
            for k, row in cd.counts.items():
                assert cd.node_of_pod[k] < 0
                self.pinned[int(self.cand_off[c]) + k] = why_row(row)
        self.why_count = capi.SR_WHY_COUNT
