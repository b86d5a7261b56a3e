"""Hand cases for sr_evacuate_plan: scenarios with the answer worked out by hand -- which spot positions are lost,
which pods move, where every pod goes on the surviving nodes (-1: stranded; positions are those of the ORIGINAL
list), what the call must say about the scenario (`how`) and, for the stranded pods a case pins, the SURVIVING
nodes refusing per reason in the pod's own context.

A scenario outside the rule (NOT_PLAIN) carries the answer on the really reduced snapshot all the same, so the CPU
test can show that it differs from what masking the standing snapshot would give (`differs`): the clause is
there for a reason.

tests/test_evacuate_reference.py proves the cases on the CPU (the reduced-snapshot oracle of
tests/evacuate_ref.py and the host view), tests/test_gpu_evacuate.py runs them through the C ABI."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

from explain_cases import CPU, MEMORY, PODS
from explain_plan_cases import pool
from known_answer import P, used
from spotplanner.model import (Container, ContainerPort, GiB, LabelSelector, Pod, PodAffinityTerm,
                               TopologySpreadConstraint, VolumeWorld)

JUDGED, FALLBACK, NOT_PLAIN = 1, 2, 3


@dataclass
class EScen:
    lost: List[int]
    pods: List[Pod]                        # the pods to re-place: pods of `base` (by identity) or pods of their own
    how: int
    node_of_pod: List[int]                 # the answer on the really reduced snapshot (all -1 for FALLBACK)
    counts: Dict[int, Dict[int, int]] = field(default_factory=dict)  # stranded index -> {SR_WHY_* bit: nodes}
    differs: bool = False                  # NOT_PLAIN: masking the standing snapshot gives another answer

    @property
    def stranded(self) -> int:
        return -1 if self.how != JUDGED else sum(1 for j in self.node_of_pod if j < 0)

    @property
    def first(self) -> int:
        return -1 if self.how != JUDGED else next((k for k, j in enumerate(self.node_of_pod) if j < 0), -1)


@dataclass
class ECase:
    name: str
    nodes: list
    base: list
    scens: List[EScen]
    world: Optional[VolumeWorld] = None


def _hp(name, port, cpu=10):
    return Pod(name, containers=[Container(cpu_milli=cpu, ports=[ContainerPort(port)])])


def _empty(n):
    return [[] for _ in range(n)]


def _judged():
    # ---- three empty 1000m nodes; the first fit of every pod on the standing snapshot is node 0
    n = 3
    a = [P("a%d" % k, cpu=600) for k in range(3)]
    yield ECase("lost_node_was_the_first_fit", pool(n), _empty(n), [
        EScen([0], a, JUDGED, [1, 2, -1], counts={2: {CPU: 2}}),      # two survivors, each 600m full
        EScen([], a, JUDGED, [0, 1, 2]),                              # nothing lost: sr_blockers_plan's loop
        EScen([0, 1, 2], a, JUDGED, [-1, -1, -1], counts={0: {}, 1: {}, 2: {}}),  # nothing survives: zero rows
        EScen([1], [], JUDGED, []),                                   # nothing to move
        EScen([2, 0], a, JUDGED, [1, -1, -1], counts={1: {CPU: 1}, 2: {CPU: 1}}),  # lost in any order
        EScen([1], a, JUDGED, [0, 2, -1], counts={2: {CPU: 2}}),      # a lost node in the middle is skipped
    ])
    # ---- the pods of the lost node itself: node 1 has 500m left, node 2 100m
    b0, b1, b2 = P("b0", cpu=600), P("b1", cpu=300), P("b2", cpu=100)
    base = [[b0, b1, b2], [used(cpu=500, name="u1")], [used(cpu=900, name="u2")]]
    yield ECase("pods_of_the_lost_node", pool(n), base, [
        EScen([0], [b0, b1, b2], JUDGED, [-1, 1, 1], counts={0: {CPU: 2}}),
        # losing node 1 instead: its pod does not fit behind node 0's 1000m, nor on node 2
        EScen([1], base[1], JUDGED, [-1], counts={0: {CPU: 2}}),
        EScen([2], base[2], JUDGED, [-1], counts={0: {CPU: 2}}),
    ])
    # ---- the lost node is the only one that admits the pod
    yield ECase("only_admitting_node_lost", pool(n, over={1: dict(cpu=4000)}), _empty(n), [
        EScen([1], [P("big", cpu=2000)], JUDGED, [-1], counts={0: {CPU: 2}}),
        EScen([0], [P("big2", cpu=2000)], JUDGED, [1]),
    ])
    # ---- accounting apart from the fit request: the init container asks 800m, AddPod accounts the 100m container,
    # so 900m still fit behind it on the one surviving node and 1m more does not
    ic = Pod("ic", containers=[Container(cpu_milli=100)], init_containers=[Container(cpu_milli=800)])
    yield ECase("init_container_accounts_less", pool(2), _empty(2), [
        EScen([0], [ic, P("a1", cpu=900), P("a2", cpu=1)], JUDGED, [1, 1, -1], counts={2: {CPU: 1}}),
    ])
    # ---- the pod count reached through the scenario's own pods: node 1 allows 3 pods and holds 1; the zero-request
    # pod behind is refused for the count alone; node 2 is full in cpu but not in pods
    base = [[], [used(cpu=10, name="u1")], [used(cpu=1000, name="u2")]]
    yield ECase("pod_count_through_own_pods", pool(n, over={1: dict(pods=3)}), base, [
        EScen([0], [P("a0", cpu=10), P("a1", cpu=10), P("a2", cpu=10), P("a3", cpu=0)], JUDGED, [1, 1, -1, 2],
              counts={2: {PODS: 1, CPU: 1}}),
    ])
    # ---- to the last milli, the last byte and the last pod slot: two and three pods on one node
    base = [[], [used(cpu=400, mem=1 * GiB, name="u1")]]
    yield ECase("exact_fits", pool(2, mem=2 * GiB, over={1: dict(pods=4)}), base, [
        EScen([0], [P("c0", cpu=300), P("c1", cpu=300), P("c2", cpu=1)], JUDGED, [1, 1, -1], counts={2: {CPU: 1}}),
        EScen([0], [P("m0", cpu=0, mem=GiB // 2), P("m1", cpu=0, mem=GiB // 2), P("m2", cpu=0, mem=1)], JUDGED,
              [1, 1, -1], counts={2: {MEMORY: 1}}),
        EScen([0], [P("s0", cpu=0), P("s1", cpu=0), P("s2", cpu=0), P("s3", cpu=0)], JUDGED, [1, 1, 1, -1],
              counts={3: {PODS: 1}}),
    ])
    # ---- one pod with a host port and one with a scalar are still arithmetic: node 1 holds port 80
    G = "nvidia.com/gpu"
    nodes = pool(n)
    nodes[2].scalar = {G: 1}
    base = [[], [_hp("h1", 80)], []]
    yield ECase("one_port_pod_one_scalar_pod", nodes, base, [
        EScen([0], [_hp("p0", 80), Pod("g0", containers=[Container(cpu_milli=10, scalar={G: 1})])], JUDGED, [2, 2]),
    ])


def _not_plain():
    H = "kubernetes.io/hostname"
    n = 3
    web, db = {"app": "web"}, {"app": "db"}

    def zoned():
        nodes = pool(n)
        for i, nd in enumerate(nodes):
            nd.labels = {H: nd.name, "zone": "a" if i < 2 else "b"}
        return nodes

    def lp(name, labels, cpu=10, **kw):
        return Pod(name, namespace="default", labels=labels, containers=[Container(cpu_milli=cpu)], **kw)
    # ---- a pod on the lost node repels from its whole zone: on the standing snapshot the web pod is kept out of
    # node 1 by a pod that is gone in S'
    guard = lp("guard", db, pod_anti_affinity=[PodAffinityTerm("zone", LabelSelector(web))])
    yield ECase("anti_affinity_pod_on_the_lost_node", zoned(), [[guard], [], []], [
        EScen([0], [lp("w", web)], NOT_PLAIN, [1], differs=True),
        EScen([2], [lp("w2", web)], JUDGED, [-1], counts={0: {1 << 9: 2}}),  # the guard survives: INTER_POD on zone a
    ])
    # ---- the moved pod's own anti-affinity: the db pod it avoids lives on the lost node
    yield ECase("moved_pod_with_anti_affinity", zoned(), [[lp("d", db)], [], []], [
        EScen([0], [lp("m", web, pod_anti_affinity=[PodAffinityTerm("zone", LabelSelector(db))])], NOT_PLAIN, [1],
              differs=True),
    ])
    # ---- the moved pod's affinity: the only pod it wants to be near lives on the lost node
    yield ECase("moved_pod_with_affinity", zoned(), [[lp("d", db)], [], []], [
        EScen([0], [lp("m", web, pod_affinity=[PodAffinityTerm("zone", LabelSelector(db))])], NOT_PLAIN, [-1],
              differs=True),
    ])
    # ---- spread: the standing snapshot still counts the lost node's two web pods in zone a
    sp = lp("s", web, topology_spread=[TopologySpreadConstraint(1, "zone", label_selector=LabelSelector(web))])
    yield ECase("moved_pod_with_spread", zoned(), [[lp("w0", web), lp("w1", web)], [], []], [
        EScen([0], [sp], NOT_PLAIN, [1], differs=True),
    ])
    # ---- two pods with the same host port meet on the node the first one took
    yield ECase("two_port_pods", pool(n), _empty(n), [
        EScen([0], [_hp("a0", 80), _hp("a1", 80)], NOT_PLAIN, [1, 2]),
    ])
    # ---- two scalar pods: node 1 has one unit
    G = "nvidia.com/gpu"
    nodes = pool(n)
    nodes[1].scalar = {G: 1}

    def gpu(name):
        return Pod(name, containers=[Container(cpu_milli=10, scalar={G: 1})])
    yield ECase("two_scalar_pods", nodes, _empty(n), [
        EScen([0], [gpu("g0"), gpu("g1")], NOT_PLAIN, [1, -1]),
    ])
    # ---- accounting: two requests of 2^61 bytes add up to 2^62, more than the encoder takes as a quantity
    yield ECase("requests_beyond_the_quantity_range", pool(n), _empty(n), [
        EScen([0], [P("h0", cpu=0, mem=1 << 61), P("h1", cpu=0, mem=1 << 61)], NOT_PLAIN, [-1, -1]),
    ])
    # ---- a pod outside the encoded predicate set: nothing is reported for its scenario, the others are judged
    yield ECase("fallback_pod", pool(n), _empty(n), [
        EScen([0], [P("a0", cpu=100), Pod("pvc", containers=[Container(cpu_milli=10)], has_pvc=True)], FALLBACK,
              [-1, -1]),
        EScen([0], [P("b0", cpu=600), P("b1", cpu=1001)], JUDGED, [1, -1], counts={1: {CPU: 2}}),
    ])


def cases() -> List[ECase]:
    out = list(_judged()) + list(_not_plain())
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
    """A case as one cluster: the scenario, the arrays of the call and the expected outputs."""

    def __init__(self, case: ECase):
        import numpy as np
        from helpers import Scenario
        self.case = case
        on_node = {id(p): None for ps in case.base for p in ps}
        query = []
        for sn in case.scens:
            for p in sn.pods:
                if id(p) not in on_node and not any(p is q for q in query):
                    query.append(p)
        self.sc = Scenario(case.nodes, case.base, query, volumes=case.world)
        index, i = {}, 0
        for ps in case.base:
            for p in ps:
                index[id(p)] = i
                i += 1
        for k, p in enumerate(query):
            index[id(p)] = self.sc.qidx(k)
        self.scen_off = np.zeros(len(case.scens) + 1, np.int32)
        self.scen_off[1:] = np.cumsum([len(sn.pods) for sn in case.scens])
        self.scen_pods = np.array([index[id(p)] for sn in case.scens for p in sn.pods], np.int32)
        self.lost_off = np.zeros(len(case.scens) + 1, np.int32)
        self.lost_off[1:] = np.cumsum([len(sn.lost) for sn in case.scens])
        self.lost_pos = np.array([j for sn in case.scens for j in sn.lost], np.int32)
        self.n_spot = len(case.nodes)
        self.how = np.array([sn.how for sn in case.scens], np.uint8)
        self.stranded = np.array([sn.stranded for sn in case.scens], np.int32)
        self.first = np.array([sn.first for sn in case.scens], np.int32)
        # what the call reports: nothing for a scenario that is not judged
        self.node_of_pod = np.array([j if sn.how == JUDGED else -1 for sn in case.scens for j in sn.node_of_pod], np.int32)
        # what the reduced-snapshot oracle says, also for NOT_PLAIN scenarios
        self.ref_node_of_pod = [list(sn.node_of_pod) for sn in case.scens]
        assert len(self.node_of_pod) == len(self.scen_pods)
        self.pinned = {}  # flat pod index -> counts row
        for s, sn in enumerate(case.scens):
            for k, row in sn.counts.items():
                assert sn.node_of_pod[k] < 0 and sn.how == JUDGED
                self.pinned[int(self.scen_off[s]) + k] = why_row(row)
