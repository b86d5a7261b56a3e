"""Hand cases for sr_explain_plan: candidates whose stop pod is explained after
their own earlier pods (rescheduler.go:366), each with the SR_WHY_* mask of
every spot node derived by hand and the way the candidate must go (`how`).

A case names, per candidate, its pods, the pod asked for (at_pod), where the
plan put the pods before it (node_of_pod) and `masks`: {node: mask} for the
nodes that refuse, every other node 0.  The mapping is the caller's: the cases
put earlier pods where they need them, as sr_explain_candidate allows.

Plain contexts (BATCHED) pin the arithmetic of the touched nodes at its edges:
free - acc == request fits and one unit less refuses, for cpu, memory and
ephemeral storage; two earlier pods on one node merged into one entry; the pod
count at slack == earlier pods; a zero-request stop pod; accounting that
differs from the fit request; a host-port stop pod after port-free pods.  The
SINGLE cases carry the mask only the earlier pod causes, for every rule that
sends a context that way.  Pools of 63, 64, 65, 257 and 300 nodes put touched
nodes at lanes 0 and 63 of a row word, at node 256 (first of a second block)
and at the last node; one query has 70 earlier pods over three row words, next
to queries with empty lists.

tests/test_explain_plan_reference.py proves the cases on the CPU (the view
library and the oracle), tests/test_gpu_explain_plan.py runs them through the
C ABI.  Past these sizes -- pools of 320 to 4,300 nodes, lists of thousands of
entries, 300 classes, the second launch of the grid split, the quantity limit
of the plain rule -- tests/explain_plan_sizes.py takes over, with
tests/test_explain_plan_sizes_reference.py and
tests/test_gpu_explain_plan_sizes.py."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

from explain_cases import CPU, EPHEMERAL, INTER_POD, MEMORY, PODS, PORTS, SCALAR, SPREAD, VOLUMES
from known_answer import N, P, used
from spotplanner.model import (Container, ContainerPort, GiB, LabelSelector, MiB, Pod, PodAffinityTerm,
                               TopologySpreadConstraint, Volume, VolumeWorld)

NONE, BATCHED, SINGLE = 0, 1, 2
OK, FALLBACK, EMPTY = -1, -2, -3  # SR_CAND_*


@dataclass
class Cand:
    pods: List[Pod]
    at_pod: int
    node_of_pod: List[int]           # one per pod; entries from at_pod on are not read
    how: int
    masks: Dict[int, int] = field(default_factory=dict)  # refusing nodes (others 0); NONE: nothing is evaluated
    ctx: Optional[list] = None       # BATCHED: the context entries [(node, pods, (cpu, memory, ephemeral))]
    first: Optional[int] = None      # the first feasible node, where the case pins it


@dataclass
class PlanCase:
    name: str
    nodes: list
    base: list
    cands: List[Cand]
    world: Optional[VolumeWorld] = None

    def expected(self, c: int) -> List[int]:
        return [self.cands[c].masks.get(j, 0) for j in range(len(self.nodes))]


E10 = 10 * GiB


def pool(n, cpu=1000, mem=8 * GiB, pods=110, eph=E10, over=None):
    """n equal nodes; over = {index: dict of N() arguments} for the ones that differ."""
    out, over = [], over or {}
    for i in range(n):
        kw = dict(cpu=cpu, mem=mem, pods=pods, eph=eph)
        kw.update(over.get(i, {}))
        out.append(N("n%d" % i, **kw))
    return out


def _hp(name, port, cpu=10):
    return Pod(name, containers=[Container(cpu_milli=cpu, ports=[ContainerPort(port)])])


def _plain():
    # ---- cpu: 1000 - 300 == 700 fits, 1000 - 301 refuses; lane 62 (last node of 63) and lane 0
    n = 63
    yield PlanCase("cpu_last_milli", pool(n), [[] for _ in range(n)], [
        Cand([P("a0", cpu=300), P("a1", cpu=700)], 1, [62, -1], BATCHED, {}, [(62, 1, (300, 0, 0))], first=0),
        Cand([P("b0", cpu=301), P("b1", cpu=700)], 1, [62, -1], BATCHED, {62: CPU}, [(62, 1, (301, 0, 0))]),
        Cand([P("c0", cpu=301), P("c1", cpu=700)], 1, [0, -1], BATCHED, {0: CPU}, [(0, 1, (301, 0, 0))], first=1),
        Cand([P("d0", cpu=700)], 0, [-1], BATCHED, {}, [], first=0),
    ])
    # ---- memory and ephemeral storage the same way; lane 63 of a full word
    n = 64
    base = [[] for _ in range(n)]
    base[63] = [used(mem=1 * GiB, eph=1 * GiB)]
    m, e = 3 * GiB, 4 * GiB  # node 63 has 7 GiB memory and 9 GiB ephemeral free
    yield PlanCase("memory_and_ephemeral_last_byte", pool(n), base, [
        Cand([P("a0", cpu=1, mem=7 * GiB - m), P("a1", cpu=1, mem=m)], 1, [63, -1], BATCHED, {},
             [(63, 1, (1, 7 * GiB - m, 0))]),
        Cand([P("b0", cpu=1, mem=7 * GiB - m + 1), P("b1", cpu=1, mem=m)], 1, [63, -1], BATCHED, {63: MEMORY},
             [(63, 1, (1, 7 * GiB - m + 1, 0))]),
        Cand([P("c0", cpu=1, eph=9 * GiB - e), P("c1", cpu=1, eph=e)], 1, [63, -1], BATCHED, {},
             [(63, 1, (1, 0, 9 * GiB - e))]),
        Cand([P("d0", cpu=1, eph=9 * GiB - e + 1), P("d1", cpu=1, eph=e)], 1, [63, -1], BATCHED, {63: EPHEMERAL},
             [(63, 1, (1, 0, 9 * GiB - e + 1))]),
        Cand([P("e0", cpu=400, mem=5 * GiB, eph=6 * GiB), P("e1", cpu=700, mem=m, eph=e)], 1, [63, -1], BATCHED,
             {63: CPU | MEMORY | EPHEMERAL}, [(63, 1, (400, 5 * GiB, 6 * GiB))]),
    ])
    # ---- two earlier pods on one node, neither enough alone: one merged entry; node 64 is the last node and
    # lane 0 of the second word; the candidate beside it splits the same pods over two nodes and fits
    n = 65
    yield PlanCase("two_pods_merge_on_one_node", pool(n), [[] for _ in range(n)], [
        Cand([P("a0", cpu=200), P("a1", cpu=200, mem=1 * MiB), P("a2", cpu=700)], 2, [64, 64, -1], BATCHED, {64: CPU},
             [(64, 2, (400, 1 * MiB, 0))]),
        Cand([P("b0", cpu=200), P("b1", cpu=200), P("b2", cpu=700)], 2, [64, 63, -1], BATCHED, {},
             [(63, 1, (200, 0, 0)), (64, 1, (200, 0, 0))]),
        Cand([P("c0", cpu=150), P("c1", cpu=150), P("c2", cpu=700)], 2, [64, 64, -1], BATCHED, {},
             [(64, 2, (300, 0, 0))]),
    ])
    # ---- the pod count: node 256 (first node of a second block) allows 3 pods and holds 1, slack 2
    n = 257
    base = [[] for _ in range(n)]
    base[256] = [used(cpu=10)]
    nodes = pool(n, over={256: dict(pods=3)})
    yield PlanCase("pod_count_at_slack", nodes, base, [
        Cand([P("a0", cpu=10), P("a1", cpu=10), P("a2", cpu=10)], 2, [256, 256, -1], BATCHED, {256: PODS},
             [(256, 2, (20, 0, 0))]),
        Cand([P("b0", cpu=10), P("b1", cpu=10), P("b2", cpu=10)], 2, [256, 255, -1], BATCHED, {},
             [(255, 1, (10, 0, 0)), (256, 1, (10, 0, 0))]),
        Cand([P("c0", cpu=10), P("c1", cpu=10), P("c2", cpu=10), P("c3", cpu=985)], 3, [256, 256, 256, -1], BATCHED,
             {256: PODS | CPU}, [(256, 3, (30, 0, 0))]),
    ])
    # ---- a zero-request stop pod: no CPU bit on a node the earlier pods over-commit, PODS when the count says so
    n = 64
    nodes = pool(n, over={0: dict(pods=2), 63: dict(pods=2)})
    yield PlanCase("zero_request_stop_pod", nodes, [[] for _ in range(n)], [
        Cand([P("a0", cpu=600), P("a1", cpu=600), P("a2", cpu=0)], 2, [0, 0, -1], BATCHED, {0: PODS},
             [(0, 2, (1200, 0, 0))], first=1),
        Cand([P("b0", cpu=600), P("b1", cpu=600), P("b2", cpu=0)], 2, [1, 1, -1], BATCHED, {},
             [(1, 2, (1200, 0, 0))], first=0),
        Cand([P("c0", cpu=600), P("c1", cpu=600), P("c2", cpu=1)], 2, [63, 62, -1], BATCHED, {},
             [(62, 1, (600, 0, 0)), (63, 1, (600, 0, 0))]),
        Cand([P("d0", cpu=600), P("d1", cpu=600), P("d2", cpu=1)], 2, [1, 1, -1], BATCHED, {1: CPU},
             [(1, 2, (1200, 0, 0))]),
    ])
    # ---- accounting apart from the fit request: an init container asks 800m, the pod accounts its 100m container
    n = 63
    ic = Pod("a0", containers=[Container(cpu_milli=100)], init_containers=[Container(cpu_milli=800)])
    ic2 = Pod("b0", containers=[Container(cpu_milli=101)], init_containers=[Container(cpu_milli=800)])
    yield PlanCase("init_container_accounts_less", pool(n), [[] for _ in range(n)], [
        Cand([ic, P("a1", cpu=900)], 1, [5, -1], BATCHED, {}, [(5, 1, (100, 0, 0))]),
        Cand([ic2, P("b1", cpu=900)], 1, [5, -1], BATCHED, {5: CPU}, [(5, 1, (101, 0, 0))]),
        # asked itself, the init container is its fit request: 800m after 201m
        Cand([P("c0", cpu=201), dataclass_copy(ic, "c1")], 1, [5, -1], BATCHED, {5: CPU}, [(5, 1, (201, 0, 0))]),
    ])
    # ---- a host-port stop pod whose earlier pods have no port stays batched: the base pod's port refuses on node
    # 2, the earlier pod's cpu on node 3
    n = 65
    base = [[] for _ in range(n)]
    base[2] = [_hp("web", 80)]
    yield PlanCase("host_port_after_port_free_pods", pool(n), base, [
        Cand([P("a0", cpu=500), _hp("a1", 80, cpu=600)], 1, [3, -1], BATCHED, {2: PORTS, 3: CPU},
             [(3, 1, (500, 0, 0))]),
        Cand([P("b0", cpu=500), _hp("b1", 80, cpu=600)], 1, [2, -1], BATCHED, {2: PORTS | CPU},
             [(2, 1, (500, 0, 0))]),
    ])
    # ---- 70 earlier pods over three row words (nodes 60 .. 129) beside queries with empty lists, and the last node
    n = 300
    many = [P("m%d" % i, cpu=400) for i in range(70)] + [P("m-stop", cpu=700)]
    yield PlanCase("seventy_earlier_pods", pool(n), [[] for _ in range(n)], [
        Cand([P("e0", cpu=700)], 0, [-1], BATCHED, {}, [], first=0),
        Cand(many, 70, list(range(60, 130)) + [-1], BATCHED, {j: CPU for j in range(60, 130)},
             [(j, 1, (400, 0, 0)) for j in range(60, 130)], first=0),
        Cand([P("e1", cpu=1001)], 0, [-1], BATCHED, {j: CPU for j in range(n)}, [], first=-1),
        Cand([P("l0", cpu=301), P("l1", cpu=301), P("l2", cpu=700)], 2, [299, 0, -1], BATCHED, {0: CPU, 299: CPU},
             [(0, 1, (301, 0, 0)), (299, 1, (301, 0, 0))], first=1),
        Cand([P("l3", cpu=300), P("l4", cpu=700)], 1, [299, -1], BATCHED, {}, [(299, 1, (300, 0, 0))]),
    ])
    # ---- a placed pod asked for: its first feasible node is where a first-fit plan puts it; and candidates the
    # plan did not stop in pass through untouched
    n = 63
    yield PlanCase("placed_pod_and_statuses", pool(n), [[] for _ in range(n)], [
        Cand([P("a0", cpu=600), P("a1", cpu=600)], 1, [0, -1], BATCHED, {0: CPU}, [(0, 1, (600, 0, 0))], first=1),
        Cand([P("b0", cpu=600)], OK, [0], NONE),
        Cand([], EMPTY, [], NONE),
        Cand([P("c0", cpu=600), P("c1", cpu=10)], FALLBACK, [-1, -1], NONE),
    ])


def dataclass_copy(pod: Pod, name: str) -> Pod:
    import dataclasses
    return dataclasses.replace(pod, name=name)


def _single():
    n = 63
    empty = [[] for _ in range(n)]
    yield PlanCase("port_against_port", pool(n), empty, [
        Cand([_hp("a0", 80), _hp("a1", 80)], 1, [7, -1], SINGLE, {7: PORTS}),
        Cand([_hp("b0", 81), _hp("b1", 80)], 1, [7, -1], SINGLE, {}),  # syntactic: any port against any port
        Cand([_hp("c0", 80)], 0, [-1], BATCHED, {}, []),               # no earlier pod: plain whatever it carries
    ])
    H = "kubernetes.io/hostname"
    nodes = pool(n)
    for i, nd in enumerate(nodes):
        nd.labels = {H: nd.name, "zone": "a" if i < 3 else "b"}
    web, db = {"app": "web"}, {"app": "db"}

    def lp(name, labels, anti=None, cpu=10):
        return Pod(name, namespace="default", labels=labels, containers=[Container(cpu_milli=cpu)],
                   pod_anti_affinity=anti)
    yield PlanCase("hostname_anti_affinity_both_ways", nodes, empty, [
        # the stop pod's own term meets the earlier pod
        Cand([lp("a0", db), lp("a1", web, [PodAffinityTerm(H, LabelSelector(db))])], 1, [4, -1], SINGLE,
             {4: INTER_POD}),
        # the earlier pod's term selects the stop pod
        Cand([lp("b0", db, [PodAffinityTerm(H, LabelSelector(web))]), lp("b1", web)], 1, [5, -1], SINGLE,
             {5: INTER_POD}),
    ])
    yield PlanCase("zone_term", nodes, empty, [
        Cand([lp("a0", db), lp("a1", web, [PodAffinityTerm("zone", LabelSelector(db))])], 1, [1, -1], SINGLE,
             {0: INTER_POD, 1: INTER_POD, 2: INTER_POD}),
    ])
    sp = Pod("a2", namespace="default", labels=web, containers=[Container(cpu_milli=10)],
             topology_spread=[TopologySpreadConstraint(1, "zone", label_selector=LabelSelector(web))])
    # zone a counts the two earlier pods, zone b none: 2 + 1 - 0 > maxSkew on zone a's nodes
    yield PlanCase("zone_spread_count", nodes, empty, [
        Cand([lp("a0", web), lp("a1", web), sp], 2, [0, 1, -1], SINGLE, {0: SPREAD, 1: SPREAD, 2: SPREAD}),
    ])
    G = "nvidia.com/gpu"

    def gpu(name, k):
        return Pod(name, containers=[Container(cpu_milli=10, scalar={G: k})])
    gnodes = pool(n)
    gnodes[9].scalar = {G: 1}
    gnodes[10].scalar = {G: 2}
    yield PlanCase("last_scalar_unit", gnodes, empty, [
        Cand([gpu("a0", 1), gpu("a1", 1)], 1, [9, -1], SINGLE, {j: SCALAR for j in range(n) if j != 10}),
        Cand([P("b0", cpu=995), gpu("b1", 1)], 1, [10, -1], BATCHED,
             {**{j: SCALAR for j in range(n) if j not in (9, 10)}, 10: CPU}, [(10, 1, (995, 0, 0))]),
    ])

    def disk(name, vol):
        return Pod(name, containers=[Container(cpu_milli=10)], volumes=[Volume(iscsi_iqn=vol)])
    yield PlanCase("inline_disk", pool(n), empty, [
        Cand([disk("a0", "iqn-1"), disk("a1", "iqn-1")], 1, [11, -1], SINGLE, {11: VOLUMES}),
    ], VolumeWorld())


def cases() -> List[PlanCase]:
    out = list(_plain()) + list(_single())
    names = [c.name for c in out]
    assert len(names) == len(set(names))
    return out


class Built:
    """A case as one cluster: the scenario, the candidate arrays, at_pod and node_of_pod."""

    def __init__(self, case: PlanCase):
        import numpy as np
        from helpers import Scenario
        self.case = case
        flat = [p for cd in case.cands for p in cd.pods]
        self.sc = Scenario(case.nodes, case.base, flat, volumes=case.world)
        self.cand_off = np.zeros(len(case.cands) + 1, np.int32)
        self.cand_off[1:] = np.cumsum([len(cd.pods) for cd in case.cands])
        self.cand_pods = np.array([self.sc.qidx(i) for i in range(len(flat))], np.int32)
        self.at_pod = np.array([cd.at_pod for cd in case.cands], np.int32)
        self.node_of_pod = np.array([x for cd in case.cands for x in cd.node_of_pod], np.int32)
        assert len(self.node_of_pod) == len(flat)
        self.n_spot = len(case.nodes)


RESOURCE_BITS = PODS | CPU | MEMORY | EPHEMERAL


def oracle_in_context(sc, osnap, pods, mapping, k, n_spot):
    """The oracle forked and filled the way canDrainNode fills it (pods[:k] at mapping[:k]): its yes / no for
    pods[k] on every node, and fitsRequest's PODS / CPU / MEMORY / EPHEMERAL bits [upstream k8s v1.19.2
    noderesources/fit.go] from its node state after the fill; reverted."""
    from oracle_lib import load_oracle
    ora = load_oracle()
    A = sc.enc.a
    pod = int(pods[k])
    req = (int(A["req_cpu"][pod]), int(A["req_mem"][pod]), int(A["req_eph"][pod]))
    lists_scalar = A["pod_scalar_off"][pod + 1] > A["pod_scalar_off"][pod]
    alloc = (A["alloc_cpu"], A["alloc_mem"], A["alloc_eph"])
    assert ora.oracle_snapshot_fork(osnap.h) == 0
    try:
        for q in range(k):
            ora.oracle_snapshot_add_pod(osnap.h, sc.ptr, int(pods[q]), int(mapping[q]))
        fits = [ora.oracle_check_predicates(osnap.h, sc.ptr, pod, j) for j in range(n_spot)]
        bits = []
        for j in range(n_spot):
            requested, num_pods = osnap.node_state(j)
            m = PODS if num_pods + 1 > int(A["alloc_pods"][j]) else 0
            if any(req) or lists_scalar:
                for d, bit in enumerate((CPU, MEMORY, EPHEMERAL)):
                    if int(alloc[d][j]) < req[d] + requested[d]:
                        m |= bit
            bits.append(m)
    finally:
        ora.oracle_snapshot_revert(osnap.h)
    return fits, bits


N_PORT_PODS = 70


def port_bits_case() -> PlanCase:
    """More distinct host ports among the stop pods of one call than the encoder's 64-bit state word has bits
    (one bit per port group of a call): the encode of the batch hands the pods past the 64th back
    as fallback although each is inside the encoded set on its own, so they are asked again alone (SINGLE,
    fallback 0).  A pod with a PVC is outside the set either way: fallback 1 whichever way it went.  The stop pod
    after a port-free pod stays in the batch.  `how` here is what the planner reports (the view agrees)."""
    n = 63
    base = [[] for _ in range(n)]
    base[5] = [_hp("web", 8003)]
    cands = [Cand([_hp("hp%d" % i, 8000 + i)], 0, [-1], BATCHED if i < 64 else SINGLE,
                  {5: PORTS} if i == 3 else {}, [] if i < 64 else None) for i in range(N_PORT_PODS)]
    cands.append(Cand([Pod("pvc", containers=[Container(cpu_milli=10)], has_pvc=True)], 0, [-1], SINGLE))
    cands.append(Cand([P("z0", cpu=301), P("z1", cpu=700)], 1, [62, -1], BATCHED, {62: CPU}, [(62, 1, (301, 0, 0))]))
    return PlanCase("port_bits_exhausted", pool(n), base, cands)


def sliced(b: "Built", first: int):
    """The candidates of `b` from `first` on as a slice of the same arrays: cand_pod_off[0] > 0, node_of_pod
    relative to it (the form sr_plan_out.node_of_pod has for a shard of a larger candidate list)."""
    lo = int(b.cand_off[first])
    return b.cand_off[first:].copy(), b.cand_pods, b.at_pod[first:].copy(), b.node_of_pod[lo:].copy()
