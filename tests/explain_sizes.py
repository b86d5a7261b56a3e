"""Inputs and hand-derived masks for sr_explain_pods / sr_explain_candidate
beyond one block: pools of 320, 1,100 and 4,300 spot nodes whose node j is built
from residues of j, so that the expected SR_WHY_* mask of every node is a
formula of j; query pods whose first feasible node lies in a late wave and
block; one call of 300 pods in as many classes, in another order than the
cluster's, fallback pods in between; and candidates whose earlier pods decide
the later pod's mask.

The formula pool.  Node j of a pool of n nodes refuses the full pod (`full_pod`)
for reason r iff j % MOD[r] == RES[r]; the moduli are pairwise coprime (4 * 5 for
the two labels of the affinity terms), so nodes refused by two and three groups
occur by construction.  The residues are chosen so that in all three pools every
reason occurs in the last live row word (nodes 256..319, 1088..1099 and
4288..4299) and alone on a node past word 0, and every row word holds a feasible
and a refused node.  The rule behind each term (k8s v1.19.2, as quoted in
tests/known_answer.py) stands beside it in `MOD_RES`.

tests/test_explain_sizes_reference.py proves every expectation on the CPU
oracle; tests/test_gpu_explain_sizes.py runs them through the C ABI."""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache
from typing import Dict, List, Optional

import numpy as np

from domain_cases import H, Z
from explain_cases import (CPU, EPHEMERAL, INTER_POD, MEMORY, NODE_AFFINITY, PODS, PORTS, SCALAR, SPREAD, TAINT,
                           UNSCHEDULABLE, VOLUMES)
from helpers import Scenario
from known_answer import N, P, used
from spotplanner.model import (Container, ContainerPort, GiB, LabelSelector, NodeSelectorRequirement, NodeSelectorTerm,
                               Pod, PodAffinityTerm, Taint, Toleration, TopologySpreadConstraint, Volume, VolumeWorld)

BITS = (UNSCHEDULABLE, TAINT, NODE_AFFINITY, PODS, CPU, MEMORY, EPHEMERAL, SCALAR, PORTS, INTER_POD, SPREAD, VOLUMES)
SIZES = (320, 1100, 4300)
G = "example.com/gpu"
KEY = Taint("k", "v", "NoSchedule")
CORDON = "node.kubernetes.io/unschedulable"
NODE_CPU, NODE_MEM, NODE_EPH = 4000, 8 * GiB, 10 * GiB
REQ_CPU, REQ_MEM, REQ_EPH = 500, 1 * GiB, 1 * GiB

# reason -> (modulus, residue): node j refuses the full pod for the reason iff j % modulus == residue
MOD_RES = {
    UNSCHEDULABLE: (11, 0),  # NodeUnschedulable: Spec.Unschedulable, and the pod does not tolerate the cordon taint
    TAINT: (7, 6),           # TaintToleration: a NoSchedule taint k=v the pod does not tolerate
    NODE_AFFINITY: (20, 9),  # NodeAffinity: no ORed term matches: j % 4 == 1 (label a=a1) and j % 5 == 4 (label b=b4)
    PODS: (13, 2),           # fitsRequest: len(Pods) + 1 > allowedPodNumber: pods=1 and one base pod
    CPU: (47, 12),           # fitsRequest: allocatable < request + requested: base pods leave 499m of the 500m
    MEMORY: (41, 31),        # the same, 1 GiB - 1 left
    EPHEMERAL: (17, 11),     # the same, 1 GiB - 1 left
    SCALAR: (3, 2),          # fitsRequest's ScalarResources loop: the node lacks the resource (even j) or a base pod
                             # holds its only unit (odd j)
    PORTS: (19, 16),         # NodePorts: a base pod holds host port 80 (0.0.0.0, TCP)
    INTER_POD: (23, 13),     # InterPodAffinity: the pod's hostname-key anti-affinity term selects a base pod app=db
    SPREAD: (29, 25),        # PodTopologySpread: hostname key, maxSkew 1: a matching base pod makes 1 + 1 - 0 > 1
                             # (on a node that passes the pod's node affinity: formula_mask)
    VOLUMES: (31, 13),       # VolumeRestrictions: a base pod mounts the same ISCSI volume read-write
}
AFF_A, AFF_B = MOD_RES[NODE_AFFINITY][1] % 4, MOD_RES[NODE_AFFINITY][1] % 5


def refuses(j: int, bit: int) -> bool:
    m, r = MOD_RES[bit]
    return j % m == r


def formula_mask(j: int, affinity: bool = True) -> int:
    """The full pod's mask on node j of any formula pool (`affinity` False: of the pod without its required node
    affinity).  One group reads another: PodTopologySpread's PreFilter makes pairs (key, value) only of the nodes
    that pass the pod's nodeSelector / required affinity (calPreFilterState), and Filter counts 0 for a node whose
    pair is missing: 0 + 1 - 0 <= maxSkew.  So a node NODE_AFFINITY refuses is never refused for SPREAD, whatever
    runs on it (nodes 489 + 580 k hold a web pod and fail the affinity)."""
    m = sum(bit for bit in BITS if refuses(j, bit))
    if not affinity:
        return m & ~NODE_AFFINITY
    return m & ~SPREAD if m & NODE_AFFINITY else m


def formula_masks(n: int, affinity: bool = True) -> np.ndarray:
    return np.array([formula_mask(j, affinity) for j in range(n)], np.uint16)


def overcommitted(j: int) -> bool:
    """In a pool built with `many`: every second CPU-refusing node requests 4001m of its 4000m, so a zero cpu
    request is refused there too (allocatable < 0 + requested) unless the whole request is zero."""
    m, r = MOD_RES[CPU]
    return j % m == r and (j // m) % 2 == 1


# ---- the full pod and the variants that leave one group out
def full_pod(name="full", **without) -> Pod:
    """The pod every reason can refuse.  `without` names the groups to leave out."""
    w = lambda k: without.get(k, False)  # noqa: E731
    c = Container(cpu_milli=0 if w("cpu") else REQ_CPU, memory=0 if w("memory") else REQ_MEM,
                  ephemeral=0 if w("ephemeral") else REQ_EPH, scalar={} if w("scalar") else {G: 1},
                  ports=[] if w("ports") else [ContainerPort(80)])
    others = ["a%d" % v for v in range(4) if v != AFF_A]
    terms = [NodeSelectorTerm([NodeSelectorRequirement("a", "In", others)]),
             NodeSelectorTerm([NodeSelectorRequirement("a", "In", ["a%d" % AFF_A]),
                               NodeSelectorRequirement("b", "NotIn", ["b%d" % AFF_B])])]
    tol = []
    if w("unschedulable"):
        tol.append(Toleration(CORDON, "Exists", "", "NoSchedule"))
    if w("taint"):
        tol.append(Toleration("k", "Equal", "v", "NoSchedule"))
    return Pod(name, labels={"app": "web"}, containers=[c], tolerations=tol,
               required_node_affinity=None if w("node_affinity") else terms,
               pod_anti_affinity=None if w("inter_pod") else [PodAffinityTerm(H, LabelSelector({"app": "db"}))],
               topology_spread=[] if w("spread") else [
                   TopologySpreadConstraint(1, H, label_selector=LabelSelector({"app": "web"}))],
               volumes=[] if w("volumes") else [Volume(iscsi_iqn="iqn-1")])


# reason -> the group `full_pod` leaves out; PODS is no field of the pod: its variant is the pool with pods=110 on
# every node (`build(n, roomy=True)`) and the full pod
LEAVE_OUT = {UNSCHEDULABLE: "unschedulable", TAINT: "taint", NODE_AFFINITY: "node_affinity", CPU: "cpu",
             MEMORY: "memory", EPHEMERAL: "ephemeral", SCALAR: "scalar", PORTS: "ports", INTER_POD: "inter_pod",
             SPREAD: "spread", VOLUMES: "volumes"}

# ---- the first feasible node in a late wave and block: key f<s> is carried by the nodes of set s only
FIRST_SETS = [lambda n: [63], lambda n: [64], lambda n: [255], lambda n: [256], lambda n: [n - 1],
              lambda n: [191, n - 1], lambda n: [256, 257, 320], lambda n: []]
FIRST_NAMES = ["63", "64", "255", "256", "last", "191_last", "256_257_320", "none"]


def first_want(n: int):
    """(first, feasible) of every set, written out: the earliest node of the set, and its size."""
    return [(63, 1), (64, 1), (255, 1), (256, 1), (n - 1, 1), (191, 2), (256, 3), (-1, 0)]


def first_pod(s: int) -> Pod:
    """Zero requests, tolerates everything, selects label f<s>: refused off the set for NODE_AFFINITY, and on a
    full node (PODS), which no node of a set is."""
    return Pod("first-%s" % FIRST_NAMES[s], containers=[Container()], tolerations=[Toleration("", "Exists")],
               node_selector={"f%d" % s: "y"})


def first_mask(n: int, s: int, j: int) -> int:
    return (0 if j in FIRST_SETS[s](n) else NODE_AFFINITY) | (PODS if refuses(j, PODS) else 0)


# ---- many pods in one call (the 1,100 pool built with `many`)
MANY_N, MANY = 1100, 300
MANY_ORDER = [(k * 101 + 17) % MANY for k in range(MANY)]  # caller entry k is pod MANY_ORDER[k]


OVER = [59 + 94 * t for t in range(12)]  # the over-committed nodes of the pool: overcommitted(j)


def many_node(i: int) -> int:
    """The one node carrying pod i's label value own=v<i>.  Six zero-request pods (i = 4, 15, .. 59) and six pods
    asking for memory alone (i = 1, 34, .. 166) select an over-committed node, so that the selector does not hide
    what fitsRequest answers there; every other pod's node is spread by 37 i + 3, which meets none of those."""
    if i % 11 == 4 and i < 66:
        return OVER[i // 11]
    if i % 33 == 1 and i < 198:
        return OVER[6 + i // 33]
    return (i * 37 + 3) % MANY_N


def many_fallback(i: int) -> bool:
    return i % 7 == 6


def many_zero(i: int) -> bool:
    return i % 11 == 4


def many_pod(i: int) -> Pod:
    """Pod i: a selector of its own (a class of its own); requests by i % 3 (cpu / memory / all three), all zero
    for i % 11 == 4; host port 80 for i % 4 == 1; the taint tolerated for i % 5 == 0; has_pvc for i % 7 == 6."""
    if many_zero(i):
        c = Container()
    else:
        kind = i % 3
        c = Container(cpu_milli=REQ_CPU if kind != 1 else 0, memory=REQ_MEM if kind != 0 else 0,
                      ephemeral=REQ_EPH if kind == 2 else 0)
    if i % 4 == 1:
        c.ports = [ContainerPort(80)]
    return Pod("many-%d" % i, containers=[c], node_selector={"own": "v%d" % i},
               tolerations=[Toleration("k", "Equal", "v", "NoSchedule")] if i % 5 == 0 else [],
               has_pvc=many_fallback(i))


def many_mask(i: int, j: int) -> int:
    """Pod i on node j of the `many` pool (a fallback pod's row is zero: nothing is evaluated)."""
    if many_fallback(i):
        return 0
    m = 0 if j == many_node(i) else NODE_AFFINITY   # the selector: one node carries own=v<i>
    m |= UNSCHEDULABLE if refuses(j, UNSCHEDULABLE) else 0
    m |= TAINT if refuses(j, TAINT) and i % 5 != 0 else 0
    m |= PODS if refuses(j, PODS) else 0             # before the zero-request shortcut
    m |= PORTS if refuses(j, PORTS) and i % 4 == 1 else 0
    if many_zero(i):
        return m                                     # fitsRequest returns after the pod count
    kind = i % 3
    # allocatable < request + requested: 499m are left (a 500m request fails), or the node is over-committed
    # (every request fails, a zero one too)
    if refuses(j, CPU) and (kind != 1 or overcommitted(j)):
        m |= CPU
    if refuses(j, MEMORY) and kind != 0:
        m |= MEMORY
    if refuses(j, EPHEMERAL) and kind == 2:
        m |= EPHEMERAL
    return m


def many_masks() -> np.ndarray:
    """[entry of the call][node], in the caller's order."""
    return np.array([[many_mask(i, j) for j in range(MANY_N)] for i in MANY_ORDER], np.uint16)


# ---- building a pool
def _z(name, **kw) -> Pod:
    """A base pod of zero requests: it leaves the resource arithmetic of its node alone."""
    return Pod(name, containers=[Container()], **kw)


@dataclass
class Pool:
    n: int
    sc: Scenario
    full: int                       # query indices (Scenario.qidx)
    variants: Dict[int, int]
    firsts: List[int]
    many: List[int] = field(default_factory=list)
    extra: List[int] = field(default_factory=list)


def build(n: int, roomy: bool = False, many: bool = False, variants: bool = True, extra=()) -> Pool:
    """`extra`: further query pods, after all others (explain_plan_sizes.py: the pods of its candidates); the
    nodes, the base pods and the indices of every other query pod come out as without them."""
    nodes, base = [], []
    for j in range(n):
        labels = {H: "s%d" % j, "a": "a%d" % (j % 4), "b": "b%d" % (j % 5)}
        for s, members in enumerate(FIRST_SETS):
            if j in members(n):
                labels["f%d" % s] = "y"
        on = []
        scalar = {G: 1}
        if refuses(j, PODS):
            on.append(_z("filler-%d" % j))
        if refuses(j, CPU):
            over = many and overcommitted(j)
            on.append(used(cpu=NODE_CPU + 1 if over else NODE_CPU - REQ_CPU + 1, name="cpu-%d" % j))
        if refuses(j, MEMORY):
            on.append(used(mem=NODE_MEM - REQ_MEM + 1, name="mem-%d" % j))
        if refuses(j, EPHEMERAL):
            on.append(used(eph=NODE_EPH - REQ_EPH + 1, name="eph-%d" % j))
        if refuses(j, SCALAR):
            if j % 2 == 0:
                scalar = {}
            else:
                on.append(Pod("gpu-%d" % j, containers=[Container(cpu_milli=10, scalar={G: 1})]))
        if refuses(j, PORTS):
            on.append(_z("port-%d" % j))
            on[-1].containers[0].ports = [ContainerPort(80)]
        if refuses(j, INTER_POD):
            on.append(_z("db-%d" % j, labels={"app": "db"}))
        if refuses(j, SPREAD):
            on.append(_z("web-%d" % j, labels={"app": "web"}))
        if refuses(j, VOLUMES):
            on.append(_z("disk-%d" % j, volumes=[Volume(iscsi_iqn="iqn-1")]))
        nodes.append(N("s%d" % j, cpu=NODE_CPU, mem=NODE_MEM, eph=NODE_EPH,
                       pods=1 if refuses(j, PODS) and not roomy else 110, labels=labels, scalar=scalar,
                       taints=[KEY] if refuses(j, TAINT) else [], unschedulable=refuses(j, UNSCHEDULABLE)))
        base.append(on)
    if many:
        assert n == MANY_N
        for i in range(MANY):
            nodes[many_node(i)].labels["own"] = "v%d" % i
    query = [full_pod()]
    vq = {}
    if variants:
        for bit, group in LEAVE_OUT.items():
            vq[bit] = len(query)
            query.append(full_pod("without-" + group, **{group: True}))
    f0 = len(query)
    query += [first_pod(s) for s in range(len(FIRST_SETS))]
    m0 = len(query)
    if many:
        query += [many_pod(i) for i in range(MANY)]
    x0 = len(query)
    query += list(extra)
    sc = Scenario(nodes, base, query, volumes=VolumeWorld())
    return Pool(n, sc, sc.qidx(0), {bit: sc.qidx(q) for bit, q in vq.items()},
                [sc.qidx(f0 + s) for s in range(len(FIRST_SETS))],
                [sc.qidx(m0 + i) for i in range(MANY)] if many else [],
                [sc.qidx(x0 + i) for i in range(len(extra))])


@lru_cache(maxsize=None)
def get_pool(n: int, roomy: bool = False, many: bool = False) -> Pool:
    return build(n, roomy, many, variants=not many)


# ---- the row-word edge pool of test_gpu_explain.test_row_word_and_block_edges
def edge_pool(n: int = 65):
    """n - 1 open nodes, then one with a taint and 50m free: (scenario, masks of a 100m pod, masks of a 0m pod)."""
    nodes = [N("n%d" % i, cpu=1000) for i in range(n - 1)] + [N("last", cpu=1000, taints=[KEY])]
    base = [[] for _ in range(n - 1)] + [[used(cpu=950)]]
    sc = Scenario(nodes, base, [P(cpu=100), P(cpu=0)])
    return sc, [0] * (n - 1) + [TAINT | CPU], [0] * (n - 1) + [TAINT]


# ---- the gridDim.y split of launch_explain: 65,537 entries cycling through three pods on three nodes
SPLIT_ENTRIES = 65537
SPLIT_MASKS = [[CPU, TAINT, 0], [0, TAINT, 0], [CPU, 0, 0]]  # pod 0: 100m; pod 1: 0m; pod 2: 100m, tolerates the taint


def split_pool():
    nodes = [N("a", cpu=1000), N("b", cpu=1000, taints=[KEY]), N("c", cpu=1000)]
    base = [[used(cpu=950)], [], []]
    pods = [P("p0", cpu=100), P("p1", cpu=0),
            P("p2", cpu=100, tolerations=[Toleration("k", "Equal", "v", "NoSchedule")])]
    return Scenario(nodes, base, pods)


# ---- sr_explain_candidate: an earlier pod of the candidate decides the later pod's mask
@dataclass
class CandCase:
    name: str
    rule: str
    nodes: list
    base: list
    pods: List[Pod]          # the candidate; the last pod is the one explained
    mapping: List[int]       # the node of every earlier pod
    without: List[int]       # the last pod's masks against the snapshot as it is
    with_: List[int]         # ... with the earlier pods added
    world: Optional[VolumeWorld] = None
    flips_to_yes: bool = False  # the earlier pod admits the later one (required affinity) instead of refusing it


def _hn(name, zone=None, **kw):
    labels = {H: name}
    if zone:
        labels[Z] = zone
    return N(name, labels=labels, **kw)


def _lp(name, app=None, **kw) -> Pod:
    return Pod(name, labels={"app": app} if app else {}, containers=[Container(cpu_milli=10)], **kw)


def _port(name) -> Pod:
    return Pod(name, containers=[Container(cpu_milli=10, ports=[ContainerPort(80)])])


def cand_cases() -> List[CandCase]:
    out = []
    sel = lambda app: LabelSelector({"app": app})  # noqa: E731
    three = lambda: [_hn("a"), _hn("b"), _hn("c")]  # noqa: E731
    zoned = lambda: [_hn("a", "a"), _hn("b", "a"), _hn("c", "b"), _hn("d")]  # noqa: E731
    out.append(CandCase(
        "ports", "HostPortInfo.CheckConflict: the earlier pod holds 0.0.0.0:80/TCP on b",
        three(), [[], [], []], [_port("e"), _port("l")], [1], [0, 0, 0], [0, PORTS, 0]))
    out.append(CandCase(
        "anti_hostname_earlier_selects_later",
        "satisfyExistingPodsAntiAffinity: the earlier pod's hostname term selects the later pod: its node c is refused",
        three(), [[], [], []],
        [_lp("e", "x", pod_anti_affinity=[PodAffinityTerm(H, sel("web"))]), _lp("l", "web")], [2],
        [0, 0, 0], [0, 0, INTER_POD]))
    out.append(CandCase(
        "anti_hostname_later_selects_earlier",
        "satisfyPodAntiAffinity: the later pod's hostname term selects the earlier pod on a",
        three(), [[], [], []],
        [_lp("e", "db"), _lp("l", "web", pod_anti_affinity=[PodAffinityTerm(H, sel("db"))])], [0],
        [0, 0, 0], [INTER_POD, 0, 0]))
    out.append(CandCase(
        "anti_zone_refuses_the_zone",
        "satisfyPodAntiAffinity: a zone term refuses every node sharing the zone of the earlier pod's node b; a node "
        "without the key is never refused",
        zoned(), [[], [], [], []],
        [_lp("e", "db"), _lp("l", "web", pod_anti_affinity=[PodAffinityTerm(Z, sel("db"))])], [1],
        [0, 0, 0, 0], [INTER_POD, INTER_POD, 0, 0]))
    web = TopologySpreadConstraint(1, Z, label_selector=sel("web"))
    # zones a and b count one web pod each: 1 + 1 - 1 <= 1 everywhere.  The earlier web pod on b (zone a) makes
    # a count 2: 2 + 1 - 1 > 1 on a's nodes, 1 + 1 - 1 <= 1 on b's
    out.append(CandCase(
        "spread_zone_count_past_max_skew", "PodTopologySpread: matchNum + 1 - minMatchNum > maxSkew",
        [_hn("a", "a"), _hn("b", "a"), _hn("c", "b"), _hn("d", "b")], [[_lp("w1", "web")], [], [_lp("w2", "web")], []],
        [_lp("e", "web"), _lp("l", "web", topology_spread=[web])], [1], [0, 0, 0, 0], [SPREAD, SPREAD, 0, 0]))

    def gpu(name):
        return Pod(name, containers=[Container(cpu_milli=10, scalar={G: 1})])
    out.append(CandCase(
        "scalar_last_unit", "fitsRequest, ScalarResources: the earlier pod takes a's only unit; c has none",
        [N("a", scalar={G: 1}), N("b", scalar={G: 2}), N("c")], [[], [gpu("u")], []], [gpu("e"), gpu("l")], [0],
        [0, 0, SCALAR], [SCALAR, 0, SCALAR]))

    def disk(name):
        return Pod(name, containers=[Container(cpu_milli=10)], volumes=[Volume(iscsi_iqn="iqn-1")])
    out.append(CandCase(
        "volumes_same_inline_disk", "VolumeRestrictions: two read-write mounts of one ISCSI volume conflict",
        three(), [[], [], []], [disk("e"), disk("l")], [1], [0, 0, 0], [0, VOLUMES, 0], VolumeWorld()))
    out.append(CandCase(
        "pods_three_pod_candidate", "fitsRequest: len(Pods) + 1 > allowedPodNumber: the earlier pods fill a (pods=1) "
        "and b (pods=2, one base pod)",
        [N("a", pods=1), N("b", pods=2), N("c")], [[], [used(name="u")], []], [_lp("e0"), _lp("e1"), _lp("l")], [0, 1],
        [0, 0, 0], [PODS, PODS, 0]))
    # no cache pod runs and the later pod does not match its own term: no node satisfies the affinity.  The
    # earlier cache pod on b satisfies it in zone a; c's zone holds none, d lacks the key
    out.append(CandCase(
        "affinity_only_the_earlier_pod_satisfies", "satisfyPodAffinity: a pod matching the term must run in the node's "
        "zone; a node without the key fails",
        zoned(), [[], [], [], []],
        [_lp("e", "cache"), _lp("l", "web", pod_affinity=[PodAffinityTerm(Z, sel("cache"))])], [1],
        [INTER_POD] * 4, [0, 0, INTER_POD, INTER_POD], flips_to_yes=True))
    # 130 nodes: the earlier pods sit on nodes 128 and 129, row word 2
    wide = [_hn("w%d" % j) for j in range(130)]
    out.append(CandCase(
        "wide_ports_and_anti_in_word_2", "the port holder on node 128, the db pod on node 129",
        wide, [[] for _ in wide],
        [_port("e0"), _lp("e1", "db"),
         Pod("l", labels={"app": "web"}, containers=[Container(cpu_milli=10, ports=[ContainerPort(80)])],
             pod_anti_affinity=[PodAffinityTerm(H, sel("db"))])], [128, 129],
        [0] * 130, [0] * 128 + [PORTS, INTER_POD]))
    for c in out:
        assert len(c.nodes) == len(c.base) == len(c.without) == len(c.with_) and len(c.mapping) == len(c.pods) - 1
        assert len(c.nodes) <= 8 or c.name.startswith("wide")
    return out


def cand_scenario(case: CandCase) -> Scenario:
    return Scenario(case.nodes, case.base, case.pods, volumes=case.world)
