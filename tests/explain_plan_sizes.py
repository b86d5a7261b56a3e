"""Inputs and rule-derived masks for sr_explain_plan beyond one block: the
formula pools of explain_sizes.py (320, 1,100 and 4,300 nodes) with contexts on
a residue class of nodes; runs of equal pods that move the first feasible node
into a late wave and block; the 300 one-class pods of the `many` pool, each
after an earlier pod on the one node its selector admits; 65,537 candidates
across the gridDim.y split of launch_explain_plan; and small pools at the
limits of the plain-context rule (explain_plan.hpp).

Every expectation is the rule applied to the input, never a result of the code
under test.  A candidate's earlier pods change, for its stop pod, the touched
nodes' fitsRequest answer and nothing else (the stop pods here carry nothing an
earlier pod can meet): `in_context` takes the stop pod's masks against the base
snapshot (the formulas of explain_sizes.py, or hand rows) and replaces PODS /
CPU / MEMORY / EPHEMERAL on every touched node by `fits_request`, which reads
the node, its base pods and the earlier pods from the scenario's own objects
[upstream k8s v1.19.2 noderesources/fit.go fitsRequest]:
    PODS   iff len(Pods) + 1 > allowedPodNumber
    nothing further for a request of all zeros that lists no scalar resource
    bit d  iff allocatable_d < request_d + Requested_d, a zero request_d included
with Pods and Requested after the earlier pods were added.

tests/test_explain_plan_sizes_reference.py proves every input on the CPU (the
host view and the oracle); tests/test_gpu_explain_plan_sizes.py sends them
through the C ABI."""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache
from typing import Dict, List, Optional, Tuple

import numpy as np

import explain_plan_cases as C
import explain_sizes as X
from explain_cases import CPU, EPHEMERAL, INTER_POD, MEMORY, NODE_AFFINITY, PODS, SPREAD, TAINT
from explain_plan_cases import BATCHED, NONE, SINGLE, Cand, PlanCase
from helpers import Scenario
from known_answer import P, used
from spotplanner.model import Container, GiB, NodeSelectorTerm, Pod, Toleration

RESOURCE_BITS = PODS | CPU | MEMORY | EPHEMERAL
DIM_BITS = (CPU, MEMORY, EPHEMERAL)


# ---- the rule
def pod_request(pod: Pod) -> Tuple[int, int, int]:
    """What the pods of this file ask for and account: the sum of their containers (none has an init container or
    an overhead, so the fit request and the accounting agree)."""
    assert not pod.init_containers and pod.overhead is None
    return (sum(c.cpu_milli for c in pod.containers), sum(c.memory for c in pod.containers),
            sum(c.ephemeral for c in pod.containers))


def fits_request(node, base_pods, earlier, stop: Pod) -> int:
    """fitsRequest's bits for `stop` on `node` holding base_pods + earlier (module docstring)."""
    on = list(base_pods) + list(earlier)
    m = PODS if len(on) + 1 > node.pods else 0
    req = pod_request(stop)
    if not any(req) and not any(c.scalar for c in stop.containers):
        return m
    alloc = (node.cpu_milli, node.memory, node.ephemeral)
    for d, bit in enumerate(DIM_BITS):
        if alloc[d] < req[d] + sum(pod_request(p)[d] for p in on):
            m |= bit
    return m


def in_context(sc: Scenario, static, stop: Pod, placed: Dict[int, List[Pod]]) -> np.ndarray:
    """The stop pod's row after `placed` ({node: earlier pods}): `static` off the touched nodes, and on them with
    the four fitsRequest bits as the rule gives them."""
    row = np.array(static, np.uint16)
    for j, earlier in placed.items():
        row[j] = (int(row[j]) & ~RESOURCE_BITS) | fits_request(sc.nodes[j], sc.spot_pods[j], earlier, stop)
    return row


def context_list(placed: Dict[int, List[Pod]]) -> list:
    """The context list plan_queries must make of `placed`: sorted by node, one entry per node, the pods counted
    and their accounting summed."""
    return [(j, len(ps), tuple(sum(pod_request(p)[d] for p in ps) for d in range(3)))
            for j, ps in sorted(placed.items()) if ps]


# ---- an input of one call
@dataclass
class Ask:
    """One candidate: its pods as query indices of the scenario's extra pods (earlier pods, then the stop pod),
    the nodes of the earlier pods, and whether it is asked (at_pod = its last pod) or passed through (at_pod -1)."""
    name: str
    pods: List[int]
    nodes: List[int]
    asked: bool = True


@dataclass
class Input:
    name: str
    sc: Scenario
    cand_off: np.ndarray
    cand_pods: np.ndarray
    at_pod: np.ndarray
    node_of_pod: np.ndarray
    n_spot: int
    names: List[str]
    how: List[int]
    fallback: List[int]                  # what sr_explain_plan reports (a PVC pod: 1)
    want: np.ndarray                     # [candidate][node]; zeros where nothing is evaluated
    ctx: List[Optional[list]]            # the context list of every BATCHED candidate (None: not batched)
    hand: Dict[int, Tuple[int, int]] = field(default_factory=dict)   # candidate -> (first, feasible) by hand
    loop: List[int] = field(default_factory=list)   # candidates the GPU test also asks sr_explain_candidate for

    @property
    def n(self) -> int:
        return len(self.names)

    def evaluated(self, c: int) -> bool:
        return self.how[c] != NONE and not self.fallback[c]

    def sums(self):
        """(counts [n][12], feasible [n], first [n]) as they follow from `want`; -1 / -1 and zeros where nothing
        is evaluated."""
        from spotplanner import capi
        want = self.want
        ev = np.array([self.evaluated(c) for c in range(self.n)], bool)
        counts = np.stack([((want >> r) & 1).sum(1) for r in range(capi.SR_WHY_COUNT)], 1).astype(np.int32)
        ok = want == 0
        feasible = np.where(ev, ok.sum(1), -1)
        first = np.where(ev & ok.any(1), ok.argmax(1), -1)
        return counts, feasible, first


def assemble(name, sc: Scenario, qidx, asks: List[Ask], want, how, fallback, ctx, hand=None, loop=()) -> Input:
    """`qidx`: index in the scenario's query list -> cluster pod index."""
    off = np.zeros(len(asks) + 1, np.int32)
    off[1:] = np.cumsum([len(a.pods) for a in asks])
    pods = np.array([qidx(q) for a in asks for q in a.pods], np.int32)
    at = np.array([len(a.pods) - 1 if a.asked else -1 for a in asks], np.int32)
    mapping = np.array([x for a in asks for x in list(a.nodes) + [-1]], np.int32)
    assert len(mapping) == len(pods) and all(len(a.nodes) == len(a.pods) - 1 for a in asks)
    want = np.asarray(want, np.uint16)
    assert want.shape == (len(asks), len(sc.nodes)) and len(how) == len(fallback) == len(ctx) == len(asks)
    return Input(name, sc, off, pods, at, mapping, len(sc.nodes), [a.name for a in asks], list(how), list(fallback),
                 want, list(ctx), dict(hand or {}), list(loop))


# ---- 1. the formula pools in context
SIZES = X.SIZES
CLASS_MOD = 37   # coprime to every modulus of X.MOD_RES: a class meets every reason's nodes, and every row word
# candidate -> the residue of its touched nodes.  1088 % 37 == 15 and 4288 % 37 == 33: residues 15 .. 26 lie in the
# last live word of the 1,100 pool, 33 .. 36 and 0 .. 7 in that of the 4,300 pool, every residue in 256 .. 319
CLASS_RES = {"cpu_one_short": 15, "cpu_exact": 33, "memory": 20, "ephemeral": 36, "all_three": 5}
FORMULA_NAMES = ["cpu_one_short", "cpu_exact", "memory", "ephemeral", "all_three", "pod_count", "empty"]


def stop_pod() -> Pod:
    """The full pod without the two groups an earlier pod could meet: its anti-affinity term and its spread
    constraint.  Its host port, scalar resource and inline disk meet nothing of the plain earlier pods."""
    return X.full_pod("stop", inter_pod=True, spread=True)


def stop_static(n: int) -> np.ndarray:
    """The stop pod against the base snapshot: the formula without INTER_POD and SPREAD (SPREAD gone, nothing
    reads NODE_AFFINITY any more: X.formula_mask)."""
    return np.array([sum(bit for bit in X.BITS if bit not in (INTER_POD, SPREAD) and X.refuses(j, bit))
                     for j in range(n)], np.uint16)


def class_nodes(n: int, name: str) -> List[int]:
    return [j for j in range(n) if j % CLASS_MOD == CLASS_RES[name]]


def base_cpu(j: int) -> int:
    """Requested cpu of node j of a formula pool (not `many`): X.build's cpu-<j> and gpu-<j> pods."""
    return (X.NODE_CPU - X.REQ_CPU + 1 if X.refuses(j, CPU) else 0) + (10 if X.refuses(j, X.SCALAR) and j % 2 else 0)


def count_nodes(n: int) -> Tuple[int, int]:
    """The two last nodes no reason refuses (no base pod, 110 pod slots): the pod-count candidate puts 110 pods
    on the later one (110 + 1 > 110) and 109 on the earlier one (109 + 1 <= 110)."""
    free = [j for j in range(n) if not any(X.refuses(j, bit) for bit in X.BITS)]
    return free[-1], free[-2]


@lru_cache(maxsize=None)
def formula_input(n: int) -> Input:
    extra: List[Pod] = [stop_pod()]
    STOP = 0

    def add(pod):
        extra.append(pod)
        return len(extra) - 1
    mem = add(P("ctx-mem", cpu=1, mem=X.NODE_MEM - X.REQ_MEM + 1))
    eph = add(P("ctx-eph", cpu=1, eph=X.NODE_EPH - X.REQ_EPH + 1))
    all3 = add(P("ctx-all", cpu=X.NODE_CPU - X.REQ_CPU + 1, mem=X.NODE_MEM - X.REQ_MEM + 1,
                 eph=X.NODE_EPH - X.REQ_EPH + 1))
    tiny = add(P("ctx-tiny", cpu=1))
    asks = []
    # a pod of its own for every node: what the node has left after it is the request less one milli (a new CPU
    # bit wherever the node had room), or exactly the request (no new bit anywhere)
    for name, left in (("cpu_one_short", X.REQ_CPU - 1), ("cpu_exact", X.REQ_CPU)):
        nodes = class_nodes(n, name)
        own = [add(P("%s-%d" % (name, j), cpu=max(0, X.NODE_CPU - base_cpu(j) - left))) for j in nodes]
        asks.append(Ask(name, own + [STOP], nodes))
    # one cluster pod repeated on every node of the class
    for name, q in (("memory", mem), ("ephemeral", eph), ("all_three", all3)):
        nodes = class_nodes(n, name)
        asks.append(Ask(name, [q] * len(nodes) + [STOP], nodes))
    full, room = count_nodes(n)
    # 110 pods on `full` and 109 on `room`, in turns: two merged entries
    asks.append(Ask("pod_count", [tiny] * 219 + [STOP], [full if i % 2 == 0 else room for i in range(219)]))
    asks.append(Ask("empty", [STOP], []))
    assert [a.name for a in asks] == FORMULA_NAMES
    pool = X.build(n, variants=False, extra=extra)
    sc = pool.sc
    static = stop_static(n)
    placed = [placed_of(sc, a, extra) for a in asks]
    want = [in_context(sc, static, extra[STOP], pl) for pl in placed]
    return assemble("formula_%d" % n, sc, lambda q: pool.extra[q], asks, want, [BATCHED] * len(asks), [0] * len(asks),
                    [context_list(pl) for pl in placed], loop=list(range(len(asks))))


def placed_of(sc, ask: Ask, pods: List[Pod]) -> Dict[int, List[Pod]]:
    out: Dict[int, List[Pod]] = {}
    for q, j in zip(ask.pods, ask.nodes):
        out.setdefault(j, []).append(pods[q])
    return out


# ---- 2. the first feasible node decided by the context
RUN_SIZES = (1100, 4300)


def run_lengths(n: int) -> List[int]:
    """k earlier pods on nodes 0 .. k-1: the first feasible node is k, in wave 0 / 1 / 3 of block 0, in block 1, on
    the first node of the last row word, on the last node, nowhere."""
    return [63, 64, 255, 256, (n - 1) // 64 * 64, n - 1, n]


HOLE = 191   # the run 0 .. 255 without this node


@lru_cache(maxsize=None)
def runs_input(n: int) -> Input:
    """A 1000m pool; 600m pods: a node holding one refuses the next (1000 < 600 + 600)."""
    nodes = C.pool(n)
    query = [P("run", cpu=600)] + [P("stop-%d" % k, cpu=600) for k in run_lengths(n)] + [P("stop-hole", cpu=600)]
    sc = Scenario(nodes, [[] for _ in range(n)], query)
    asks, want, hand = [], [], {}
    for i, k in enumerate(run_lengths(n)):
        asks.append(Ask("run_%d" % k, [0] * k + [1 + i], list(range(k))))
        want.append([CPU] * k + [0] * (n - k))
        hand[i] = (k, n - k) if k < n else (-1, 0)
    on = [j for j in range(256) if j != HOLE]
    asks.append(Ask("hole", [0] * len(on) + [len(query) - 1], on))
    want.append([0 if j == HOLE or j >= 256 else CPU for j in range(n)])
    hand[len(asks) - 1] = (HOLE, n - 255)
    ctx = [[(j, 1, (600, 0, 0)) for j in a.nodes] for a in asks]
    return assemble("runs_%d" % n, sc, sc.qidx, asks, want, [BATCHED] * len(asks), [0] * len(asks), ctx, hand)


# ---- 3. many classes in the caller's order, a context of its own each
# the earlier pod of candidate k (pod i = MANY_ORDER[k]) is EARLIER[i // 3 % 3], on many_node(i): each asks in all
# three dimensions and takes more than a whole node in one, so that the node refuses that dimension whatever the
# stop pod asks in it -- zero too -- unless the stop pod asks nothing at all
def many_earlier() -> List[Pod]:
    return [P("over-cpu", cpu=X.NODE_CPU + 1, mem=1, eph=1), P("over-mem", cpu=1, mem=X.NODE_MEM + 1, eph=1),
            P("over-eph", cpu=1, mem=1, eph=X.NODE_EPH + 1)]


def many_over(i: int) -> int:
    return i // 3 % 3


@lru_cache(maxsize=None)
def many_input() -> Input:
    earlier = many_earlier()
    pool = X.build(X.MANY_N, many=True, variants=False, extra=earlier)
    sc = pool.sc
    q0 = pool.many[0] - sc.q0     # query index of many_pod(0); the extra pods follow the 300
    e0 = pool.extra[0] - sc.q0
    asks, want, how, fallback, ctx = [], [], [], [], []
    for i in X.MANY_ORDER:
        e, j = many_over(i), X.many_node(i)
        asks.append(Ask("many-%d" % i, [e0 + e, q0 + i], [j]))
        placed = {j: [earlier[e]]}
        if X.many_fallback(i):   # a PVC pod: handed back by the batched encode, asked again alone, outside the set
            want.append(np.zeros(X.MANY_N, np.uint16))
            how.append(SINGLE)
            fallback.append(1)
            ctx.append(None)
        else:
            static = [X.many_mask(i, jj) for jj in range(X.MANY_N)]
            want.append(in_context(sc, static, sc.query[q0 + i], placed))
            how.append(BATCHED)
            fallback.append(0)
            ctx.append(context_list(placed))
    return assemble("many", sc, sc.qidx, asks, want, how, fallback, ctx, loop=list(range(X.MANY)))


# ---- 4. the gridDim.y split: 65,537 queries, the second launch starts at query 65,535
# Candidate k stops at pod STOP_CYCLE[k % 4] of X.split_pool in context CTX_CYCLE[k % 7].  A context is "none"
# (the stop pod alone), "skip" (two pods, at_pod -1: not asked) or the node the one earlier pod (950m) is put on;
# node 0 refuses 100m already, so a context there changes nothing and stands in the cycle as a guard.  A candidate
# that is not asked takes no query: 76,460 candidates make the 65,537 queries of X.SPLIT_ENTRIES, and queries
# 65,534 / 65,535 / 65,536 are candidates 76,456 / 76,457 / 76,459 (a skipped one between the last two: the
# result slot is not the query index).  Any three neighbours of a cycle of period 3 hold the zero-request pod p1,
# whose row no single earlier pod changes on a node of 110 slots; so the stop pods cycle with period 4, p2 twice:
# those three candidates (k % 4 == 0, 1, 3; k % 7 == 2, 3, 5) are p2 after node 1, p0 after node 2, p2 after node 2.
SPLIT_QUERIES = X.SPLIT_ENTRIES
SPLIT_N = 76460
STOP_CYCLE = (2, 0, 1, 2)
CTX_CYCLE = (0, "none", 1, 2, "skip", 2, 1)
SPLIT_EARLIER_CPU = 950
SPLIT_HAND = {76456: ([CPU, CPU, 0], 2, 1),        # p2 tolerates b's taint; the earlier pod leaves b 50m
              76457: ([CPU, TAINT, CPU], -1, 0),   # p0: a has 50m, b the taint, c 50m after the earlier pod
              76459: ([CPU, 0, CPU], 1, 1)}        # p2 after the earlier pod on c: (row, first, feasible)


def split_kind(k: int):
    return STOP_CYCLE[k % 4], CTX_CYCLE[k % 7]


@lru_cache(maxsize=None)
def split_input() -> Input:
    base = X.split_pool()
    earlier = P("e", cpu=SPLIT_EARLIER_CPU)
    sc = Scenario(base.nodes, base.spot_pods, base.query + [earlier])
    E = 3
    rows, lists = {}, {}
    for k in range(28):   # every (stop pod, context) of the two cycles, by the rule
        p, where = split_kind(k)
        placed = {where: [earlier]} if isinstance(where, int) else {}
        rows[p, where] = (np.zeros(3, np.uint16) if where == "skip"
                          else in_context(sc, X.SPLIT_MASKS[p], sc.query[p], placed))
        lists[p, where] = None if where == "skip" else context_list(placed)
    asks, want, how, ctx = [], [], [], []
    for k in range(SPLIT_N):
        p, where = split_kind(k)
        if where == "none":
            asks.append(Ask("", [p], []))
        else:
            asks.append(Ask("", [E, p], [0 if where == "skip" else where], asked=where != "skip"))
        want.append(rows[p, where])
        how.append(NONE if where == "skip" else BATCHED)
        ctx.append(lists[p, where])
    hand = {k: (first, feasible) for k, (_, first, feasible) in SPLIT_HAND.items()}
    return assemble("split", sc, sc.qidx, asks, np.stack(want), how, [0] * SPLIT_N, ctx, hand)


# ---- 6. the limits of the rule: small pools, hand masks
Q62 = 1 << 62   # the encoder takes node quantities in [0, 2^62)


def _nowhere(name) -> Pod:
    """Zero requests, every taint tolerated, a nodeSelector no node satisfies (as X.first_pod of the empty set)."""
    return Pod(name, containers=[Container()], tolerations=[Toleration("", "Exists")], node_selector={"nolabel": "y"})


def limit_cases() -> List[PlanCase]:
    out = []
    # ---- Requested after the fill up to 2^62 - 1 is a plain context and answers to the byte
    n = 3
    nodes = C.pool(n, over={0: dict(mem=Q62 - 1)})
    empty = [[] for _ in range(n)]
    out.append(PlanCase("quantity_below_the_limit", nodes, empty, [
        # 2^62 - 1 - (2^62 - 6) == 5 bytes are left on node 0
        Cand([P("a0", cpu=1, mem=Q62 - 6), P("a1", cpu=1, mem=5)], 1, [0, -1], BATCHED, {},
             [(0, 1, (1, Q62 - 6, 0))], first=0),
        Cand([P("b0", cpu=1, mem=Q62 - 6), P("b1", cpu=1, mem=6)], 1, [0, -1], BATCHED, {0: MEMORY},
             [(0, 1, (1, Q62 - 6, 0))], first=1),
        # Requested == 2^62 - 1 == allocatable: nothing is left, a zero memory request still fits
        Cand([P("c0", cpu=1, mem=Q62 - 1), P("c1", cpu=1)], 1, [0, -1], BATCHED, {},
             [(0, 1, (1, Q62 - 1, 0))], first=0),
        Cand([P("d0", cpu=1, mem=Q62 - 1), P("d1", cpu=1, mem=1)], 1, [0, -1], BATCHED, {0: MEMORY},
             [(0, 1, (1, Q62 - 1, 0))], first=1),
    ]))
    # ---- ... from 2^62 on it is not: SINGLE, where the encoder refuses the filled snapshot
    out.append(PlanCase("quantity_at_the_limit", nodes, empty, [
        Cand([P("a0", cpu=1, mem=Q62), P("a1", cpu=1, mem=1)], 1, [0, -1], SINGLE, {0: MEMORY})]))
    out.append(PlanCase("quantity_two_pods_reach_the_limit", nodes, empty, [
        Cand([P("a0", cpu=1, mem=Q62 // 2), P("a1", cpu=1, mem=Q62 // 2), P("a2", cpu=1, mem=1)], 2, [0, 0, -1], SINGLE,
             {0: MEMORY})]))
    # (2^63 - 1) + 1 is no int64: the merge of the two entries overflows
    out.append(PlanCase("accounting_sum_overflows_int64", nodes, empty, [
        Cand([P("a0", cpu=1, mem=2 * Q62 - 1), P("a1", cpu=1, mem=1), P("a2", cpu=1, mem=1)], 2, [0, 0, -1], SINGLE,
             {0: MEMORY})]))
    # ---- a stop pod no node admits, after earlier pods that fill node 1 (2 slots) and beside node 3, which holds
    # two pods on one slot (slack -1).  The class's program judges the pod count before anything else, whatever
    # decides the class afterwards (a selector row of zeros; required node affinity without a valid term, which
    # the encoder decides without rows), and fitsRequest does not read the selector: NODE_AFFINITY everywhere and
    # PODS on the full nodes
    n = 5
    nodes = C.pool(n, over={1: dict(pods=2), 3: dict(pods=1)})
    base = [[] for _ in range(n)]
    base[3] = [used(cpu=1, name="u0"), used(cpu=1, name="u1")]
    nowhere = {j: NODE_AFFINITY | (PODS if j in (1, 3) else 0) for j in range(n)}
    noterm = Pod("b2", containers=[Container()], required_node_affinity=[NodeSelectorTerm([])])
    out.append(PlanCase("class_decided_everywhere", nodes, base, [
        Cand([P("a0", cpu=1), P("a1", cpu=1), _nowhere("a2")], 2, [1, 1, -1], BATCHED, nowhere, [(1, 2, (2, 0, 0))],
             first=-1),
        Cand([P("b0", cpu=1), P("b1", cpu=1), noterm], 2, [1, 1, -1], BATCHED, nowhere, [(1, 2, (2, 0, 0))], first=-1),
        # one earlier pod leaves node 1 a slot: no PODS there
        Cand([P("c0", cpu=1), _nowhere("c1")], 1, [1, -1], BATCHED, {**nowhere, 1: NODE_AFFINITY}, [(1, 1, (1, 0, 0))],
             first=-1),
    ]))
    # ---- a node over its pod count before the context touches it: slack -1, -2 after the earlier pod
    out.append(PlanCase("negative_slack_touched", nodes, base, [
        Cand([P("a0", cpu=1), P("a1", cpu=10)], 1, [3, -1], BATCHED, {3: PODS}, [(3, 1, (1, 0, 0))], first=0),
        Cand([P("b0", cpu=1), P("b1", cpu=0)], 1, [3, -1], BATCHED, {3: PODS}, [(3, 1, (1, 0, 0))], first=0),
        Cand([P("c0", cpu=10)], 0, [-1], BATCHED, {3: PODS}, [], first=0),
    ]))
    # ---- a dimension the stop pod asks zero of still refuses on a node the context over-commits in it:
    # 8 GiB < 0 + 0 + 9 GiB.  Only a request of all zeros is let through
    out.append(PlanCase("zero_dimension_over_committed", nodes, base, [
        Cand([P("a0", cpu=1, mem=9 * GiB), P("a1", cpu=10)], 1, [2, -1], BATCHED, {2: MEMORY, 3: PODS},
             [(2, 1, (1, 9 * GiB, 0))], first=0),
        Cand([P("b0", cpu=1, mem=9 * GiB), P("b1", cpu=0, mem=1)], 1, [2, -1], BATCHED, {2: MEMORY, 3: PODS},
             [(2, 1, (1, 9 * GiB, 0))], first=0),
        Cand([P("c0", cpu=1, mem=9 * GiB), P("c1", cpu=0)], 1, [2, -1], BATCHED, {3: PODS},
             [(2, 1, (1, 9 * GiB, 0))], first=0),
        Cand([P("d0", cpu=1, mem=8 * GiB), P("d1", cpu=10)], 1, [2, -1], BATCHED, {3: PODS},
             [(2, 1, (1, 8 * GiB, 0))], first=0),
        Cand([P("e0", cpu=1, mem=1, eph=C.E10 + 1), P("e1", cpu=10, mem=1)], 1, [0, -1], BATCHED,
             {0: EPHEMERAL, 3: PODS}, [(0, 1, (1, 1, C.E10 + 1))], first=1),
    ]))
    names = [c.name for c in out]
    assert len(names) == len(set(names))
    return out


REFUSED = ("quantity_at_the_limit", "quantity_two_pods_reach_the_limit", "accounting_sum_overflows_int64")
NO_INT64 = "accounting_sum_overflows_int64"   # the oracle adds in int64 as well: it is not asked
