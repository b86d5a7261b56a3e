"""Inputs and hand-derived expectations for sr_shortfall_pods / sr_shortfall_plan at the sizes where their
reductions can go wrong: pools of 65, 257 and 320 spot nodes whose node j is built from a formula of j, so the
mask and the four shortfalls of every node are arithmetic on j.

A case is an explain_plan_cases.PlanCase (candidates, the pod asked for, where the earlier pods went) with, per
candidate, the expected shortfalls of every refusing node (`shorts`: {node: (cpu, memory, ephemeral, pods)}, every
other node zeros) and the reductions a reader can check by eye (`pin`: near / only_nodes / only_min / only_at).
A candidate asked at its first pod has an empty context: the same pod goes through sr_shortfall_pods too.

  minimum     the unique smallest only-d shortfall at 0, 63, 64, 255, 256, the last live node and nowhere; equal
              minima at {63, 64} (two waves) and {255, 256} (two blocks); a last word of one live node and 63 pads
  high bits   2^32 + 1 against 2^32 - 1 (the low word of the smaller is the larger); a shortfall of 2^61
  dimensions  every dimension as the only bit, two and three resource bits, a resource bit beside a taint, a
              zero-request pod, a zero cpu request on an over-committed node, a class decided without rows
  contexts    touched nodes on a residue turned cpu-only by one milli, exactly at the limit, 110 against 109 pods
  pods        allowed pods near -2^63: the one shortfall that saturates at 2^63 - 1
  split       65,537 queries on a 70-node pool, a context each (`split_input`)

tests/test_shortfall_reference.py proves every expectation on the CPU (the oracle's arithmetic and the host
statements); tests/test_gpu_shortfall_sizes.py runs them through the C ABI."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

import explain_plan_cases as C
from explain_plan_cases import BATCHED, Cand, PlanCase
from explain_cases import CPU, EPHEMERAL, MEMORY, NODE_AFFINITY, PODS, TAINT
from helpers import Scenario
from known_answer import N, P, used
from spotplanner.model import Container, GiB, NodeSelectorTerm, Pod, Taint

KEY = Taint("k", "v", "NoSchedule")
NODE = (4000, 8 * GiB, 10 * GiB)   # allocatable cpu / memory / ephemeral of a pool node
REQ = (500, 1 * GiB, 1 * GiB)      # the full pod's requests
DIM_BITS = (CPU, MEMORY, EPHEMERAL, PODS)
INT64_MAX = (1 << 63) - 1
POOLS = (65, 257, 320)


@dataclass
class SCase:
    name: str
    plan: PlanCase
    shorts: List[Dict[int, Tuple[int, int, int, int]]]   # per candidate
    pin: List[dict] = field(default_factory=list)         # per candidate: the reductions stated by hand (may be {})

    def expected_shorts(self, c: int) -> List[List[int]]:
        return [list(self.shorts[c].get(j, (0, 0, 0, 0))) for j in range(len(self.plan.nodes))]


def _z(name) -> Pod:
    return Pod(name, containers=[Container()])


def _used(j, short, req=REQ, node=NODE):
    """A base pod that leaves node j `short[d]` units short of `req[d]` in every dimension d named in `short`
    (allocatable - request + short are taken), and nothing taken elsewhere."""
    take = [node[d] - req[d] + short[d] if d in short else 0 for d in range(3)]
    return used(cpu=take[0], mem=take[1], eph=take[2], name="u%d" % j)


def _ask(pod: Pod, masks, shorts):
    """One candidate of one pod, asked at it: an empty context."""
    return Cand([pod], 0, [-1], BATCHED, masks, []), shorts


# ---- the unique minimum (or equal minima) of dimension d at given positions
MIN_SHORT = 7


def min_case(n: int, d: int, at: Tuple[int, ...], name: str) -> SCase:
    """The full pod on a pool where node j is only-d with shortfall 1000 + j, but MIN_SHORT at the nodes of `at`;
    j % 5 == 2: a taint beside a shortfall of 1 in d (smaller than every only-d one: it must never win);
    j % 7 == 3: feasible.  `at` empty: the only-d nodes are short of a second dimension too (no only node at all)."""
    e = (d + 1) % 3
    nodes, base, masks, shorts = [], [], {}, {}
    for j in range(n):
        kw, on = {}, []
        if j in at:
            s = {d: MIN_SHORT}
        elif j % 5 == 2:
            s, kw = {d: 1}, dict(taints=[KEY])
        elif j % 7 == 3:
            s = {}
        elif at:
            s = {d: 1000 + j}
        else:
            s = {d: 1000 + j, e: 5}
        if s:
            on.append(_used(j, s))
            masks[j] = sum(DIM_BITS[x] for x in s) | (TAINT if kw else 0)
            shorts[j] = tuple(s.get(x, 0) for x in range(3)) + (0,)
        nodes.append(N("n%d" % j, cpu=NODE[0], mem=NODE[1], eph=NODE[2], **kw))
        base.append(on)
    cand, sh = _ask(P("full", cpu=REQ[0], mem=REQ[1], eph=REQ[2]), masks, shorts)
    near = sum(1 for m in masks.values() if not m & TAINT)
    only = sum(1 for m in masks.values() if m == DIM_BITS[d])
    pin = dict(near=near, only_nodes=[only if x == d else 0 for x in range(4)],
               only_min=[MIN_SHORT if x == d and at else 0 for x in range(4)],
               only_at=[min(at) if x == d and at else -1 for x in range(4)])
    return SCase(name, PlanCase(name, nodes, base, [cand]), [sh], [pin])


def min_cases() -> List[SCase]:
    out = []
    for n in POOLS:
        spots = [("0", (0,)), ("63", (63,)), ("64", (64,)), ("255", (255,)), ("256", (256,)), ("last", (n - 1,)),
                 ("nowhere", ())]
        for k, (tag, at) in enumerate(spots):
            if at and at[0] >= n:
                continue
            out.append(min_case(n, k % 3, at, "min_%d_at_%s" % (n, tag)))
    out.append(min_case(320, 0, (63, 64), "tie_two_waves"))
    out.append(min_case(320, 1, (255, 256), "tie_two_blocks"))
    out.append(min_case(257, 2, (64, 256), "tie_across_three_blocks"))
    return out


# ---- shortfalls that differ only above bit 31, and one of 2^61
def high_cases() -> List[SCase]:
    out = []
    n, mem = 130, 1 << 40
    req = 1 << 33
    sf = {j: (1 << 34) + j for j in range(n)}
    sf[3], sf[70] = (1 << 32) + 1, (1 << 32) - 1
    nodes = [N("n%d" % j, cpu=NODE[0], mem=mem, eph=NODE[2]) for j in range(n)]
    base = [[used(mem=mem - req + sf[j], name="u%d" % j)] for j in range(n)]
    cand, sh = _ask(P("big", cpu=1, mem=req), {j: MEMORY for j in range(n)}, {j: (0, sf[j], 0, 0) for j in range(n)})
    pin = dict(near=n, only_nodes=[0, n, 0, 0], only_min=[0, (1 << 32) - 1, 0, 0], only_at=[-1, 70, -1, -1])
    out.append(SCase("above_bit_31", PlanCase("above_bit_31", nodes, base, [cand]), [sh], [pin]))
    # the pod asks 2^61 + 1024 bytes; node 64 offers 1024, every other node none
    n = 65
    nodes = [N("n%d" % j, cpu=NODE[0], mem=1024 if j == 64 else 0, eph=NODE[2]) for j in range(n)]
    big = (1 << 61) + 1024
    cand, sh = _ask(P("huge", cpu=1, mem=big), {j: MEMORY for j in range(n)},
                    {j: (0, big - (1024 if j == 64 else 0), 0, 0) for j in range(n)})
    pin = dict(near=n, only_nodes=[0, n, 0, 0], only_min=[0, 1 << 61, 0, 0], only_at=[-1, 64, -1, -1])
    out.append(SCase("two_to_the_61", PlanCase("two_to_the_61", nodes, [[] for _ in range(n)], [cand]),
                     [sh], [pin]))
    return out


# ---- every dimension alone, several together, beside a taint; the pods whose request skips or keeps a compare
DIMS_N = 65


def dims_spec(j: int) -> dict:
    """Node j of the dimensions pool by j % 8: what its base pods take (`take`), zero-request fillers and the
    allowed pods (`fill`, `pods`), a taint."""
    k = j % 8
    s = dict(take=(0, 0, 0), fill=0, pods=110, taint=False)
    full = lambda short: tuple(NODE[d] - REQ[d] + short[d] if short[d] else 0 for d in range(3))  # noqa: E731
    if k == 1:    # cpu alone; every second one over-committed (more requested than allocatable)
        s["take"] = (NODE[0] + j, 0, 0) if j % 16 == 9 else full((10 + j, 0, 0))
    elif k == 2:  # memory alone
        s["take"] = full((0, 20 + j, 0))
    elif k == 3:  # ephemeral alone
        s["take"] = full((0, 0, 30 + j))
    elif k == 4:  # the pod count alone: one slot, 1 .. 3 pods on it
        s.update(fill=1 + (j // 8) % 3, pods=1)
    elif k == 5:  # cpu and memory
        s["take"] = full((5 + j, 6 + j, 0))
    elif k == 6:  # all three
        s["take"] = full((1 + j, 2 + j, 3 + j))
    elif k == 7:  # a taint beside cpu
        s.update(take=full((1, 0, 0)), taint=True)
    return s


def dims_expect(req, j: int):
    """fitsRequest for a pod asking `req` on node j of the dimensions pool: (mask, shortfalls)."""
    s = dims_spec(j)
    mask, short = (TAINT if s["taint"] else 0), [0, 0, 0, 0]
    if s["fill"] + 1 > s["pods"]:
        mask |= PODS
        short[3] = s["fill"] + 1 - s["pods"]
    if any(req):
        for d in range(3):
            if NODE[d] < req[d] + s["take"][d]:
                mask |= DIM_BITS[d]
                short[d] = req[d] + s["take"][d] - NODE[d]
    return mask, tuple(short)


DIMS_PODS = [("full", REQ), ("zero", (0, 0, 0)), ("zero_cpu", (0, 1, 0)), ("cpu_only", (REQ[0], 0, 0))]


def dims_case() -> SCase:
    n = DIMS_N
    nodes, base = [], []
    for j in range(n):
        s = dims_spec(j)
        on = [used(cpu=s["take"][0], mem=s["take"][1], eph=s["take"][2], name="u%d" % j)] if any(s["take"]) else []
        on += [_z("f%d-%d" % (j, i)) for i in range(s["fill"])]
        nodes.append(N("n%d" % j, cpu=NODE[0], mem=NODE[1], eph=NODE[2], pods=s["pods"],
                       taints=[KEY] if s["taint"] else []))
        base.append(on)
    cands, shorts, pins = [], [], []
    for name, req in DIMS_PODS:
        ex = {j: dims_expect(req, j) for j in range(n)}
        cand, sh = _ask(P(name, cpu=req[0], mem=req[1], eph=req[2]), {j: m for j, (m, _) in ex.items() if m},
                        {j: s for j, (m, s) in ex.items() if m})
        cands.append(cand)
        shorts.append(sh)
        pins.append({})
    # stated by hand.  full: j % 8 == 1 is cpu-only, 10 + j short (500 + j over-committed): 11 at node 1;
    # memory-only 22 at node 2; ephemeral-only 33 at node 3; pods-only 1 at node 4; 8 nodes each (j < 65), near
    # misses are j % 8 in 1 .. 6: 8 * 6.  zero: only the pod count, the taint on j % 8 == 7.  zero_cpu: a cpu
    # shortfall of j on the over-committed nodes 9, 25, 41, 57 alone
    pins[0] = dict(near=48, only_nodes=[8, 8, 8, 8], only_min=[11, 22, 33, 1], only_at=[1, 2, 3, 4])
    pins[1] = dict(near=8, only_nodes=[0, 0, 0, 8], only_min=[0, 0, 0, 1], only_at=[-1, -1, -1, 4])
    pins[2] = dict(near=12, only_nodes=[4, 0, 0, 8], only_min=[9, 0, 0, 1], only_at=[9, -1, -1, 4])
    # a class decided without rows (required node affinity without a valid term): NODE_AFFINITY everywhere, the
    # pod count judged first (explain_plan_sizes.limit_cases): a pod shortfall only where the mask holds PODS,
    # no near miss, no only node
    noterm = Pod("noterm", containers=[Container()], required_node_affinity=[NodeSelectorTerm([])])
    ex = {j: dims_expect((0, 0, 0), j) for j in range(n)}
    cand, sh = _ask(noterm, {j: (ex[j][0] & (PODS | TAINT)) | NODE_AFFINITY for j in range(n)},
                    {j: (0, 0, 0, ex[j][1][3]) for j in range(n) if ex[j][0] & PODS})
    cands.append(cand)
    shorts.append(sh)
    pins.append(dict(near=0, only_nodes=[0] * 4, only_min=[0] * 4, only_at=[-1] * 4))
    return SCase("dimensions", PlanCase("dimensions", nodes, base, cands), shorts, pins)


# ---- contexts: touched nodes on a residue of a 320-node pool
CTX_N, CTX_MOD = 320, 37


def ctx_case() -> SCase:
    """1000m nodes, a 700m stop pod.  a: 301m earlier pods on j % 37 == 15: one milli short there; b: 300m on
    j % 37 == 33: exactly at the limit, still feasible; c: 110 one-milli pods on node 256 (110 allowed) merged into
    one entry: a pod shortfall of 1, 810m fit; d: 109 of them: feasible; e: 111 on node 64 and a 295m pod: 112 + 1
    against 110 pods, 406m + 700m against 1000m."""
    n = CTX_N
    nodes = C.pool(n)
    base = [[] for _ in range(n)]
    at15 = [j for j in range(n) if j % CTX_MOD == 15]
    at33 = [j for j in range(n) if j % CTX_MOD == 33]
    cands, shorts, pins = [], [], []

    def add(pods, mapping, masks, ctx, sh, pin):
        cands.append(Cand(pods, len(pods) - 1, mapping + [-1], BATCHED, masks, ctx))
        shorts.append(sh)
        pins.append(pin)
    add([P("a%d" % i, cpu=301) for i in range(len(at15))] + [P("a-stop", cpu=700)], at15,
        {j: CPU for j in at15}, [(j, 1, (301, 0, 0)) for j in at15], {j: (1, 0, 0, 0) for j in at15},
        dict(near=len(at15), only_nodes=[len(at15), 0, 0, 0], only_min=[1, 0, 0, 0], only_at=[15, -1, -1, -1]))
    add([P("b%d" % i, cpu=300) for i in range(len(at33))] + [P("b-stop", cpu=700)], at33, {},
        [(j, 1, (300, 0, 0)) for j in at33], {},
        dict(near=0, only_nodes=[0] * 4, only_min=[0] * 4, only_at=[-1] * 4))
    add([P("c%d" % i, cpu=1) for i in range(110)] + [P("c-stop", cpu=700)], [256] * 110, {256: PODS},
        [(256, 110, (110, 0, 0))], {256: (0, 0, 0, 1)},
        dict(near=1, only_nodes=[0, 0, 0, 1], only_min=[0, 0, 0, 1], only_at=[-1, -1, -1, 256]))
    add([P("d%d" % i, cpu=1) for i in range(109)] + [P("d-stop", cpu=700)], [256] * 109, {},
        [(256, 109, (109, 0, 0))], {},
        dict(near=0, only_nodes=[0] * 4, only_min=[0] * 4, only_at=[-1] * 4))
    add([P("e%d" % i, cpu=1) for i in range(111)] + [P("e-big", cpu=295), P("e-stop", cpu=700)], [64] * 112,
        {64: PODS | CPU}, [(64, 112, (406, 0, 0))], {64: (106, 0, 0, 3)},
        dict(near=1, only_nodes=[0] * 4, only_min=[0] * 4, only_at=[-1] * 4))
    return SCase("contexts", PlanCase("contexts", nodes, base, cands), shorts, pins)


# ---- allowed pods near -2^63: where the pod shortfall saturates
def saturation_case() -> SCase:
    """pods + 1 - allowed: node 0 allows -2^63 + 2 and holds one pod: 2^63, which no int64 holds: 2^63 - 1; node 1
    the same allowance, empty: 2^63 - 1 exactly; node 2 allows -2^63 + 3: 2^63 - 2; node 3 allows 110."""
    lo = -(1 << 63)
    nodes = [N("a", pods=lo + 2), N("b", pods=lo + 2), N("c", pods=lo + 3), N("d")]
    base = [[_z("x")], [], [], []]
    cand, sh = _ask(P("p", cpu=10), {0: PODS, 1: PODS, 2: PODS},
                    {0: (0, 0, 0, INT64_MAX), 1: (0, 0, 0, INT64_MAX), 2: (0, 0, 0, INT64_MAX - 1)})
    pin = dict(near=3, only_nodes=[0, 0, 0, 3], only_min=[0, 0, 0, INT64_MAX - 1], only_at=[-1, -1, -1, 2])
    return SCase("pods_saturate", PlanCase("pods_saturate", nodes, base, [cand]), [sh], [pin])


def cases() -> List[SCase]:
    out = min_cases() + high_cases() + [dims_case(), ctx_case(), saturation_case()]
    names = [c.name for c in out]
    assert len(names) == len(set(names))
    return out


# ---- the hand tick of DESIGN.md 1.2: five 600m pods, four open 1000m nodes
def hand_tick():
    """(Built, the candidate's fifth pod): against the snapshot as it is the four nodes take the pod; after the
    candidate's own four earlier pods each is 200m short."""
    case = PlanCase("hand_tick", C.pool(4), [[] for _ in range(4)],
                    [Cand([P("c-%d" % k, cpu=600) for k in range(5)], 4, [0, 1, 2, 3, -1], BATCHED,
                          {j: CPU for j in range(4)}, [(j, 1, (600, 0, 0)) for j in range(4)])])
    return C.Built(case)


# ---- 65,537 queries on a 70-node pool: launch_shortfall_plan's second launch starts at query 65,535
SPLIT_QUERIES, SPLIT_NODES = 65537, 70
SPLIT_EARLIER = (301, 302, 350)   # the earlier pod of query c asks SPLIT_EARLIER[c % 3] and sits on node c % 70


def split_input():
    """(scenario, cand_off, cand_pods, at_pod, node_of_pod): every candidate is [an earlier pod, the 700m stop
    pod]; the 1000m node c % 70 is cpu-only for query c, 1 / 2 / 50 short, every other node takes the pod."""
    nodes = C.pool(SPLIT_NODES)
    sc = Scenario(nodes, [[] for _ in nodes], [P("e%d" % k, cpu=v) for k, v in enumerate(SPLIT_EARLIER)] +
                  [P("stop", cpu=700)])
    n = SPLIT_QUERIES
    c = np.arange(n)
    cand_off = (2 * np.arange(n + 1)).astype(np.int32)
    cand_pods = np.stack([sc.q0 + c % 3, np.full(n, sc.q0 + 3)], 1).reshape(-1).astype(np.int32)
    at_pod = np.ones(n, np.int32)
    node_of_pod = np.stack([c % SPLIT_NODES, np.full(n, -1)], 1).reshape(-1).astype(np.int32)
    return sc, cand_off, cand_pods, at_pod, node_of_pod


def split_short(c: int) -> int:
    return SPLIT_EARLIER[c % 3] + 700 - 1000
