"""Hand cases for sr_node_view_pods / sr_node_view_plan: a few nodes and pods each, every expected number
written out.

A case is an explain_plan_cases.PlanCase (candidates, the pod asked for, where the earlier pods went; per
candidate the expected mask of every refusing node) with, per candidate, the expected shortfalls of every refusing
node (`shorts`: {node: (cpu, memory, ephemeral, pods)}) and the per-node result stated by hand (`want`):

  judged    the queries counted
  admits    [n_spot]
  near      [n_spot]
  refuses   {node: {reason name: queries}}, everything else 0
  sole      {node: {reason name: queries}}, everything else 0
  closest   {node: {dimension name: (smallest sole shortfall, lowest slot attaining it)}}, everything else (0, -1)

`as_pods`: every candidate is asked at its first pod, so the same pods through sr_node_view_pods give the same
numbers (slot = asked index = candidate).  tests/test_node_view_reference.py proves the masks and shortfalls on
the oracle and that `want` is their fold; tests/test_gpu_node_view.py runs the cases through the C ABI."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import explain_plan_cases as C
import shortfall_sizes as S
from explain_cases import CPU, PODS, PORTS, TAINT
from explain_plan_cases import BATCHED, NONE, SINGLE, Cand, PlanCase
from known_answer import N, P, used
from spotplanner import capi
from spotplanner.model import Container, Pod, Taint

KEY = Taint("k", "v", "NoSchedule")
INT64_MAX = (1 << 63) - 1


@dataclass
class VCase:
    name: str
    plan: PlanCase
    shorts: List[Dict[int, Tuple[int, int, int, int]]]   # per candidate
    want: dict
    fallback: List[int] = field(default_factory=list)     # per candidate (default: none)
    as_pods: bool = False

    def expected_shorts(self, c: int) -> List[List[int]]:
        return [list(self.shorts[c].get(j, (0, 0, 0, 0))) for j in range(len(self.plan.nodes))]

    def expected_fallback(self) -> List[int]:
        return self.fallback or [0] * len(self.plan.cands)

    def expanded(self) -> dict:
        """`want` as node_view_ref.fold returns it."""
        n = len(self.plan.nodes)
        w = self.want
        out = dict(judged=w["judged"], admits=list(w["admits"]), near=list(w["near"]),
                   refuses=[[0] * capi.SR_WHY_COUNT for _ in range(n)], sole=[[0] * capi.SR_WHY_COUNT for _ in range(n)],
                   sole_min=[[0] * capi.SR_SHORT_COUNT for _ in range(n)],
                   sole_at=[[-1] * capi.SR_SHORT_COUNT for _ in range(n)])
        assert len(out["admits"]) == len(out["near"]) == n
        for f in ("refuses", "sole"):
            for j, by in w.get(f, {}).items():
                for name, k in by.items():
                    out[f][j][capi.WHY_NAMES.index(name)] = k
        for j, by in w.get("closest", {}).items():
            for name, (m, at) in by.items():
                d = capi.SHORT_NAMES.index(name)
                out["sole_min"][j][d], out["sole_at"][j][d] = m, at
        return out


def _ask(pod, masks):
    return Cand([pod], 0, [-1], BATCHED, masks, [])


def hand_tick() -> VCase:
    """five 600m pods on four open 1000m nodes.  In the context of the candidate's own four earlier
    pods every node is 200m short for the fifth, and cpu is the only thing wrong with it."""
    plan = S.hand_tick().case
    want = dict(judged=1, admits=[0] * 4, near=[1] * 4, refuses={j: {"CPU": 1} for j in range(4)},
                sole={j: {"CPU": 1} for j in range(4)}, closest={j: {"CPU": (200, 0)} for j in range(4)})
    return VCase("hand_tick", plan, [{j: (200, 0, 0, 0) for j in range(4)}], want)


def leftover_taint() -> VCase:
    """Three 100m pods.  Node 0 carries a leftover taint and nothing else: the taint alone keeps all three off
    it.  Node 1 carries the taint and has 50m left: two bits, so refuses counts the pods and sole does not, and
    no shortfall is reported (cpu is not the only thing wrong).  Node 2 takes them."""
    nodes = [N("t", cpu=1000, taints=[KEY]), N("tc", cpu=1000, taints=[KEY]), N("open", cpu=1000)]
    base = [[], [used(cpu=950)], []]
    cands = [_ask(P("p%d" % i, cpu=100), {0: TAINT, 1: TAINT | CPU}) for i in range(3)]
    want = dict(judged=3, admits=[0, 0, 3], near=[0, 0, 0], refuses={0: {"TAINT": 3}, 1: {"TAINT": 3, "CPU": 3}},
                sole={0: {"TAINT": 3}})
    return VCase("leftover_taint", PlanCase("leftover_taint", nodes, base, cands), [{1: (50, 0, 0, 0)}] * 3, want,
                 as_pods=True)


def tie_lower_slot() -> VCase:
    """Node 0 has 50m left.  Slot 0 asks 200m (150m short), slots 1 and 2 ask 100m (50m short each): the smallest
    shortfall is 50m and the lower of the two slots attaining it is 1."""
    nodes = [N("a", cpu=1000), N("b", cpu=1000)]
    base = [[used(cpu=950)], []]
    cands = [_ask(P("p0", cpu=200), {0: CPU}), _ask(P("p1", cpu=100), {0: CPU}), _ask(P("p2", cpu=100), {0: CPU})]
    want = dict(judged=3, admits=[0, 3], near=[3, 0], refuses={0: {"CPU": 3}}, sole={0: {"CPU": 3}},
                closest={0: {"CPU": (50, 1)}})
    return VCase("tie_lower_slot", PlanCase("tie_lower_slot", nodes, base, cands),
                 [{0: (150, 0, 0, 0)}, {0: (50, 0, 0, 0)}, {0: (50, 0, 0, 0)}], want, as_pods=True)


def tie_single_and_batched() -> VCase:
    """The pair of equal shortfalls where the lower slot goes one at a time and the higher through the batched
    pass, which runs first.  Candidate 0: a host-port pod placed on node 1, then a 100m host-port pod (SINGLE):
    node 0 is 50m short, node 1 holds the port, node 2 takes it.  Candidate 1: a plain 100m pod (BATCHED): node 0
    is 50m short."""
    nodes = [N("a", cpu=1000), N("b", cpu=1000), N("c", cpu=1000)]
    base = [[used(cpu=950)], [], []]
    cands = [Cand([C._hp("a0", 80), C._hp("a1", 80, cpu=100)], 1, [1, -1], SINGLE, {0: CPU, 1: PORTS}),
             _ask(P("p", cpu=100), {0: CPU})]
    want = dict(judged=2, admits=[0, 1, 2], near=[2, 0, 0], refuses={0: {"CPU": 2}, 1: {"PORTS": 1}},
                sole={0: {"CPU": 2}, 1: {"PORTS": 1}}, closest={0: {"CPU": (50, 0)}})
    return VCase("tie_single_and_batched", PlanCase("tie_single_and_batched", nodes, base, cands),
                 [{0: (50, 0, 0, 0)}, {0: (50, 0, 0, 0)}], want)


def fallback_and_not_asked() -> VCase:
    """Four candidates of one pod: a 100m pod; a pod with a PVC (outside the encoded set: asked again alone, still
    fallback); a candidate that is not asked; a zero-request pod.  Two are judged.  Node 0 has 50m left: the 100m
    pod is 50m short, the zero-request pod fits (fitsRequest returns after the pod count).  Node 1 is tainted."""
    nodes = [N("a", cpu=1000), N("b", cpu=1000, taints=[KEY]), N("c", cpu=1000)]
    base = [[used(cpu=950)], [], []]
    cands = [_ask(P("p0", cpu=100), {0: CPU, 1: TAINT}),
             Cand([Pod("fb", containers=[Container(cpu_milli=100)], has_pvc=True)], 0, [-1], SINGLE),
             Cand([P("idle", cpu=100)], -1, [-1], NONE),
             _ask(P("p3", cpu=0), {1: TAINT})]
    want = dict(judged=2, admits=[1, 0, 2], near=[1, 0, 0], refuses={0: {"CPU": 1}, 1: {"TAINT": 2}},
                sole={0: {"CPU": 1}, 1: {"TAINT": 2}}, closest={0: {"CPU": (50, 0)}})
    return VCase("fallback_and_not_asked", PlanCase("fallback_and_not_asked", nodes, base, cands),
                 [{0: (50, 0, 0, 0)}, {}, {}, {}], want, fallback=[0, 1, 0, 0])


def pods_saturate() -> VCase:
    """shortfall_sizes.pods_saturate's nodes: a and b allow -2^63 + 2 pods (a holds one), c allows -2^63 + 3, d
    110.  Candidate 0 places a zero-request pod on c first, then asks a 10m pod; candidate 1 asks a 10m pod.
    pods + earlier + 1 - allowed: on a 2^63 for both, which saturates to 2^63 - 1: a tie, slot 0; on b 2^63 - 1
    for both; on c 2^63 - 1 after candidate 0's earlier pod and 2^63 - 2 without it: the smaller one, slot 1."""
    plan0 = S.saturation_case().plan
    z = Pod("e", containers=[Container()])
    cands = [Cand([z, P("p0", cpu=10)], 1, [2, -1], BATCHED, {0: PODS, 1: PODS, 2: PODS}, [(2, 1, (0, 0, 0))]),
             _ask(P("p1", cpu=10), {0: PODS, 1: PODS, 2: PODS})]
    M = INT64_MAX
    want = dict(judged=2, admits=[0, 0, 0, 2], near=[2, 2, 2, 0], refuses={j: {"PODS": 2} for j in range(3)},
                sole={j: {"PODS": 2} for j in range(3)},
                closest={0: {"PODS": (M, 0)}, 1: {"PODS": (M, 0)}, 2: {"PODS": (M - 1, 1)}})
    return VCase("pods_saturate", PlanCase("pods_saturate", plan0.nodes, plan0.base, cands),
                 [{0: (0, 0, 0, M), 1: (0, 0, 0, M), 2: (0, 0, 0, M)}, {0: (0, 0, 0, M), 1: (0, 0, 0, M), 2: (0, 0, 0, M - 1)}],
                 want)


def admits_and_refuses() -> VCase:
    """Node 0 has 500m left: it takes the 400m pod and is 100m short for the 600m pod."""
    nodes = [N("a", cpu=1000), N("b", cpu=1000)]
    base = [[used(cpu=500)], []]
    cands = [_ask(P("small", cpu=400), {}), _ask(P("big", cpu=600), {0: CPU})]
    want = dict(judged=2, admits=[1, 2], near=[1, 0], refuses={0: {"CPU": 1}}, sole={0: {"CPU": 1}},
                closest={0: {"CPU": (100, 1)}})
    return VCase("admits_and_refuses", PlanCase("admits_and_refuses", nodes, base, cands), [{}, {0: (100, 0, 0, 0)}],
                 want, as_pods=True)


def none_judged() -> VCase:
    """A candidate that is not asked and a fallback pod alone in its batch: nothing is counted."""
    nodes = [N("a", cpu=1000), N("b", cpu=1000, taints=[KEY])]
    base = [[used(cpu=950)], []]
    cands = [Cand([P("idle", cpu=100)], -1, [-1], NONE),
             Cand([Pod("fb", containers=[Container(cpu_milli=100)], has_pvc=True)], 0, [-1], BATCHED)]
    want = dict(judged=0, admits=[0, 0], near=[0, 0])
    return VCase("none_judged", PlanCase("none_judged", nodes, base, cands), [{}, {}], want, fallback=[0, 1])


def cases() -> List[VCase]:
    out = [hand_tick(), leftover_taint(), tie_lower_slot(), tie_single_and_batched(), fallback_and_not_asked(),
           pods_saturate(), admits_and_refuses(), none_judged()]
    assert len({c.name for c in out}) == len(out)
    return out
