"""The inputs of the sequence tests at the ledger's and K2's size boundaries
(test_sequence_sizes_reference.py asserts their preconditions on the oracle,
test_gpu_sequence_sizes.py runs them on the GPU).

ladder:       many one-pod candidates of which only the listed ones ("wins")
              and the candidate directly below each one (its "twin") fit: the
              wins sit on both sides of every stride of the ledger kernels
              (64 lanes, 1,024 threads, 16,384 = 64 blocks of 256) and early
              candidates without pods keep the active index (cand_src's rank)
              apart from the caller's.
large_drains: candidates of 64 to 512 pods that drain one after the other, so
              that a winner's mapping is longer than a wave and every K2 path
              of a large candidate runs under a floor and against a snapshot
              an earlier large drain changed.
many_needs:   limits under which one candidate commits 512 needs, one is
              refused by a need that is not its first, one by its last.

Every input is built once per process and carries pod stamps."""
from __future__ import annotations

import random
from typing import Dict, List

import numpy as np

from domain_cases import Z, pod as domain_pod, term
from sequence_ref import SeqInput, from_scenario
from spotplanner.model import Container, Node, Pod

FITS, TOO_BIG, SPOT_CPU = 100, 4000, 1000
EMPTIES = (10, 500, 5000)
LADDERS = {
    "ladder-17k": dict(n=16900, wins=[63, 64, 65, 1023, 1024, 1025, 2048, 4096, 16383, 16384, 16385, -1]),
    "ladder-4200-domain": dict(n=4200, wins=[63, 64, 1023, 1024, 2047, 2048, 4099, -1], domain=True),
}


class Ladder:
    """The input and what it was built from: `wins` / `twins` are active indices, `active` the caller's index
    of each active candidate, `domain` the caller's indices of the two-pod anti-affinity candidates, `cands`
    and `nodes` the objects."""

    def __init__(self, inp: SeqInput, nodes, cands, wins, twins, active, domain):
        self.inp, self.nodes, self.cands = inp, nodes, cands
        self.wins, self.twins, self.active, self.domain = wins, twins, active, domain

    def caller(self, active_indices) -> List[int]:
        return [int(self.active[a]) for a in active_indices]


def _cpu_pod(name, cpu) -> Pod:
    return Pod(name, containers=[Container(cpu_milli=cpu)])


def ladder(n, wins, empties=EMPTIES, domain=False, fallback_at=None, name="ladder") -> Ladder:
    """`n` candidates (the ones at the caller's indices `empties` without pods); a win of -1 is the last active
    candidate.  `fallback_at`: the active index of one candidate whose pod has a claim (the reference path)."""
    empties = set(e for e in empties if e < n)
    active = np.array([g for g in range(n) if g not in empties], np.int32)
    wins = sorted(set(len(active) - 1 if a < 0 else a for a in wins))
    twins = sorted(set(a - 1 for a in wins) - set(wins))
    small = set(wins) | set(twins)
    assert wins[0] >= 1 and wins[-1] < len(active) and (fallback_at is None or fallback_at not in small)
    labels = [{Z: "a"}, {Z: "a"}, {Z: "b"}] if domain else [{}, {}, {}]
    nodes = [Node("s%d" % i, cpu_milli=SPOT_CPU, labels=labels[i]) for i in range(3)]
    cands, dom = [], []
    rank = {int(g): a for a, g in enumerate(active)}
    for g in range(n):
        if g in empties:
            cands.append([])
            continue
        a = rank[g]
        if domain and a % 200 == 100 and a not in small:  # two pods that refuse each other's zone
            pods = [domain_pod("d%d_%d" % (g, k), "web", anti=[term(Z, "web")]) for k in range(2)]
            for p in pods:
                p.containers[0].cpu_milli = TOO_BIG
            cands.append(pods)
            dom.append(g)
            continue
        pods = [_cpu_pod("p%d" % g, FITS if a in small else TOO_BIG)]
        if g % 7 == 0:  # pod offsets apart from candidate indices
            pods.insert(0, _cpu_pod("f%d" % g, 10))
        if a == fallback_at:
            pods[-1].has_pvc = True
        cands.append(pods)
    inp = from_scenario(nodes, [[] for _ in nodes], cands, stamped=name)
    return Ladder(inp, nodes, cands, wins, twins, active, dom)


def ladder_limits(lad: Ladder, also_refused=()):
    """Group 0 (nothing allowed) holds every twin's last pod and the last pod of the active candidates
    `also_refused`; each win's last pod is in one of groups 1-3, which allow exactly the wins they hold."""
    off = lad.inp.cand_off - lad.inp.cand_off[0]
    pod_group = np.full(int(off[-1]), -1, np.int32)
    allowed = np.zeros(4, np.int32)
    for a in list(lad.twins) + list(also_refused):
        pod_group[off[lad.active[a] + 1] - 1] = 0
    for k, a in enumerate(lad.wins):
        pod_group[off[lad.active[a] + 1] - 1] = 1 + k % 3
        allowed[1 + k % 3] += 1
    return allowed, pod_group


FALLBACK_AT = 16500  # ladder-17k-fallback: the active index of its reference-path candidate

_ladders: Dict[str, Ladder] = {}


def get_ladder(name: str) -> Ladder:
    if name not in _ladders:
        if name == "ladder-17k-fallback":  # the wins end below the fallback candidate, failed ones in between
            kw = dict(LADDERS["ladder-17k"])
            kw["wins"] = [w for w in kw["wins"] if w >= 0]
            _ladders[name] = ladder(name=name, fallback_at=FALLBACK_AT, **kw)
        else:
            _ladders[name] = ladder(name=name, **LADDERS[name])
    return _ladders[name]


# ------------------------------------------------------------------ large candidates that drain
# (the 3-pod candidates at the end keep a round running behind the large ones: see many_needs)
PLAIN_SIZES = [65, 0, 128, 40, 129, 256, 30, 257, 512, 64, 3]
PLAIN_FAILING = (3, 6)  # the 40- and 30-pod candidates end in a pod that fits nowhere
DOMAIN_SIZES = [64, 65, 127, 128, 255, 256, 299, 511]  # web-c pods; one db-c pod each on top
DOMAIN_TAIL = 3  # ... and one candidate of three pods without terms behind them
KINDS = ("plain", "spread-out", "domain", "ext")
# spread-out: one pod slot per node, so a drain of m pods lands on m distinct nodes
SPREAD_SIZES = [64, 70, 65, 128, 140, 129, 200]


def _plain(ext: bool):
    r = random.Random(1711)
    nodes = [Node("s%d" % i, cpu_milli=1500, pods=12) for i in range(300)]
    if ext:
        for i in range(0, len(nodes), 3):
            nodes[i].scalar = {"example.com/dongle": 4}
    cands = []
    for c, m in enumerate(PLAIN_SIZES):
        pods = [_cpu_pod("c%d_%d" % (c, k), r.choice([100, 150, 200, 250, 300, 400])) for k in range(m)]
        if ext:
            for k, p in enumerate(pods):
                if k % 5 == 1:  # fit request above the accounting: an extension record when not the last pod
                    p.init_containers = [Container(cpu_milli=600)]
                if k % 11 == 3:
                    p.containers[0].scalar = {"example.com/dongle": 1}
        if c in PLAIN_FAILING:
            pods[-1] = _cpu_pod("c%d_big" % c, 5000)
        cands.append(pods)
    return nodes, [[] for _ in nodes], cands


def _spread_out():
    """One pod slot per node; the nodes differ in CPU so that a drain does not simply take the next free ones.
    A candidate of m pods lands on m distinct nodes: 64 / 65 and 128 / 129 sit at the touched-slot edges, 70,
    140 and 200 beyond them."""
    r = random.Random(1712)
    nodes = [Node("s%d" % i, cpu_milli=r.choice([300, 500, 1000]), pods=1) for i in range(sum(SPREAD_SIZES) + 40)]
    cands = [[_cpu_pod("c%d_%d" % (c, k), r.choice([100, 250, 400])) for k in range(m)]
             for c, m in enumerate(SPREAD_SIZES)]
    return nodes, [[] for _ in nodes], cands


def _domain():
    nodes = []
    for i in range(72):
        labels = {} if i % 9 == 8 else {Z: "z%d" % (i % 8)}
        nodes.append(Node("s%d" % i, cpu_milli=8000, pods=110, labels=labels))
    cands = []
    for c, m in enumerate(DOMAIN_SIZES):
        pods = [domain_pod("w%d_%d" % (c, k), "web-%d" % c, anti=[term(Z, "db-%d" % c)]) for k in range(m)]
        pods.insert(m // 3, domain_pod("db%d" % c, "db-%d" % c))
        cands.append(pods)
    cands.append([domain_pod("t%d" % k, "tail") for k in range(DOMAIN_TAIL)])
    return nodes, [[] for _ in nodes], cands


_large: Dict[str, SeqInput] = {}
_objects: Dict[str, tuple] = {}


def large_objects(kind: str):
    """(nodes, spot pods, candidates) of large_drains(kind)."""
    if kind not in _objects:
        _objects[kind] = {"plain": lambda: _plain(False), "ext": lambda: _plain(True), "spread-out": _spread_out,
                          "domain": _domain}[kind]()
    return _objects[kind]


def large_drains(kind: str) -> SeqInput:
    if kind not in _large:
        _large[kind] = from_scenario(*large_objects(kind), stamped="large-" + kind)
    return _large[kind]


def distinct_nodes(inp: SeqInput, ref, c) -> int:
    off = inp.cand_off - inp.cand_off[0]
    return len(set(int(x) for x in ref.node_of_pod[off[c]:off[c + 1]]))


# ------------------------------------------------------------------ limits with hundreds of needs
def big_and_later(inp: SeqInput):
    """(the largest candidate, the next candidate behind it with at least 64 pods -- or, when it is last, the
    largest one before it)."""
    sizes = np.diff(inp.cand_off)
    big = int(np.argmax(sizes))
    later = [c for c in range(big + 1, len(sizes)) if sizes[c] >= 64]
    return big, (later[0] if later else int(np.argmax(sizes[:big])))


def many_needs(inp: SeqInput, refuse_last: bool = False):
    """Pod k of the largest candidate (m pods) is alone in group 1 + k: accepted with every need exactly at what
    is left, it commits m needs.  The other large candidate (see big_and_later) has its pod 0 in group 0, which
    the big one does not use and which always holds -- a candidate's needs ascend by group, so that need is its
    first -- and its other pods one each in the big one's highest groups.  Behind the big candidate it is
    refused by those, never by its first need; in front of it the shared groups allow two evictions, it drains
    and the big one is then accepted at equality.  `refuse_last`: the big candidate's last group allows
    nothing, the only one of its m needs that refuses it.
    Returns (allowed, pod_group)."""
    off = inp.cand_off - inp.cand_off[0]
    big, other = big_and_later(inp)
    m = int(off[big + 1] - off[big])
    k = int(off[other + 1] - off[other])
    pod_group = np.full(int(off[-1]), -1, np.int32)
    pod_group[off[big]:off[big + 1]] = 1 + np.arange(m)
    allowed = np.ones(m + 1, np.int32)
    pod_group[off[other]] = 0
    if other > big:  # (with refuse_last not the last group: the candidate then drains behind the refused big one)
        top = m if refuse_last else m + 1
        pod_group[off[other] + 1:off[other + 1]] = np.arange(top - (k - 1), top)
    else:  # (not the big one's last group: refuse_last is to be the only refusing need)
        pod_group[off[other] + 1:off[other + 1]] = 1 + np.arange(k - 1)
        allowed[1:k] = 2
    if refuse_last:
        allowed[m] = 0
    return allowed, pod_group


def masking_large(inp: SeqInput, ref):
    """masking_groups for a large pair: the first two consecutive drains of the plain pass `ref` that both have
    more than 128 pods; the lower one's pods are all in group 0, which allows one eviction fewer than it needs.  Returns (refused candidate, allowed, pod_group)."""
    off = inp.cand_off - inp.cand_off[0]
    sizes = np.diff(inp.cand_off)
    d = [int(c) for c in ref.drained]
    c = next(a for a, b in zip(d, d[1:]) if sizes[a] > 128 and sizes[b] > 128)
    pod_group = np.full(int(off[-1]), -1, np.int32)
    pod_group[off[c]:off[c + 1]] = 0
    return c, np.array([sizes[c] - 1], np.int32), pod_group


def sliced(inp: SeqInput, pad: int = 37):
    """The same candidates as a slice of a longer pod list: cand_pod_off[0] == pad."""
    filler = np.resize(inp.cand_pods[::-1], pad).astype(np.int32)  # unrelated pod indices in front
    return SeqInput(inp.ptr, inp.spot, inp.node_pod_off, inp.node_pod_idx, (inp.cand_off + pad).astype(np.int32),
                    np.concatenate([filler, inp.cand_pods]).astype(np.int32), keep=inp.keep)
