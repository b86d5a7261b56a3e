"""Steady ticks whose changed spot node decides the plan: the inputs and the
hand-derived expectations (test_steady_tick_cases_reference.py asserts their
preconditions on the oracle, test_gpu_steady_tick_cases.py runs them on the GPU).

Pools.  Every node: 1000m cpu, 4 GiB memory, 10 GiB ephemeral storage, 110
pods, its hostname label and tier=head (nodes below 512) or tier=far.  A closed
node holds one base pod of 950m, an open node none (the base pod of node 90
also holds memory and ephemeral storage: see NE).  The open nodes have names
(ROLES) that mean the same in every pool:

    A0 A1 A2 = 0 1 2     BM B0 | B1 B2 B3 = 62 63 | 64 65 66 (the first word edge)
    KH                   the head class's open node no tick touches
    ZM Z0                the last two head nodes (510 511; in `head`: 94 95, the pool's last)
    F0 F1 P0 | Q0 Q1     512 513 575 | 576 577 (word 8 | word 9)
    XM X0 | X1 X2        4094 4095 | 4096 4097 (`wide`: the chunk edge)
    KF                   the far class's open node no tick touches
    LM L                 the pool's last two nodes (the last word's padding bits follow L)

Probes.  Every candidate is one probe; all start from the tick's base state.
A "comb" is a run of equal pods of which an open node takes exactly one (a
second does not fit beside it), so pod j lands on the j-th node of its class
that is open *for that kind of pod*; closing a node moves the pod that was on
it and every later one a node further, opening one moves them back:

    kind   request                       closed for it by the filler
    cpu    600m                          c401 (599 = r-1 left), c701, c1050
    port   300m + host port 8080         c701 (299 = r-1 left), c1050
    mem    100m, 3 GiB                   m (3 GiB - 1 MiB left)
    modd   100m, 3 GiB + 1 (odd bytes)   m, m1g (3 GiB = r-1 left; m1gm1 leaves exactly r)
    eph    100m, 6 GiB ephemeral         e (6 GiB - 1 MiB left)
    c1     100m, 3.5 GiB                 m, m1g, m1gm1, mp (3.4 GiB left: `wide` keeps mp or more on every
                                         open far node below 4,096, so c1 first fits in chunk 1)

Fillers are unbound pods of the same cluster added to a tick's snapshot:
cpu-only (c100 ... c1050), memory-only (m, m1g, m1gm1, mp), ephemeral-only (e) and
all-zero (z).  With c400 a node has exactly 600m left (r of the cpu kind), with
c300 700m: inside [600, 1000), 1000 being the threshold the tables gave a 600m
request while no node had 600..999 left.

TICKS[pool][t] is the whole filler state of tick t ({role: [fillers]}); the
candidate input never changes.  t0 and t1 are cold (the tables are written from
t1's state), t2..t10 accumulate to exactly 16 changed nodes, t11 changes a
17th (K0 runs, and applies the pod patches pending since t4), t12 changes one
more node against the new tables, t13 drops every filler.  `head` has no far
nodes and reaches 16 with closed nodes next to the edges (PADS), which decide
nothing.  Beside the cpu combs, spill_head asks for more head nodes than are
open (its last pod scans the far words in vain), g_head / g_far have one pod
per open node of their class (any closed node fails them), the pair asks for
2 x 450m, `ext` starts with an init-container pod, `edge` is an all-zero and a
memory-only pod, big100 / big200 put 91 / 191 memory-only crumbs (110 fill a
node's pod slots) in front of a cpu comb.

ENTRIES lists every decisive (pool, tick, candidate, pod): the node the pod
has on the state the tables were last written from (`before`), the node it
has now, the changed node that decides it, the site in k2_node_order where it
meets that node and the situation (see SITUATIONS).  A guard entry
(before == now) is a pod that must *not* move although a node it could reach
changed: by the definition of (b, f1 = r-1), (c) and (e, all-zero) the stale
and the current plan agree there, so the stale-plan proof does not apply to
them; each stands beside a decisive entry of the same tick and node."""
from __future__ import annotations

from collections import namedtuple
from typing import Dict, List

import zlib

import numpy as np

from helpers import Scenario
from spotplanner.model import Container, ContainerPort, GiB, MiB, Node, Pod

HEAD_NODES = 512
POOLS = {"head": 96, "far": 1100, "wide": 4300}
_HEAD_ROLES = dict(A0=0, A1=1, A2=2, BM=62, B0=63, B1=64, B2=65, B3=66)
_FAR_ROLES = dict(F0=512, F1=513, P0=575, Q0=576, Q1=577)
ROLES: Dict[str, Dict[str, int]] = {
    "head": dict(_HEAD_ROLES, KH=80, ZM=94, Z0=95),
    "far": dict(_HEAD_ROLES, KH=300, ZM=510, Z0=511, **_FAR_ROLES, KF=900, LM=1098, L=1099),
    "wide": dict(_HEAD_ROLES, KH=300, ZM=510, Z0=511, **_FAR_ROLES, XM=4094, X0=4095, X1=4096, X2=4097, KF=4200,
                 LM=4298, L=4299),
}
KEEPERS = ("KH", "KF")  # no tick touches them
# closed nodes next to the edges that `head` changes to reach 16 (they decide nothing: see TICKS)
PADS = {"head": dict(N3=3, N4=4, N61=61, N67=67, N68=68, N92=92, N93=93), "far": {}, "wide": {}}
# The base pod of this closed node also asks for 2 GiB of memory and 4 GiB + 1 MiB of ephemeral storage, so
# that the pool's smallest memory and ephemeral values never move.  (A value that becomes or stops being a
# dimension's smallest re-points every pod that asks for less: hundreds of pod patches in one call's copy,
# which in a pool as small as `head` outgrow the device arena; a new arena holds no candidate section, so
# that tick runs K0 on every row -- the host is right to, but the script is about the ticks that do not.)
NE = 90

FILLERS = {
    "c100": Container(cpu_milli=100), "c200": Container(cpu_milli=200), "c300": Container(cpu_milli=300),
    "c400": Container(cpu_milli=400), "c401": Container(cpu_milli=401), "c700": Container(cpu_milli=700),
    "c701": Container(cpu_milli=701), "c1050": Container(cpu_milli=1050),
    "m": Container(memory=GiB + MiB), "m1g": Container(memory=GiB), "m1gm1": Container(memory=GiB - 1),
    "mp": Container(memory=600 * MiB),
    "e": Container(ephemeral=4 * GiB + MiB), "z": Container(),
}


def _sel(tier):
    return {} if tier is None else {"tier": tier}


def _pod(name, tier, **req):
    ports = [ContainerPort(host_port=req.pop("port"))] if "port" in req else []
    return Pod(name, containers=[Container(ports=ports, **req)], node_selector=_sel(tier))


KINDS = {
    "cpu": dict(cpu_milli=600), "port": dict(cpu_milli=300, port=8080), "mem": dict(cpu_milli=100, memory=3 * GiB),
    "modd": dict(cpu_milli=100, memory=3 * GiB + 1), "eph": dict(cpu_milli=100, ephemeral=6 * GiB),
    "c1": dict(cpu_milli=100, memory=3 * GiB + 512 * MiB),
}


def _comb(name, tier, kind, n):
    return [_pod("%s-%d" % (name, k), tier, **KINDS[kind]) for k in range(n)]


def _ext(name, tier, n):
    """An init-container pod (fit request 600m, 100m accounted: an extension record) and n cpu-kind pods: the
    node that takes the first pod has 900m left of 1000m and takes the second as well."""
    first = Pod(name + "-init", containers=[Container(cpu_milli=100)], init_containers=[Container(cpu_milli=600)],
                node_selector=_sel(tier))
    return [first] + _comb(name, tier, "cpu", n)


def _edge(name, tier):
    """(e): an all-zero pod, then a memory-only one (cpu 0, 1 GiB)."""
    return [Pod(name + "-zero", containers=[Container()], node_selector=_sel(tier)),
            Pod(name + "-memonly", containers=[Container(memory=GiB)], node_selector=_sel(tier))]


HEAVY_LANES = tuple(range(0, 8)) + tuple(range(27, 36)) + (63,)


def _big(name, n, n_comb):
    """n pods: memory-only crumbs (cpu 0, 1 MiB: on the first nodes that are not overcommitted in cpu, 110 pod
    slots each), then the cpu comb, whose pods have indices >= n - n_comb.  The crumbs in the lanes the comb
    pods have in their own pod groups are heavy (cpu 0, 3.5 GiB: one per node): they do not fit B0 once it
    holds m1g, where the comb pods do, so a comb pod that read a lower group's fit mask would pass B0 by."""
    crumbs = [Pod("%s-crumb%d" % (name, k), containers=[Container(
        memory=3 * GiB + 512 * MiB if k % 64 in HEAVY_LANES else MiB)]) for k in range(n - n_comb)]
    return crumbs + _comb(name, None, "cpu", n_comb)


N_ANY = {"head": 6, "far": 9, "wide": 9}  # pods of the combs without selector


def candidates(pool: str, big: bool = True):
    """[(name, pods)]; `big`: with the 100- and the 200-pod candidate (two and four pod groups)."""
    n = N_ANY[pool]
    out = [("comb_any", _comb("comb_any", None, "cpu", n)),
           ("comb_head", _comb("comb_head", "head", "cpu", 6)),
           ("pair_any", _comb("pair_any", None, "cpu", 2)),
           ("port_any", _comb("port_any", None, "port", 9)),
           ("mem_any", _comb("mem_any", None, "mem", 9)),
           ("eph_head", _comb("eph_head", "head", "eph", 8)),
           ("g_head", _comb("g_head", "head", "eph", 11)),  # one pod per open head node
           ("ext_any", _ext("ext_any", None, n - 1)),
           ("edge_any", _edge("edge_any", None)),
           ("spill_head", _comb("spill_head", "head", "cpu", 12))]  # more pods than the head has open nodes
    for p in out[2][1]:
        p.containers[0].cpu_milli = 450  # the pair: two fit an empty node, one a node with 200m used
    if pool != "head":
        n_far = len([r for r in ROLES[pool] if ROLES[pool][r] >= HEAD_NODES])
        pair = _comb("pair_far", "far", "cpu", 2)
        for p in pair:
            p.containers[0].cpu_milli = 450
        out += [("comb_far", _comb("comb_far", "far", "cpu", 5)),
                ("pair_far", pair),
                ("modd_far", _comb("modd_far", "far", "modd", 5)),
                ("eph_far", _comb("eph_far", "far", "eph", 5)),
                ("g_far", _comb("g_far", "far", "eph", n_far)),  # one pod per open far node
                ("ext_far", _ext("ext_far", "far", 4)),
                ("edge_far", _edge("edge_far", "far"))]
    if pool == "wide":
        out.append(("c1_far", _comb("c1_far", "far", "c1", 2)))
    if big:
        out += [("big100", _big("big100", 100, n)), ("big200", _big("big200", 200, n))]
    return out


# ------------------------------------------------------------------ the ticks
def _ticks(pool: str) -> List[Dict[str, List[str]]]:
    far = pool != "head"
    wide = pool == "wide"
    mp = {r: ["mp"] for r in ("F0", "F1", "Q0", "Q1", "XM", "X0")} if wide else {}

    def tick(**fill):
        out = {r: list(v) for r, v in mp.items()}
        for r, v in fill.items():
            if r in ROLES[pool] or r in PADS[pool]:
                out[r] = out.get(r, []) + v
        return out

    # table time: closed for the cpu kind B0, B1, F0, Q0, for cpu and port ZM, for the memory kinds A1, P0, X1,
    # for eph L
    s = dict(B0=["c401"], B1=["c401"], ZM=["c701"], A1=["m"], F0=["c401"], Q0=["c401"], L=["e"], X1=["m"],
             P0=["m"])
    ticks = [tick(**s), tick(**s)]                                   # t0, t1: cold

    def step(**chg):
        # a pad's filler stays for one tick: when more than an eighth of a pool changes at once the encoder
        # rebuilds its state view and every row is rewritten, and `head` is to stay below that at t13
        for r in [r for r in s if r in PADS[pool]]:
            del s[r]
        for r, v in chg.items():
            if v:
                s[r] = v
            else:
                s.pop(r, None)
        ticks.append(tick(**s))

    step(A0=["c200"], B0=["c400", "m1g"], X2=["m"])                # t2
    step(F0=["c400"], Q0=["c400"], X1=[])                          # t3
    step(B1=["c300"], ZM=["c700"], P0=["m1g"])                     # t4
    step(A0=["c401"], B2=["c701"], P0=["m1gm1"])                   # t5: A0, P0 a second time; B0 (t2), A0 both decide
    step(F0=["c100"], Z0=["e"], N3=["c401"], N4=["m"])             # t6
    step(F0=["c100", "m1g"], L=[], A1=["m1g"])                     # t7
    step(A0=["c1050"], Z0=[], Q0=["c400", "e"], P0=["m1gm1", "c401"], N61=["e"])  # t8
    step(F0=["c1050"], Q1=["c401"], LM=["c401"], N67=["z"], N68=["c100"])  # t9
    if pool == "wide":                                             # t10: up to 16 changed nodes
        step(A0=["c401"], F0=["c100"], Q0=["c400"], X0=["c401", "z"])  # (X0 = 4,095: its only change)
    else:
        step(A0=["c401"], F0=["c100"], Q0=["c400"], F1=["z", "c401"], A2=["c401"], BM=["m"], N92=["c401"],
             N93=["m1g"])
    step(B3=["c401"])                                              # t11: the 17th
    step(L=["e"]) if far else step(Z0=["e"])                       # t12: one more, against the new tables
    ticks.append({})                                               # t13: every filler leaves
    return ticks


TICKS = {pool: _ticks(pool) for pool in POOLS}
N_TICKS = 14
# the tick whose state the tables K2 reads were last written from (a tick that runs K0 writes them)
TABLES_OF = {t: (1 if t <= 11 else 11) for t in range(2, 13)}
K0_LESS = tuple(range(2, 11)) + (12,)   # ticks that launch no K0 under the default form
K0_TICK = 11                            # the 17th changed node: K0 runs


def changed_nodes(pool: str, since: int, tick: int):
    """Nodes whose filler state at some tick in (since, tick] differs from the tick before: what the planner
    has accumulated at `tick` when its tables are those of `since`."""
    out = set()
    tk = TICKS[pool]
    for t in range(since + 1, tick + 1):
        for r in set(tk[t]) | set(tk[t - 1]):
            if tk[t].get(r, []) != tk[t - 1].get(r, []):
                out.add(node_of(pool, r))
    return out


def node_of(pool: str, role):
    if role is None or isinstance(role, int):
        return role
    return ROLES[pool][role] if role in ROLES[pool] else PADS[pool][role]


# ------------------------------------------------------------------ the matrix
SITUATIONS = {
    "a": "f0 >= r > f1: the pod moves on", "b_exact": "f0 < r <= f1, f1 == r",
    "b": "f0 < r <= f1", "b_minus1": "f0 < r, f1 == r - 1: does not fit (guard)",
    "b_inside": "f0 < r <= f1 < the row's old threshold",
    "c": "the node opens up, the pod's selector refuses it (guard)",
    "d": "the first pod still fits the node, the second no more", "d_grew": "the node grew and takes two pods",
    "e_zero": "all-zero request on an overcommitted node: fits (guard)",
    "e_memonly": "cpu 0, memory > 0 on a node overcommitted in cpu: refused",
    "f_mem": "the change is in memory only", "f_eph": "the change is in ephemeral storage only",
    "g_fail": "status OK -> failing pod index", "g_ok": "status failing pod index -> OK",
}
GUARDS = ("b_minus1", "c", "e_zero")
SITES = ("head_w0", "head_w1_7", "far_scan_c0", "far_scan_c1", "far_move", "group1", "group2_3", "ext", "port",
         "mem32", "mem64")
# far_window: a far window an earlier pod of the candidate resolved (not a required site of its own)
FAR_SITES = ("far_scan_c0", "far_scan_c1", "far_move", "far_window")
# candidates whose every decisive entry also counts for a site of its own
CAND_SITE = {"big100": "group1", "big200": "group2_3", "ext_any": "ext", "ext_far": "ext", "port_any": "port",
             "mem_any": "mem32", "modd_far": "mem64", "c1_far": "mem32"}

Entry = namedtuple("Entry", "pool tick cand pod before now changed site situation")
# (a node of None: the pod has no node, and the candidate's status is the pod's index)

# (pools, tick, candidate, pod, before, now, changed, site, situations); nodes as roles ({pool: role} where
# the pools differ).  `pod`: an index, "+k" for pod k of the cpu comb that ends big100 / big200, "-1" for
# the candidate's last pod.
_E = [
    # t2: A0 has 800m left: the pair's second pod moves on (window 0's running state is the patch's).  B0 has
    #     exactly 600m left (and 3 GiB of memory: not enough for the heavy crumbs of big100 / big200): the fifth
    #     comb pod comes back to it; the far class must not see it.  wide: X2
    #     closes in memory, the first fit of c1 moves from X2 to KF (both in chunk 1)
    ("head far wide", 2, "pair_any", 1, "A0", "A1", "A0", "head_w0", "d"),
    ("head far wide", 2, "comb_any", 4, "B2", "B0", "B0", "head_w0", "b_exact"),
    ("head far wide", 2, "comb_head", 4, "B2", "B0", "B0", "head_w0", "b_exact"),
    ("head far wide", 2, "ext_any", 5, "B2", "B0", "B0", "head_w0", "b_exact"),
    ("head far wide", 2, "big100", "+4", "B2", "B0", "B0", "head_w0", "b_exact"),
    ("head far wide", 2, "big200", "+3", "B2", "B0", "B0", "head_w0", "b_exact"),  # (A0 holds 110 crumbs: full)
    ("far wide", 2, "comb_far", 0, "F1", "F1", "B0", "head_w0", "c"),
    ("wide", 2, "c1_far", 0, "X2", "KF", "X2", "far_scan_c1", "a f_mem"),
    # t3: F0 has exactly 600m left: the far comb's first pod (no head node: the far scan) comes back to it.
    #     Q0 too: the comb's fourth pod finds word 8 full of the first three and moves to word 9, where Q1
    #     keeps the word non-zero whether or not Q0 fits.  The head class must not see either: the last pod
    #     of spill_head has no head node left and scans the far words.  wide: X1 is free again
    ("far wide", 3, "comb_far", 0, "F1", "F0", "F0", "far_scan_c0", "b_exact"),
    ("far wide", 3, "ext_far", 0, "F1", "F0", "F0", "far_scan_c0", "b_exact"),
    ("far wide", 3, "comb_far", 3, {"far": "KF", "wide": "XM"}, "Q0", "Q0", "far_move", "b_exact"),
    ("far wide", 3, "spill_head", "-1", None, None, "F0", "far_scan_c0", "c"),
    ("wide", 3, "c1_far", 0, "X2", "X1", "X1", "far_scan_c1", "b f_mem"),
    # t4: B1 has 700m left, inside [600, 1000); P0 has 3 GiB of memory left, one byte less than modd asks
    ("head far wide", 4, "comb_any", 5, "B3", "B1", "B1", "head_w1_7", "b_inside"),
    ("head far wide", 4, "comb_head", 5, "B3", "B1", "B1", "head_w1_7", "b_inside"),
    ("far wide", 4, "ext_any", 6, "B3", "B1", "B1", "head_w1_7", "b_inside"),
    ("head far wide", 4, "big100", "+5", "B3", "B1", "B1", "head_w1_7", "b_inside"),
    ("head far wide", 4, "big200", "+4", "B3", "B1", "B1", "head_w1_7", "b_inside"),
    ("far wide", 4, "modd_far", 2, "Q0", "Q0", "P0", "far_window", "b_minus1 f_mem"),
    # t5: A0 (changed at t2) has 599m left: every cpu comb starts at A1, and B0 (t2) and B1 (t4) take their
    #     pods as well; B2 has 299m left: the port comb's seventh pod moves on and its ninth reaches ZM,
    #     which has had exactly 300m left since t4; P0 has 3 GiB + 1 left: exactly what modd asks
    ("head far wide", 5, "comb_any", 0, "A0", "A1", "A0", "head_w0", "a"),
    ("head far wide", 5, "comb_head", 0, "A0", "A1", "A0", "head_w0", "a"),
    ("head far wide", 5, "ext_any", 0, "A0", "A1", "A0", "head_w0", "a"),
    ("head far wide", 5, "big100", "+0", "A0", "A1", "A0", "head_w0", "a"),
    ("head far wide", 5, "big200", "+3", "B2", "B0", "B2", "head_w1_7", "a"),
    ("head far wide", 5, "port_any", 6, "B2", "B3", "B2", "head_w1_7", "a"),
    ("head far wide", 5, "port_any", 8, "KH", "ZM", "ZM", "head_w1_7", "b_exact"),
    ("far wide", 5, "modd_far", 2, "Q0", "P0", "P0", "far_window", "b_exact f_mem"),
    # t6: F0 has 900m left and takes both pods of the pair; Z0, the last open head node, closes in
    #     ephemeral storage: g_head (one pod per open head node) fails at its last pod
    ("far wide", 6, "pair_far", 1, "F1", "F0", "F0", "far_window", "d_grew"),
    ("head far wide", 6, "g_head", 10, "Z0", None, "Z0", "head_w1_7", "a f_eph g_fail"),
    # t7: F0 closes in memory for modd (far: 3 GiB = r - 1 left): its first pod's far scan moves to F1; A1
    #     has exactly 3 GiB left; L, the last node, is free again in ephemeral storage: g_far drains
    ("far wide", 7, "modd_far", 0, "F0", "F1", "F0", "far_scan_c0", "a f_mem"),
    ("head far wide", 7, "mem_any", 1, "A2", "A1", "A1", "head_w0", "b_exact f_mem"),
    ("far wide", 7, "g_far", "-1", None, "L", "L", "far_window", "b f_eph g_ok"),
    # t8: A0 is overcommitted in cpu (-50m): the all-zero pod stays, the memory-only pod and the crumbs go to
    #     A1; Q0 closes in ephemeral storage: the eph comb's fourth pod (word 8 full) moves on to Q1
    ("head far wide", 8, "edge_any", 0, "A0", "A0", "A0", "head_w0", "e_zero"),
    ("head far wide", 8, "edge_any", 1, "A0", "A1", "A0", "head_w0", "e_memonly"),
    ("head far wide", 8, "big100", 10, "A0", "A1", "A0", "head_w0", "e_memonly"),
    ("far wide", 8, "eph_far", 3, "Q0", "Q1", "Q0", "far_move", "a f_eph"),
    # t9: the same on F0
    ("far wide", 9, "edge_far", 0, "F0", "F0", "F0", "far_scan_c0", "e_zero"),
    ("far wide", 9, "edge_far", 1, "F0", "F1", "F0", "far_scan_c0", "e_memonly"),
    # t10: BM closes in memory (head, far)
    ("head far", 10, "mem_any", 2, "BM", "A2", "BM", "head_w0", "a f_mem"),
    # wide: node 4,095 closes for the cpu kind: the far comb's fifth pod crosses the chunk edge
    ("wide", 10, "comb_far", 4, "X0", "X1", "X0", "far_window", "a"),
    # t11, the tick that runs K0: B3 has 599m left
    ("head far", 11, "comb_any", 5, "B3", "Z0", "B3", "head_w1_7", "a"),
    ("wide", 11, "comb_any", 5, "B3", "KH", "B3", "head_w1_7", "a"),
    # t12, against the tables of t11: the pool's last open node closes in ephemeral storage
    ("far wide", 12, "g_far", "-1", "L", None, "L", "far_window", "a f_eph g_fail"),
    ("head", 12, "g_head", 10, "Z0", None, "Z0", "head_w1_7", "a f_eph g_fail"),
]


def entries(pool: str) -> List[Entry]:
    cands = dict(candidates(pool, True))
    out = []

    def node(r):
        return node_of(pool, r[pool] if isinstance(r, dict) else r)

    for pools, tick, cand, pod, before, now, changed, site, sits in _E:
        if pool not in pools.split():
            continue
        if isinstance(pod, str):
            pod = len(cands[cand]) + int(pod) - (0 if pod[0] == "-" else N_ANY[pool])
        out.append(Entry(pool, tick, cand, pod, node(before), node(now), node(changed), site, tuple(sits.split())))
    return out


# Candidates that do not drain: {pool: {candidate: {tick: failing pod index}}}; every other status is OK.
# spill_head asks for twelve 600m head nodes, and fails at the pod after the last head node open for it;
# g_head / g_far have one pod per open node of their class and fail at the last pod while one of those nodes
# is closed for them (at the pod before it while two are: far t9, F0 overcommitted and Q0); comb_far (far:
# five pods) is left with F1 / F0, Q0, KF and L from t9 on.
def _spill(*per_tick):
    return dict(enumerate(per_tick))


FAILING = {
    "head": {"spill_head": _spill(8, 8, 9, 9, 10, 8, 8, 8, 8, 8, 7, 6, 6, 11),
             "g_head": {6: 10, 7: 10, 8: 10, 9: 10, 12: 10}},
    "far": {"spill_head": _spill(8, 8, 9, 9, 10, 8, 8, 8, 8, 8, 7, 6, 6, 11),
            "g_head": {6: 10, 7: 10, 8: 10, 9: 10},
            "g_far": {0: 7, 1: 7, 2: 7, 3: 7, 4: 7, 5: 7, 6: 7, 8: 7, 9: 6, 12: 7},
            "comb_far": {9: 4, 10: 4, 11: 4, 12: 4}},
    "wide": {"spill_head": _spill(8, 8, 9, 9, 10, 8, 8, 8, 8, 8, 8, 7, 7, 11),
             "g_head": {6: 10, 7: 10, 8: 10, 9: 10},
             "g_far": {0: 11, 1: 11, 2: 11, 3: 11, 4: 11, 5: 11, 6: 11, 8: 11, 9: 10, 12: 11}},
}


def expected_status(pool: str, tick: int, cand: str) -> int:
    return FAILING[pool].get(cand, {}).get(tick, -1)  # SR_CAND_OK == -1


# ------------------------------------------------------------------ the encoded input
class PoolInput:
    """One pool's cluster (built once per process): nodes, base pods, every probe pod and one pod per filler
    kind, with pod stamps (without them the encoder never reuses the candidate side)."""

    def __init__(self, pool: str):
        self.pool = pool
        n = POOLS[pool]
        open_nodes = set(ROLES[pool].values())
        nodes = [Node("n%d" % i, cpu_milli=1000, memory=4 * GiB, ephemeral=10 * GiB, pods=110,
                      labels={"kubernetes.io/hostname": "n%d" % i, "tier": "head" if i < HEAD_NODES else "far"})
                 for i in range(n)]
        spot_pods = [[] if i in open_nodes else [Pod("base%d" % i, containers=[Container(cpu_milli=950)])]
                     for i in range(n)]
        spot_pods[NE][0].containers[0].memory = 2 * GiB
        spot_pods[NE][0].containers[0].ephemeral = 4 * GiB + MiB
        self.cands = candidates(pool, True)
        flat = [p for _, ps in self.cands for p in ps]
        self.filler_names = sorted(FILLERS)
        fillers = [Pod("filler-" + f, containers=[FILLERS[f]]) for f in self.filler_names]
        n_pods = sum(len(ps) for ps in spot_pods) + len(flat) + len(fillers)
        stamps = [(1 << 63) | (zlib.crc32(("steady-" + pool).encode()) << 24) | (i + 1) for i in range(n_pods)]
        self.sc = Scenario(nodes, spot_pods, flat + fillers, stamps=stamps)
        self.filler_pod = {f: self.sc.qidx(len(flat) + k) for k, f in enumerate(self.filler_names)}
        self.first = {}
        k = 0
        for name, ps in self.cands:
            self.first[name] = k
            k += len(ps)

    def candidate_arrays(self, big: bool = True, ext: bool = True):
        """(names, cand_off, cand_pods) with or without the two large candidates, and with or without the
        candidates that have extension records (a launch with those has no cooperative blocks); the same
        pods either way."""
        names = [nm for nm, _ in self.cands
                 if (big or not nm.startswith("big")) and (ext or not nm.startswith("ext"))]
        sizes = [len(dict(self.cands)[nm]) for nm in names]
        cand_off = np.cumsum([0] + sizes).astype(np.int32)
        cand_pods = np.concatenate([np.arange(self.sc.qidx(self.first[nm]), self.sc.qidx(self.first[nm]) + m)
                                    for nm, m in zip(names, sizes)]).astype(np.int32)
        return names, cand_off, cand_pods

    def fillers_of(self, tick: int):
        """[(pod index, spot position)] of tick `tick`, in a fixed order."""
        out = []
        for role in sorted(TICKS[self.pool][tick], key=lambda r: node_of(self.pool, r)):
            for f in TICKS[self.pool][tick][role]:
                out.append((self.filler_pod[f], node_of(self.pool, role)))
        return out


_inputs: Dict[str, PoolInput] = {}


def get_pool(pool: str) -> PoolInput:
    if pool not in _inputs:
        _inputs[pool] = PoolInput(pool)
    return _inputs[pool]
