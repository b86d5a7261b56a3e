"""Inputs and hand-derived plans for K2's domain path (kernels.hip k2_domain,
antiaff.cpp, encode.cpp analyse_spread) at its limits: domain ids up to 63 of
a shared key, the four key slots, four terms per affinity set, two interacting
spread constraints per pod, and pools of more than one 4,096-node chunk.
test_domain_limits_reference.py asserts every plan and its preconditions on
the oracle, test_gpu_domain_limits.py runs them through the C ABI.

A `Call` is one candidate list planned in one call (key slots are per call);
a `Cand` one candidate with the node of every pod (`want`, -1 from the failing
pod `fail` on), written out with its derivation.  `fallback`: one step over a
limit, the planner must answer SR_CAND_FALLBACK (the oracle plans it, except
beyond a spread limit, which it mirrors: `oracle_too`).
`decided` maps a pod of the candidate to (the open node it takes when its
refusal / requirement / minimum is dropped, the id of the domain that decides
it or None).  The rules are those of domain_cases.py; topology spread
(PodTopologySpread.Filter, k8s v1.19.2): with c[v] the selected pods in the
pair of value v and m the minimum over the pairs, a node of value v passes
when c[v] + self - m <= maxSkew; a node without the key never passes, and the
selected pods on such nodes count into the pair of "" when it exists.

Pool z64: 192 nodes s000..s191 in NodeInfoArray order, node n in zone
"z%02d" % (n // 3) -- the planner numbers a key's values by first appearance,
so zone id == n // 3 and zone 21 spans row words 0 | 1 -- and with rack n % 2,
team n % 3, region n // 96, cell n % 5 and its hostname.  The first node of
zones 1, 6, .., 61 is full (a base pod): fo(z) is a zone's first open node, and
every zone keeps two open nodes.  Base web pods (one per zone on its last node,
none in zones 40 and 63) are what the spread cases count.  Three term-less
pods (PRE) in front of each candidate land on node 0 and keep pod index, lane
and domain id apart.
  z65:  z64 and node s192 in a 65th zone.
  z63k: nodes 189..191 without the zone key (63 zones).
  z63e: node 189 with zone "" (the 64th value, id 63), 190 / 191 without the
        key, a base web pod on 191 that counts into the pair of "".

Pools wide2 (4,300 nodes, 68 row words) and wide3 (8,300 nodes, 130 row words,
three chunks): every node closed -- even ones unschedulable (S rows), odd ones
without free cpu (T rows) -- except
  62 63 64 65 4094 4095 4096   zone za, roomy (4096 is the first node of chunk 1)
  4097                         zone zb
  wide2:  4298  no zone, room for two pods (pod count);  4299  zone zd
  wide3:  8190  no zone, room for two pods (pod count)   (chunk 1)
          8191  zone zc                                  (chunk 1)
          8192  no zone, cpu for two pods                (chunk 2)
          8193  no zone, roomy                           (chunk 2)
          8298  zone zd;  8299  no zone, room for one pod
Closed nodes carry zone "z" + "abcd"[n % 4], so zd's only open node is in the
last chunk.  Chunk 1 begins at node 4,096 (row word 64), chunk 2 at 8,192 (row
word 128).

Every pool is built once per process, with all its calls' pods as unbound
pods of one encoding and pod stamps."""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from domain_cases import H, pod, term
from helpers import Scenario
from oracle_lib import oracle_plan
from scenario_gen import req, spread, zc
from scenario_gen import term as node_term
from sequence_ref import SeqInput, from_scenario
from spotplanner.model import Container, ContainerPort, LabelSelector, Node, Pod

Z, RACK, TEAM, REGION, CELL = "zone", "rack", "team", "region", "cell"
N_PRE = 3
NO_WEB = (40, 63)  # zones without a base web pod


@dataclass
class Cand:
    name: str
    why: str
    pods: List[Pod]
    want: Optional[List[int]]
    fail: int = -1
    fallback: bool = False
    oracle_too: bool = False  # a spread limit, which the oracle mirrors (its o_spread_dyn_fallback): FALLBACK there too
    decided: Dict[int, Tuple[int, Optional[int]]] = field(default_factory=dict)
    high: bool = False  # claims a deciding domain id >= 31 for every entry of `decided`


@dataclass
class Call:
    name: str
    cands: List[Cand]


def fo(z: int) -> int:
    """z64: the first open node of zone z."""
    return 3 * z + (1 if z % 5 == 1 else 0)


def sname(n: int) -> str:
    return "s%03d" % n


def pre(tag: str) -> List[Pod]:
    return [pod("pre-%s-%d" % (tag, i), "pre") for i in range(N_PRE)]


def zones_only(p: Pod, *zones: int) -> Pod:
    p.required_node_affinity = [node_term(req(Z, "In", *["z%02d" % z for z in zones]))]
    return p


def sel(app) -> LabelSelector:
    return LabelSelector(match_labels={"app": app})


# ------------------------------------------------------------------ the 192-node pools
def z_nodes(keyless=(), empty=(), extra=0) -> List[Node]:
    nodes = []
    for n in range(192 + extra):
        labels = {H: sname(n), RACK: "r%d" % (n % 2), TEAM: "t%d" % (n % 3), REGION: "g%d" % (n // 96),
                  CELL: "c%d" % (n % 5)}
        if n in empty:
            labels[Z] = ""
        elif n not in keyless:
            labels[Z] = "z%02d" % (n // 3)
        nodes.append(Node(sname(n), cpu_milli=8000, pods=110, labels=labels))
    return nodes


def z_base(n_nodes, web_zones, web_nodes=()) -> List[List[Pod]]:
    base = [[] for _ in range(n_nodes)]
    for z in range(1, 64, 5):
        base[3 * z].append(Pod("full%d" % z, labels={"app": "filler"}, containers=[Container(cpu_milli=8000)]))
    for n in [3 * z + 2 for z in web_zones] + list(web_nodes):
        base[n].append(pod("bw%d" % n, "web"))
    return base


def _rep(tag, i, on=None) -> Pod:
    return pod("%s-%d" % (tag, i), "rep-" + tag, anti=[term(Z, "rep-" + tag)], on=on)


def _web(tag, i, *cs, **kw) -> Pod:
    p = spread(pod("%s-%d" % (tag, i), "web"), *cs)
    p.node_selector = dict(kw)
    return p


P0 = [0] * N_PRE  # the PRE pods: term-less, the pool's first open node


def anti_cands() -> List[Cand]:
    out = [
        Cand("anti64", "replica r refuses zones 0..r-1 (every earlier replica's): fo(r); 67 pods, two pod groups",
             pre("a64") + [_rep("a64", i) for i in range(64)], P0 + [fo(z) for z in range(64)],
             decided={N_PRE + r: (0, r - 1) for r in range(32, 64)}, high=True),
        Cand("anti65", "as anti64; replica 64 finds all 64 zones refused and every node has a zone: fails (pod 67)",
             pre("a65") + [_rep("a65", i) for i in range(65)], P0 + [fo(z) for z in range(64)] + [-1], fail=N_PRE + 64,
             decided={N_PRE + 64: (0, 63)}, high=True),
        Cand("anti64_one_group", "replica 0 pinned to s189 (zone 63); replica k refuses zones 63, 0..k-2: fo(k-1); "
             "64 pods, one pod group, lane k against domain k-1",
             [_rep("a1g", 0, on=sname(189))] + [_rep("a1g", i) for i in range(1, 64)],
             [189] + [fo(k - 1) for k in range(1, 64)], decided={k: (0, k - 2) for k in range(33, 64)}, high=True),
    ]
    for zz in (31, 32, 33, 62):
        d, x = 3 * zz + 2, 3 * zz + 2
        out.append(Cand(
            "both_%d" % zz, "d pinned to s%03d (zone %d); w (zones %d | %d only) has a term selecting d: zone %d "
            "refused -> fo(%d); x pinned there has a term selecting y (same zones): -> fo(%d)" % (d, zz, zz, zz + 1, zz,
                                                                                                  zz + 1, zz + 1),
            pre("b%d" % zz) + [pod("d%d" % zz, "db", on=sname(d)),
                               zones_only(pod("w%d" % zz, "wb", anti=[term(Z, "db")]), zz, zz + 1),
                               pod("x%d" % zz, "xw", anti=[term(Z, "xd")], on=sname(x)),
                               zones_only(pod("y%d" % zz, "xd"), zz, zz + 1)],
            P0 + [d, fo(zz + 1), x, fo(zz + 1)], decided={N_PRE + 1: (fo(zz), zz), N_PRE + 3: (fo(zz), zz)}, high=True))
    out += [
        Cand("both_63_incoming", "d pinned to s191 (zone 63); w may only run in zone 63, which its term refuses: fails",
             pre("b63i") + [pod("d63", "db", on=sname(191)), zones_only(pod("w63", "wb", anti=[term(Z, "db")]), 63)],
             P0 + [191, -1], fail=N_PRE + 1, decided={N_PRE + 1: (189, 63)}, high=True),
        Cand("both_63_existing", "x pinned to s191 has a term selecting y, which may only run in zone 63: fails",
             pre("b63e") + [pod("x63", "xw", anti=[term(Z, "xd")], on=sname(191)), zones_only(pod("y63", "xd"), 63)],
             P0 + [191, -1], fail=N_PRE + 1, decided={N_PRE + 1: (189, 63)}, high=True),
    ]
    return out


def aff_cands() -> List[Cand]:
    out = []
    for zz in (31, 32, 61, 63):
        c = 3 * zz + 2
        out.append(Cand("follow_%d" % zz, "c pinned to s%03d; w needs a cache pod in its zone: zone %d -> fo(%d)%s" % (
            c, zz, zz, ", its second node" if zz % 5 == 1 else ""),
            pre("f%d" % zz) + [pod("c%d" % zz, "cache", on=sname(c)), pod("w%d" % zz, "fw", aff=[term(Z, "cache")])],
            P0 + [c, fo(zz)], decided={N_PRE + 1: (0, zz)}, high=True))
    out += [
        Cand("self_exception_63", "s1 pinned to s190: empty pair map and it matches its own term -> s190; s2 follows "
             "into zone 63 -> fo(63)",
             pre("se") + [pod("s1", "self", aff=[term(Z, "self")], on=sname(190)),
                          pod("s2", "self", aff=[term(Z, "self")])],
             P0 + [190, 189], decided={N_PRE + 1: (0, 63)}, high=True),
        Cand("two_terms_32", "c pinned to s098 matches both terms; w: zone 32 and host s098 -> s098 (zone alone: s096)",
             pre("tt") + [pod("ctt", "cache", on=sname(98)),
                          pod("wtt", "fw", aff=[term(Z, "cache"), term(H, "cache")])],
             P0 + [98, 98], decided={N_PRE + 1: (96, 32)}, high=True),
    ]
    return out


def _replicas(tag, n, *cs, **kw) -> List[Pod]:
    return pre(tag) + [_web(tag, i, *cs, **kw) for i in range(n)]


def spread_cands() -> List[Cand]:
    zone1 = zc(1, key=Z)
    return [
        Cand("spread_skew1", "base c = 1 but zones 40, 63 (0).  r0: m = 0, only c <= 0 passes: zone 40 -> s120; r1: "
             "zone 63 -> s189; then every c = 1 = m: r(2+j) -> fo(j), which makes c[j] = 2 > m, for j = 0..63; "
             "then every c = 2 = m: fo(0), fo(1)",
             _replicas("s1", 68, zone1), P0 + [120, 189] + [fo(j) for j in range(64)] + [fo(0), fo(1)],
             decided={N_PRE: (0, 40), N_PRE + 1: (0, 63)}, high=True),
        Cand("spread_skew2", "c <= m + 1 passes.  m = 0 while zone 63 has none: r(j) -> fo(j), which makes c[j] = 2, "
             "for j = 0..39; zone 40 passes twice (0, 1): s120, s120; fo(41)..fo(62); zone 63 once: s189, now m = 1 "
             "and c <= 2 passes: fo(0) (c = 3), fo(1)",
             _replicas("s2", 67, zc(2, key=Z)),
             P0 + [fo(j) for j in range(40)] + [120, 120] + [fo(j) for j in range(41, 63)] + [189, fo(0), fo(1)],
             decided={N_PRE + 1: (0, 63)}, high=True),
        Cand("spread_pairs_32_up", "region g1 only: the pairs are zones 32..63 (no id below 32).  m = 0: s120, s189; "
             "then m = 1: fo(32)..fo(63); then m = 2: fo(32)",
             _replicas("sh", 35, zone1, **{REGION: "g1"}), P0 + [120, 189] + [fo(j) for j in range(32, 64)] + [fo(32)],
             decided={N_PRE: (96, 40), N_PRE + 1: (96, 63)}, high=True),
        Cand("spread_zone_and_host", "zone as spread_skew1; hostname (m = 0 on 130 nodes) refuses every node with a "
             "web pod: s120, s189, then fo(j) -- s121 and s190 for j = 40, 63, whose first node holds r0 / r1 -- "
             "then zone 0 again, s000 holds r2: s001",
             _replicas("zh", 67, zone1, zc(1, key=H)),
             P0 + [120, 189] + [fo(j) + (1 if j in NO_WEB else 0) for j in range(64)] + [1],
             decided={N_PRE + 2 + 40: (120, 40), N_PRE + 2 + 63: (189, 63)}, high=True),
        Cand("spread_three_constraints", "a third interacting constraint (rack): beyond the two spread slots",
             _replicas("s3", 3, zone1, zc(1, key=H), zc(1, key=RACK)), None, fallback=True, oracle_too=True),
    ]


def plain_cand(tag) -> Cand:
    return Cand("plain_" + tag, "no terms: the first open node", pre(tag), list(P0))


def value_cands(n_zones: int) -> List[Cand]:
    """The same candidates on 64 and on 65 zones: the ones interacting through the zone key fall back on 65."""
    over = n_zones > 64
    t = "v%d" % n_zones
    return [
        Cand("anti_zone", "r0 -> s000; r1: zone 0 refused -> fo(1)",
             pre(t + "a") + [_rep(t, i) for i in range(2)], P0 + [0, fo(1)], fallback=over),
        Cand("follow_zone", "c pinned to s098; w follows into zone 32 -> fo(32)",
             pre(t + "f") + [pod("c" + t, "cache", on=sname(98)), pod("w" + t, "fw", aff=[term(Z, "cache")])],
             P0 + [98, 96], fallback=over),
        Cand("spread_zone", "m = 0 in zones 40 and 63: s120, s189; then m = 1: s000",
             _replicas(t + "s", 3, zc(1, key=Z)), None if over else P0 + [120, 189, 0], fallback=over, oracle_too=over),
        Cand("anti_team", "teams n % 3: s000, s001, s002; the fourth finds every team refused: fails",
             pre(t + "t") + [pod("%s-tm%d" % (t, i), "tm", anti=[term(TEAM, "tm")]) for i in range(4)],
             P0 + [0, 1, 2, -1], fail=N_PRE + 3),
        Cand("static_one", "a term against the base web pods only: the first open node of a zone without one, s120",
             [pod("sw" + t, "sw", anti=[term(Z, "web")])], [120]),
        Cand("static_two", "two such pods, neither selected by the other's term: both s120",
             [pod("su%s-%d" % (t, i), "su", anti=[term(Z, "web")]) for i in range(2)], [120, 120]),
        plain_cand(t),
    ]


KEY_SECOND = {Z: 4, RACK: 1, TEAM: 1, REGION: 96, CELL: 1}


def key_cand(key, tag="") -> Cand:
    t = "k" + key + tag
    return Cand("anti_" + key, "k1 -> s000; k2: s000's %s refused -> s%03d" % (key, KEY_SECOND[key]),
                pre(t) + [pod("%s-%d" % (t, i), t, anti=[term(key, t)]) for i in range(2)], P0 + [0, KEY_SECOND[key]],
                decided={N_PRE + 1: (0, None)})


def all4_cand(tag="") -> Cand:
    t = "all4" + tag
    terms = [term(k, t) for k in (Z, RACK, TEAM, REGION)]
    return Cand("anti_all_four", "b1 -> s000; b2: zone 0, rack 0 (even), team 0 (n % 3 == 0) and region 0 (n < 96) "
                "refused -> s097 (without the region term: s005)",
                pre(t) + [pod("%s-%d" % (t, i), t, anti=list(terms)) for i in range(2)], P0 + [0, 97],
                decided={N_PRE + 1: (5, None)})


def host_aff_cand(tag="") -> Cand:
    return Cand("aff_hostname", "c pinned to s100; w needs a cache pod on its node -> s100",
                pre("ha" + tag) + [pod("cha" + tag, "cache", on=sname(100)),
                                   pod("wha" + tag, "fw", aff=[term(H, "cache")])],
                P0 + [100, 100], decided={N_PRE + 1: (0, None)})


def region_aff_cand(tag="") -> Cand:
    return Cand("aff_region", "c pinned to s100; w follows into region g1 -> s096",
                pre("ra" + tag) + [pod("cra" + tag, "cache", on=sname(100)),
                                   pod("wra" + tag, "fw", aff=[term(REGION, "cache")])],
                P0 + [100, 96])


def fallen(c: Cand) -> Cand:
    c.fallback = True
    return c


def term_cands() -> List[Cand]:
    keys4 = (Z, RACK, TEAM, H)
    return [
        Cand("aff_four_terms", "c pinned to s098 matches all four terms; w: zone 32, rack 0, team 2, host s098 -> s098",
             pre("t4") + [pod("ct4", "cache", on=sname(98)), pod("wt4", "fw", aff=[term(k, "cache") for k in keys4])],
             P0 + [98, 98], decided={N_PRE + 1: (0, 32)}),
        Cand("aff_five_terms", "a fifth term (region): beyond the four terms of a set",
             pre("t5") + [pod("ct5", "cache", on=sname(98)),
                          pod("wt5", "fw", aff=[term(k, "cache") for k in keys4 + (REGION,)])],
             P0 + [98, 98], fallback=True),
        plain_cand("t"),
    ]


def z64_calls() -> List[Call]:
    return [
        Call("main", anti_cands() + aff_cands() + spread_cands() + [plain_cand("m")]),
        Call("values", value_cands(64)),
        # key slots are taken in candidate order, anti-affinity before affinity
        Call("keys_forward", [key_cand(Z), key_cand(RACK), key_cand(TEAM), key_cand(REGION), all4_cand(),
                              fallen(key_cand(CELL)), plain_cand("kf")]),
        Call("keys_reverse", [key_cand(CELL, "r"), key_cand(REGION, "r"), key_cand(TEAM, "r"), key_cand(RACK, "r"),
                              fallen(key_cand(Z, "r")), fallen(all4_cand("r")), plain_cand("kr")]),
        Call("keys_hostname_fourth", [host_aff_cand(), key_cand(Z, "h"), key_cand(RACK, "h"), key_cand(TEAM, "h")]),
        Call("keys_hostname_fifth", [host_aff_cand("5"), key_cand(Z, "h5"), key_cand(RACK, "h5"), key_cand(TEAM, "h5"),
                                     fallen(region_aff_cand("5")), plain_cand("kh")]),
        Call("keys_four_a", [key_cand(Z, "a"), key_cand(RACK, "a"), key_cand(TEAM, "a"), key_cand(REGION, "a")]),
        Call("keys_four_b", [key_cand(CELL, "b"), key_cand(Z, "b"), key_cand(RACK, "b"), key_cand(TEAM, "b")]),
        Call("terms", term_cands()),
    ]


def z63k_calls() -> List[Call]:
    return [Call("main", [
        Cand("anti_spill", "63 replicas take the 63 zones; the next two find every zone refused and land on s189, "
             "which has no zone: neither's term has a pair there",
             pre("k65") + [_rep("k65", i) for i in range(65)], P0 + [fo(z) for z in range(63)] + [189, 189],
             decided={N_PRE + 63: (0, 62), N_PRE + 64: (0, 62)}, high=True),
        Cand("anti_from_keyless", "r0 pinned to s190 (no zone): its term has no pair; r1 -> s000",
             pre("kk") + [_rep("kk", 0, on=sname(190)), _rep("kk", 1)], P0 + [190, 0]),
        plain_cand("k"),
    ])]


def z63e_calls() -> List[Call]:
    return [Call("main", [
        Cand("spread_empty_value", "pairs: zones 0..62 and \"\" (s189, id 63); c = 1 but zone 40 (0); the web pod on "
             "s191 (no key) counts into \"\": 1.  r0: m = 0 -> s120; then m = 1: fo(0)..fo(62), s189; then m = 2: s000 "
             "(without that pod \"\" has 0 and r1 -> s189)",
             _replicas("e", 66, zc(1, key=Z)), P0 + [120] + [fo(j) for j in range(63)] + [189, 0],
             decided={N_PRE + 1: (189, 63)}, high=True),
        plain_cand("e"),
    ])]


# ------------------------------------------------------------------ the wide pools
WIDE = {"wide2": 4300, "wide3": 8300}


def wide_open(n: int) -> Dict[int, dict]:
    """Open node -> zone (None: no key), cpu, pods."""
    roomy = dict(cpu=8000, pods=110)
    o = {k: dict(zone="za", **roomy) for k in (62, 63, 64, 65, 4094, 4095, 4096)}
    o[4097] = dict(zone="zb", **roomy)
    if n > 8200:
        o[8190] = dict(zone=None, cpu=8000, pods=2)
        o[8191] = dict(zone="zc", **roomy)
        o[8192] = dict(zone=None, cpu=20, pods=110)
        o[8193] = dict(zone=None, **roomy)
        o[n - 2] = dict(zone="zd", **roomy)
        o[n - 1] = dict(zone=None, cpu=8000, pods=1)
    else:
        o[n - 2] = dict(zone=None, cpu=8000, pods=2)
        o[n - 1] = dict(zone="zd", **roomy)
    return o


def wname(n: int) -> str:
    return "s%04d" % n


def wide_nodes(n_nodes: int) -> List[Node]:
    op = wide_open(n_nodes)
    nodes = []
    for n in range(n_nodes):
        if n in op:
            labels = {H: wname(n)}
            if op[n]["zone"]:
                labels[Z] = op[n]["zone"]
            nodes.append(Node(wname(n), cpu_milli=op[n]["cpu"], pods=op[n]["pods"], labels=labels))
        else:
            labels = {H: wname(n), Z: "z" + "abcd"[n % 4]}
            nodes.append(Node(wname(n), cpu_milli=8000 if n % 2 == 0 else 5, pods=110, labels=labels,
                              unschedulable=n % 2 == 0))
    return nodes


W0 = [62] * N_PRE


def _ported(p: Pod) -> Pod:
    p.containers[0].ports = [ContainerPort(80)]
    return p


def wide3_main() -> List[Cand]:
    reps = [_rep("w3", i) for i in range(12)]
    for i in (7, 8, 10, 11):
        _ported(reps[i])
    hs_nodes = (4096, 4097, 8192, 8193, 8298, 8299)
    hs = [spread(pod("hs-%d" % i, "hs"), zc(1, sel=sel("hs"), key=H)) for i in range(6)]
    for p in hs:  # six pairs, all at the minimum, and at most five counted pods: within the node-local rule
        p.required_node_affinity = [node_term(req(H, "In", *[wname(n) for n in hs_nodes]))]
    zs = [spread(pod("zs-%d" % i, "zs"), zc(1, sel=sel("zs"), key=Z)) for i in range(5)]
    return [
        Cand("anti_chunks", "r0 -> s0062 (za, chunk 0); r1: za refused, skips s0063..s4096 (s4096 in chunk 1) -> s4097 "
             "(zb); r2, r3 -> s8190 (no zone, two pods); r4: s8190 is full -> s8191 (zc); r5: za, zb, zc refused -> "
             "s8192 (chunk 2, no zone, cpu for two); r6 -> s8192; r7 (port 80): s8192 has no cpu -> s8193; r8 (port "
             "80): the port is taken on s8193 -> s8298 (zd); r9 -> s8193; r10 (port 80): zd refused too -> s8299 (one "
             "pod); r11 (port 80): nothing left, fails",
             pre("w3") + reps, W0 + [62, 4097, 8190, 8190, 8191, 8192, 8192, 8193, 8298, 8193, 8299, -1],
             fail=N_PRE + 11,
             decided={N_PRE + 1: (63, 0), N_PRE + 3: (8191, None), N_PRE + 4: (8190, None), N_PRE + 6: (8193, None),
                      N_PRE + 7: (8192, None), N_PRE + 8: (8193, None), N_PRE + 9: (8299, None)}),
        Cand("spread_hostname", "node affinity: s4096, s4097, s8192, s8193, s8298, s8299 only, the six pairs; m = 0: a "
             "node passes while it holds no hs pod, so the replicas take them in order (s4097 because s4096 holds r0, "
             "s8193 because s8192 holds r2)",
             pre("hs") + hs, W0 + list(hs_nodes), decided={N_PRE + 1: (4096, None), N_PRE + 3: (8192, None)}),
        Cand("aff_hostname_4097", "c pinned to s4097; w needs a cache pod on its node -> s4097",
             pre("h1") + [pod("ch1", "cache", on=wname(4097)), pod("wh1", "fw", aff=[term(H, "cache")])],
             W0 + [4097, 4097], decided={N_PRE + 1: (62, None)}),
        Cand("aff_hostname_8193", "c pinned to s8193; w -> s8193",
             pre("h2") + [pod("ch2", "cache", on=wname(8193)), pod("wh2", "fw", aff=[term(H, "cache")])],
             W0 + [8193, 8193], decided={N_PRE + 1: (62, None)}),
        Cand("spread_zone_last_chunk", "zones za..zd, every c = 0.  r0 -> s0062 (za); r1: m = 0, za has 1 -> s4097 "
             "(zb); r2 -> s8191 (zc); r3: only zd is at the minimum, its one open node is s8298; r4: m = 1 -> s0062",
             pre("zs") + zs, W0 + [62, 4097, 8191, 8298, 62], decided={N_PRE + 3: (62, 3)}),
        Cand("aff_zone_last_chunk", "c pinned to s8298 (zd); w follows into zd, whose only open node is s8298",
             pre("za") + [pod("cza", "cache", on=wname(8298)), pod("wza", "fw", aff=[term(Z, "cache")])],
             W0 + [8298, 8298], decided={N_PRE + 1: (62, 3)}),
        Cand("plain_w3", "no terms: the first open node", pre("pw3"), list(W0)),
    ]


def _plain_wide(tag) -> List[Cand]:
    big = Pod("big-" + tag, labels={"app": "plain"}, containers=[Container(cpu_milli=9000)])
    return [
        Cand("plain_a", "no terms: s0062", pre("pa" + tag), list(W0)),
        Cand("plain_b", "two pods pinned to s4298 (chunk 1, beyond the S-row heads), one free -> s0062",
             [pod("pb1" + tag, "plain", on=wname(4298)), pod("pb2" + tag, "plain", on=wname(4298)),
              pod("pb3" + tag, "plain")], [4298, 4298, 62]),
        Cand("plain_c", "9,000 mcpu fit nowhere: fails at once", [big], [-1], fail=0),
    ]


def wide2_domain(tag) -> Cand:
    return Cand("anti_chunks2", "r0 -> s0062 (za); r1: za refused, skips s0063..s4096 -> s4097 (zb); r2, r3 -> s4298 "
                "(no zone, two pods); r4 -> s4299 (zd); r5: nothing left, fails",
                pre(tag) + [_rep(tag, i) for i in range(6)], W0 + [62, 4097, 4298, 4298, 4299, -1], fail=N_PRE + 5,
                decided={N_PRE + 1: (63, 0), N_PRE + 3: (4299, None)})


# wide2's later calls: the filler pod added to s4298, which then takes one more pod.  plain_b's second pod fails;
# the replicas r2, r3 no longer share s4298: r3 -> s4299 (zd), r4 finds zd refused and fails.
CHANGED_NODE = 4298
CHANGED = {"plain_b": ([4298, -1, -1], 1),
           "anti_chunks2": (W0 + [62, 4097, 4298, 4299, -1, -1], N_PRE + 4)}


def wide2_calls() -> List[Call]:
    filler = Cand("filler", "(the pod the later calls add to s4298)", [pod("fill4096", "filler")], [62])
    plain = _plain_wide("")  # the same pods in both lists
    return [Call("without", plain), Call("with", plain + [wide2_domain("w2")]), Call("filler", [filler])]


class Pool:
    def __init__(self, name, nodes, base, calls):
        self.name, self.nodes, self.base = name, nodes, base
        self.calls: Dict[str, Call] = {c.name: c for c in calls}
        seen: Dict[int, int] = {}
        flat = []
        for c in calls:  # a pod object shared by two calls (wide2's lists) is encoded once
            for cd in c.cands:
                for p in cd.pods:
                    if id(p) not in seen:
                        seen[id(p)] = len(flat)
                        flat.append(p)
        n = sum(len(b) for b in base) + len(flat)
        stamps = [(1 << 63) | (zlib.crc32(("domain-limits-" + name).encode()) << 24) | (i + 1) for i in range(n)]
        self.sc = Scenario(nodes, base, flat, stamps=stamps)
        self._index = seen
        self._oracle: Dict[str, dict] = {}

    def arrays(self, call: str):
        cands = self.calls[call].cands
        cand_off = np.cumsum([0] + [len(c.pods) for c in cands]).astype(np.int32)
        cand_pods = np.array([self.sc.q0 + self._index[id(p)] for c in cands for p in c.pods], np.int32)
        return cand_off, cand_pods

    def pod_index(self, p: Pod) -> int:
        return self.sc.q0 + self._index[id(p)]

    def oracle(self, call: str) -> dict:
        """The oracle's plan of the call from the base snapshot (computed once, never changed)."""
        if call not in self._oracle:
            cand_off, cand_pods = self.arrays(call)
            self._oracle[call] = oracle_plan(self.sc.oracle_snapshot(), self.sc.ptr, cand_off, cand_pods, mode=1,
                                             threads=8)
        return self._oracle[call]

    def open_nodes(self) -> List[int]:
        """Nodes a 10-mcpu pod without terms fits from the base snapshot."""
        out = []
        for i, n in enumerate(self.nodes):
            used = sum(p.containers[0].cpu_milli for p in self.base[i])
            if not n.unschedulable and n.cpu_milli - used >= 10 and len(self.base[i]) < n.pods:
                out.append(i)
        return out

    def domain_id(self, key: str, node: int) -> Optional[int]:
        """The id DomKeys::slot gives the node's value of `key`: values numbered by first appearance."""
        ids: Dict[str, int] = {}
        for n in self.nodes:
            if key in n.labels:
                ids.setdefault(n.labels[key], len(ids))
        v = self.nodes[node].labels.get(key)
        return None if v is None else ids[v]

    def n_values(self, key: str) -> int:
        return len({n.labels[key] for n in self.nodes if key in n.labels})


def _without_web_63():
    return [z for z in range(63) if z != 40]


BUILDERS = {
    "z64": lambda: Pool("z64", z_nodes(), z_base(192, [z for z in range(64) if z not in NO_WEB]), z64_calls()),
    "z65": lambda: Pool("z65", z_nodes(extra=1), z_base(193, [z for z in range(64) if z not in NO_WEB]),
                        [Call("values", value_cands(65))]),
    "z63k": lambda: Pool("z63k", z_nodes(keyless=(189, 190, 191)), z_base(192, _without_web_63()), z63k_calls()),
    "z63e": lambda: Pool("z63e", z_nodes(keyless=(190, 191), empty=(189,)), z_base(192, _without_web_63(), [191]),
                         z63e_calls()),
    "wide2": lambda: Pool("wide2", wide_nodes(4300), [[] for _ in range(4300)], wide2_calls()),
    "wide3": lambda: Pool("wide3", wide_nodes(8300), [[] for _ in range(8300)], [Call("main", wide3_main())]),
}
CALLS = [("z64", "main"), ("z64", "values"), ("z65", "values"), ("z64", "keys_forward"), ("z64", "keys_reverse"),
         ("z64", "keys_hostname_fourth"), ("z64", "keys_hostname_fifth"), ("z64", "keys_four_a"),
         ("z64", "keys_four_b"), ("z64", "terms"), ("z63k", "main"), ("z63e", "main"), ("wide3", "main"),
         ("wide2", "without"), ("wide2", "with")]
_pools: Dict[str, Pool] = {}


def get_pool(name: str) -> Pool:
    if name not in _pools:
        _pools[name] = BUILDERS[name]()
    return _pools[name]


# ------------------------------------------------------------------ sr_plan_sequence on wide2
@dataclass
class SeqCase:
    cands: List[Cand]  # `want`: the mapping the pass gives (an earlier drain's pods are in the snapshot)
    drained: List[int]


def sequence_cases() -> Dict[str, SeqCase]:
    def pinned(tag):
        return [pod("pin%s-%d" % (tag, i), "plain", on=wname(4298)) for i in range(2)]

    return {
        "node_order_first": SeqCase([
            Cand("pinned", "both pods pinned to s4298, which takes two: drains", pinned("a"), [4298, 4298]),
            Cand("domain", "s4298 is full now: r0 -> s0062, r1 -> s4097 (zb), r2 -> s4299 (zd): drains",
                 pre("sa") + [_rep("sa", i) for i in range(3)], W0 + [62, 4097, 4299]),
            Cand("plain", "s0062: drains", pre("sa2"), list(W0)),
        ], [0, 1, 2]),
        "domain_first": SeqCase([
            Cand("domain", "r0 -> s0062, r1 -> s4097, r2, r3 -> s4298 (no zone): drains",
                 pre("sb") + [_rep("sb", i) for i in range(4)], W0 + [62, 4097, 4298, 4298]),
            Cand("pinned", "s4298 holds r2 and r3: the first pod fails", pinned("b"), [-1, -1], fail=0),
            Cand("plain", "s0062: drains", pre("sb2"), list(W0)),
        ], [0, 2]),
    }


_seq: Dict[str, Tuple[SeqCase, SeqInput]] = {}


def get_sequence(name: str) -> Tuple[SeqCase, SeqInput]:
    if name not in _seq:
        case = sequence_cases()[name]
        nodes = get_pool("wide2").nodes
        _seq[name] = (case, from_scenario(nodes, [[] for _ in nodes], [c.pods for c in case.cands],
                                          stamped="domain-limits-seq-" + name))
    return _seq[name]
