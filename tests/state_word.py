"""K2's 64-bit state word at its high bits and at its 64 / 65-bit limit: the
inputs, the layout rule restated in Python and the hand-derived plans
(test_state_word_reference.py proves them on the oracle and the layout on the
encoder's host view, test_gpu_state_word.py runs them through the C ABI).

The word (encode.cpp "host ports ... as state
bits"; antiaff.cpp) holds what the pods of one candidate do to each other on a
node:

    [0, 2A)            hostname anti-affinity pairs (A, B), numbered per candidate; A is the call's maximum
    [2A, 2A + 2P)      pairs (W, S) of port groups with a specific host IP and of inline disks, call-wide
    [2A + 2P, ...)     single bits: a wildcard-only port group, and I(ip) per specific IP, call-wide

Pairs and singles are numbered in candidate order, pod by pod, port by port.
A pod conflicts with a node whose word holds the pair-swapped image of what
the pod sets (A <-> B, W <-> S, singles fixed); swap_mask covers [0, 2A + 2P).
A candidate whose groups would take the word past 64 bits has them undone and
is SR_CAND_FALLBACK; more than 32 anti-affinity pairs in one candidate
likewise.  `layout` below is that rule and nothing else.

Pools.  Nodes s0, s1, .. in NodeInfoArray order, 64 cpus, room for 300 pods,
the hostname label (and zone z<n // 2> where a case says so); every candidate
pod asks for 10m.  Every pod fits every node by every predicate but the one
under test, so first fit puts a pod on node 0 unless a state bit -- or a base
pod's port, addressed through the same bit -- refuses it.

The deciding shape: pods a, b of one candidate; a takes node 0, b must go to
node 1 because of the bit.  A candidate's `bits` names the positions the
deciding pods set, its twin (`twin_pods`) is the same candidate with the
deciding port, disk or term removed from b, which then shares node 0.

Pads are earlier candidates of the call that use up positions (they are
planned and compared like every other candidate; each is one pod on node 0,
the anti-affinity pad two pods on nodes 0 and 1):

    pad_single(n)   n distinct wildcard host ports         n singles
    pad_ip(p)       p (port, specific IP) groups           p pairs and p singles
    pad_disk(p)     p inline read-only ISCSI disks         p pairs, no single (host.hpp for_each_port)
    pad_anti(k)     x with k hostname terms selecting y    A = k
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from helpers import Scenario
from spotplanner.model import (Container, ContainerPort, LabelSelector, Node, Pod, PodAffinityTerm, Volume)

H, Z = "kubernetes.io/hostname", "zone"
OK, FB = -1, -2  # SR_CAND_OK, SR_CAND_FALLBACK
FULL = (1 << 64) - 1


@dataclass
class Cand:
    name: str
    pods: List[Pod]
    want: List[int]                      # node of every pod (ignored for a fallback candidate)
    status: int = OK                     # SR_CAND_OK, SR_CAND_FALLBACK
    bits: Dict[int, List[int]] = field(default_factory=dict)  # pod -> the positions it sets (deciding pods)
    twin_pods: Optional[List[Pod]] = None
    twin_want: Optional[List[int]] = None


@dataclass
class Case:
    name: str
    rule: str
    cands: List[Cand]
    swap_mask: int
    n_nodes: int = 6
    node_pods: int = 300
    base: Dict[int, List[Pod]] = field(default_factory=dict)       # node -> its base pods
    twin_base: Optional[Dict[int, List[Pod]]] = None                # the twin's base pods (default: `base`)
    closed: Tuple[int, ...] = ()      # nodes a base pod fills (no cpu left)
    zones: bool = False
    memory: int = 1 << 36
    ext: bool = False                 # has an init-container candidate (a launch with one has no cooperative blocks)
    extra: List[Pod] = field(default_factory=list)  # further unbound pods of the cluster (fillers of a tick)


# ------------------------------------------------------------------ the layout rule
def pod_ports(p: Pod):
    """(group, ip) in the encoder's order: host ports (port > 0) of the containers, then inline disks.
    ip: None wildcard / read-write mount, "ro" a read-only mount (EBS is always read-write), else the host IP."""
    out = []
    for hp in p.host_ports():
        out.append((("port", hp.protocol or "TCP", hp.host_port), None if hp.host_ip in ("", "0.0.0.0") else hp.host_ip))
    for v in p.volumes:
        for kind, vid in (("gce", v.gce_pd), ("ebs", v.aws_ebs), ("iscsi", v.iscsi_iqn)):
            if vid is not None:
                out.append((("disk", kind, vid), "ro" if v.read_only and kind != "ebs" else None))
    return out


def _selects(t: PodAffinityTerm, owner: Pod, p: Pod) -> bool:
    ns = t.namespaces or [owner.namespace]
    sel = t.label_selector
    return sel is not None and p.namespace in ns and all(p.labels.get(k) == v for k, v in sel.match_labels.items())


def _term_key(t: PodAffinityTerm, owner: Pod):
    return (t.topology_key, tuple(sorted(t.namespaces or [owner.namespace])),
            tuple(sorted(t.label_selector.match_labels.items())))


def anti_pairs(pods: List[Pod]):
    """The candidate's interacting hostname terms in order of first appearance, and per pod the pair bits
    (relative to bit 0): A = 2p for a pod that has the term, B = 2p + 1 for a pod it selects.  A term interacts
    when one pod of the candidate has it and one matches it, unless that is one and the same single pod."""
    terms = []
    for p in pods:
        for t in p.pod_anti_affinity or []:
            if t.topology_key == H and _term_key(t, p) not in [k for k, _, _ in terms]:
                terms.append((_term_key(t, p), t, p))
    need, masks = [], [0] * len(pods)
    for key, t, owner in terms:
        has = [i for i, p in enumerate(pods) if any(_term_key(u, p) == key for u in p.pod_anti_affinity or [])]
        sel = [i for i, p in enumerate(pods) if _selects(t, owner, p)]
        if has and sel and not (len(has) == 1 and has == sel):
            for i in has:
                masks[i] |= 1 << (2 * len(need))
            for i in sel:
                masks[i] |= 2 << (2 * len(need))
            need.append(key)
    return len(need), masks


def layout(cands: List[List[Pod]]):
    """(per candidate per pod the mask it sets, swap_mask, the candidates that fall back)."""
    fallback = set()
    anti = []
    for c, pods in enumerate(cands):
        n, masks = anti_pairs(pods)
        if n > 32:
            fallback.add(c)
            n, masks = 0, [0] * len(pods)
        anti.append((n, masks))
    A = max([n for n, _ in anti] + [0])
    live = [c for c in range(len(cands)) if c not in fallback]
    specific = {}
    for c in live:
        for p in cands[c]:
            for g, ip in pod_ports(p):
                specific[g] = specific.get(g, False) or ip is not None
    pair, single, ipbit = {}, {}, {}
    n_pairs = n_single = 0
    for c in live:
        if not any(pod_ports(p) for p in cands[c]):
            continue
        saved = (dict(pair), dict(single), dict(ipbit), n_pairs, n_single)
        for p in cands[c]:
            for g, ip in pod_ports(p):
                if g not in pair and g not in single:
                    if specific[g]:
                        pair[g] = n_pairs
                        n_pairs += 1
                    else:
                        single[g] = n_single
                        n_single += 1
                if ip not in (None, "ro") and (g, ip) not in ipbit:
                    ipbit[(g, ip)] = n_single
                    n_single += 1
        if 2 * A + 2 * n_pairs + n_single > 64:
            pair, single, ipbit, n_pairs, n_single = saved
            fallback.add(c)
    base = 2 * A + 2 * n_pairs
    masks = []
    for c, pods in enumerate(cands):
        out = []
        for i, p in enumerate(pods):
            m = 0 if c in fallback else anti[c][1][i]
            for g, ip in pod_ports(p) if c not in fallback else []:
                if g in single:
                    m |= 1 << (base + single[g])
                elif ip is None:
                    m |= 3 << (2 * A + 2 * pair[g])
                elif ip == "ro":
                    m |= 2 << (2 * A + 2 * pair[g])
                else:
                    m |= (2 << (2 * A + 2 * pair[g])) | (1 << (base + ipbit[(g, ip)]))
            out.append(m)
        masks.append(out)
    return masks, (FULL if base >= 64 else (1 << base) - 1), fallback


# ------------------------------------------------------------------ pods
_CPU = 10


def wp(name, *ports, **kw) -> Pod:
    """A pod with wildcard TCP host ports."""
    return Pod(name, containers=[Container(cpu_milli=_CPU, ports=[ContainerPort(p) for p in ports])], **kw)


def ipp(name, port, ip="", proto="TCP") -> Pod:
    return Pod(name, containers=[Container(cpu_milli=_CPU, ports=[ContainerPort(port, protocol=proto, host_ip=ip)])])


def dsk(name, *disks) -> Pod:
    """disks: (iqn, read_only)."""
    return Pod(name, containers=[Container(cpu_milli=_CPU)],
               volumes=[Volume(name="v%d" % k, iscsi_iqn=d, read_only=ro) for k, (d, ro) in enumerate(disks)])


def plain(name, **kw) -> Pod:
    return Pod(name, containers=[Container(cpu_milli=_CPU)], **kw)


def term(key, **labels) -> PodAffinityTerm:
    return PodAffinityTerm(key, LabelSelector(match_labels=dict(labels)))


def pad_single(tag, n, first=20000) -> Cand:
    return Cand("pad_single_" + tag, [wp("ps-%s" % tag, *range(first, first + n))], [0])


def pad_ip(tag, p, first=30000) -> Cand:
    pod = Pod("pi-%s" % tag, containers=[Container(cpu_milli=_CPU, ports=[
        ContainerPort(first + k, host_ip="10.9.0.%d" % (k + 1)) for k in range(p)])])
    return Cand("pad_ip_" + tag, [pod], [0])


def pad_disk(tag, p, first=0) -> Cand:
    return Cand("pad_disk_" + tag, [dsk("pd-%s" % tag, *[("iqn.pad:%d" % (first + k), True) for k in range(p)])], [0])


def pad_anti(tag, k) -> Cand:
    """x has k hostname terms, each selecting y through a label of its own: y is refused where x is."""
    x = plain("pax-%s" % tag, pod_anti_affinity=[term(H, **{"pa%d-%s" % (i, tag): "y"}) for i in range(k)])
    y = plain("pay-%s" % tag, labels={"pa%d-%s" % (i, tag): "y" for i in range(k)})
    return Cand("pad_anti_" + tag, [x, y], [0, 1],
                bits={0: [2 * i for i in range(k)], 1: [2 * i + 1 for i in range(k)]},
                twin_pods=[x, plain("pay-%s" % tag)], twin_want=[0, 0])


# ------------------------------------------------------------------ the cases
SINGLE_POS = (0, 31, 32, 33, 62, 63)


def _singles_call(form: str) -> Case:
    """One call, 64 single bits: probes at 0, 31, 32, 33, 62, 63 (port 9000 + position), pads between them."""
    cands, at = [], 0
    for s in SINGLE_POS:
        if s > at:
            cands.append(pad_single("%s%d" % (form, s), s - at, first=20000 + at))
        port, t = 9000 + s, "%s%d" % (form, s)
        if form == "excl":    # every pod of the candidate sets the one bit: the exclusive form
            c = Cand("excl_%d" % s, [wp("a-" + t, port), wp("b-" + t, port)], [0, 1], bits={0: [s], 1: [s]},
                     twin_pods=[wp("a-" + t, port), plain("b-" + t)], twin_want=[0, 0])
        else:                 # a port-less pod between them: not exclusive
            c = Cand("mid_%d" % s, [wp("a-" + t, port), plain("m-" + t), wp("b-" + t, port)], [0, 0, 1],
                     bits={0: [s], 2: [s]}, twin_pods=[wp("a-" + t, port), plain("m-" + t), plain("b-" + t)],
                     twin_want=[0, 0, 0])
        cands.append(c)
        at = s + 1
    rule = {"excl": "two pods on one wildcard port: every pod sets the bit (the exclusive form)",
            "mid": "a port-less pod between the two: not exclusive"}
    return Case("singles_" + form, rule[form], cands, swap_mask=0)


IP1, IP2 = "10.0.0.1", "10.0.0.2"


def _ip_cases() -> List[Case]:
    """I(ip) at 32 and 63, the group's pair (W, S) at bits (0, 1): one pair, so singles start at bit 2 (two
    pairs, bit 4, where a second protocol brings a group of its own)."""
    out = []
    for hi in (32, 63):
        def call(name, rule, probe, pairs=1, n_ip=1):
            first_ip = hi - n_ip + 1 if hi == 63 else hi      # the probe's first I bit
            pad = pad_single("%s%d" % (name, hi), first_ip - 2 * pairs)
            probe.bits = {k: [b if b < 2 * pairs else first_ip + b - 2 * pairs for b in v]
                          for k, v in probe.bits.items()}
            return Case("ip_%s_%d" % (name, hi), rule, [pad, probe], swap_mask=(1 << (2 * pairs)) - 1)

        t = str(hi)
        # relative bits: 0 = W, 1 = S, 2.. = the probe's I bits in order (call() moves them up)
        out.append(call("same", "the same IP twice: S, I(ip) against I(ip)",
                        Cand("same", [ipp("a-same" + t, 7000, IP1), ipp("b-same" + t, 7000, IP1)], [0, 1],
                             bits={0: [1, 2], 1: [1, 2]},
                             twin_pods=[ipp("a-same" + t, 7000, IP1), plain("b-same" + t)], twin_want=[0, 0])))
        out.append(call("two", "two IPs of one group share a node: I(ip1), I(ip2) are two bits",
                        Cand("two", [ipp("a-two" + t, 7000, IP1), ipp("b-two" + t, 7000, IP2)], [0, 0],
                             bits={0: [1, 2], 1: [1, 3]}), n_ip=2))
        out.append(call("wild_after", "0.0.0.0 after an IP: W, S against S",
                        Cand("wild_after", [ipp("a-wa" + t, 7000, IP1), ipp("b-wa" + t, 7000, "0.0.0.0")], [0, 1],
                             bits={0: [1, 2], 1: [0, 1]},
                             twin_pods=[ipp("a-wa" + t, 7000, IP1), plain("b-wa" + t)], twin_want=[0, 0])))
        out.append(call("ip_after", "an IP after 0.0.0.0: S, I(ip) against W",
                        Cand("ip_after", [ipp("a-ia" + t, 7000), ipp("b-ia" + t, 7000, IP1)], [0, 1],
                             bits={0: [0, 1], 1: [1, 2]},
                             twin_pods=[ipp("a-ia" + t, 7000), plain("b-ia" + t)], twin_want=[0, 0])))
        # TCP is pair 0 (bits 0, 1), UDP pair 1 (bits 2, 3); relative 4 = I(tcp ip), 5 = I(udp ip)
        out.append(call("proto", "another protocol on the same port and IP is another group: they share a node",
                        Cand("proto", [ipp("a-pr" + t, 7000, IP1), ipp("b-pr" + t, 7000, IP1, "UDP")], [0, 0],
                             bits={0: [1, 4], 1: [3, 5]}), pairs=2, n_ip=2))
    return out


def _pair_cases() -> List[Case]:
    out = []
    # pairs 15 and 16 after fifteen disk pairs: bits (30, 31) and (32, 33); their I bits are singles 0 and 1
    # (bits 34, 35); `ip_pad`: behind fifteen (port, IP) groups instead, whose I bits are singles 0..14, so the
    # probes' are singles 15 and 16 (bits 49, 50)
    for order in ("wild_first", "ip_first", "ip_pad"):
        cands = [pad_ip(order, 15) if order == "ip_pad" else pad_disk(order, 15)]
        for k, port in enumerate((7100, 7200)):
            W, S, I = 30 + 2 * k, 31 + 2 * k, (49 if order == "ip_pad" else 34) + k
            t = "%s%d" % (order, port)
            if order != "ip_first":
                pods, bits = [ipp("a-" + t, port), ipp("b-" + t, port, IP1)], {0: [W, S], 1: [S, I]}
            else:
                pods, bits = [ipp("a-" + t, port, IP1), ipp("b-" + t, port)], {0: [S, I], 1: [W, S]}
            cands.append(Cand("pair_%d" % (30 + 2 * k), pods, [0, 1], bits=bits,
                              twin_pods=[pods[0], plain("b-" + t)], twin_want=[0, 0]))
        out.append(Case("pairs_30_32_" + order, "a port group with a specific IP whose pair is (30, 31) / (32, 33): "
                        "%s, the other pod meets W / S" % {"ip_pad": "wild first, behind a pad with I bits"}.get(
                            order, order.replace("_", " ")), cands, swap_mask=(1 << 34) - 1))
    # 32 disk pairs: single_base == 64, swap_mask == ~0; the probe's disk is pair 31, bits (62, 63)
    D = "iqn.probe:31"
    for name, rule, a_ro, b_ro, want in (
            ("rw_after_ro", "read-write after read-only: W, S against S", True, False, [0, 1]),
            ("ro_after_rw", "read-only after read-write: S against W", False, True, [0, 1]),
            ("ro_ro", "two read-only mounts share a node: S never meets S", True, True, [0, 0])):
        probe = Cand(name, [dsk("a-" + name, (D, a_ro)), dsk("b-" + name, (D, b_ro))], want,
                     bits={0: [63] if a_ro else [62, 63], 1: [63] if b_ro else [62, 63]})
        if want == [0, 1]:
            probe.twin_pods, probe.twin_want = [probe.pods[0], plain("b-" + name)], [0, 0]
        out.append(Case("disk_62_" + name, rule, [pad_disk(name, 31), probe], swap_mask=FULL))
    return out


def _anti32(tag, n_pairs, last) -> Cand:
    """2 * n_pairs pods in label pairs: pods 2i, 2i + 1 carry g<i> and a hostname term selecting g<i> (each pair
    self-anti-affine: A and B on both), so even pods take node 0 and odd pods node 1.  The last pair is
    one-sided: `has_second` x is selected and comes first, y has the term and comes second; `selected_second`
    the other way round."""
    pods, want, n = [], [], n_pairs - 1
    for i in range(n):
        for j in (0, 1):
            pods.append(plain("%s-%d-%d" % (tag, i, j), labels={"g%d" % i: tag},
                              pod_anti_affinity=[term(H, **{"g%d" % i: tag})]))
        want += [0, 1]
    has = plain("%s-has" % tag, pod_anti_affinity=[term(H, **{"g%d" % n: tag})])
    sel = plain("%s-sel" % tag, labels={"g%d" % n: tag})
    A, B = 2 * n, 2 * n + 1
    if last == "has_second":
        pods += [sel, has]
        bits = {2 * n: [B], 2 * n + 1: [A]}
        twin = pods[:-1] + [plain("%s-has" % tag)]
    else:
        pods += [has, sel]
        bits = {2 * n: [A], 2 * n + 1: [B]}
        twin = pods[:-1] + [plain("%s-sel" % tag)]
    return Cand("anti%d_%s" % (n_pairs, last), pods, want + [0, 1], bits=bits, twin_pods=twin, twin_want=want + [0, 0])


def _anti_cases() -> List[Case]:
    out = []
    for last in ("has_second", "selected_second"):
        out.append(Case("anti32_" + last, "an anti-affinity-only word: 32 pairs, pair 31 at bits 62 / 63 decides pods "
                        "62 and 63 (%s)" % last.replace("_", " "), [_anti32("aa" + last[0], 32, last)], swap_mask=FULL))
    c33 = _anti32("ab", 33, "has_second")
    c33.status, c33.twin_pods, c33.twin_want, c33.bits = FB, None, None, {}
    out.append(Case("anti33", "33 hostname terms in one candidate: it alone falls back (need.size() > 32); the "
                    "candidate behind it is planned with A = 1",
                    [c33, pad_anti("a33", 1)], swap_mask=3))
    port = Cand("port_after_anti32", [wp("a-p32", 9100), wp("b-p32", 9100)], [], status=FB)
    out.append(Case("anti32_and_port", "32 pairs fill the word: a port candidate in the same call falls back, the "
                    "anti-affinity one does not", [_anti32("ac", 32, "has_second"), port], swap_mask=FULL))
    return out


def _mixed() -> Case:
    """A = 3 (bits 0..5), one port pair (6, 7), singles 8..63: I(ip) at 8, 54 pad singles, the probe's at 63."""
    a, b = ipp("a-mix", 7000), ipp("b-mix", 7000, IP1)
    c = plain("c-mix", pod_anti_affinity=[term(H, mix="a")])
    a.labels = {"mix": "a"}
    return Case("mixed", "A = 3, a port pair, singles up to bit 63; one probe decided in each region; a candidate "
                "with one anti-affinity pair keeps its port bits above 2A = 6",
                [pad_anti("mix", 3),
                 Cand("mix_pair", [a, b, c], [0, 1, 1], bits={0: [1, 6, 7], 1: [7, 8], 2: [0]},
                      twin_pods=[a, plain("b-mix"), c], twin_want=[0, 0, 1]),
                 pad_single("mix", 54),
                 Cand("mix_single", [wp("a-mixs", 9063), wp("b-mixs", 9063)], [0, 1], bits={0: [63], 1: [63]},
                      twin_pods=[wp("a-mixs", 9063), plain("b-mixs")], twin_want=[0, 0])],
                swap_mask=0xff)


def _probe2(tag, p1, p2, extra=()) -> Cand:
    """a lists p1, p2 (and `extra`), b lists p2: two new singles, b decided by the second."""
    return Cand("probe_" + tag, [wp("a-" + tag, p1, p2, *extra), wp("b-" + tag, p2)], [0, 1],
                twin_pods=[wp("a-" + tag, p1, p2, *extra), plain("b-" + tag)], twin_want=[0, 0])


def _limit_cases() -> List[Case]:
    out = []
    p = _probe2("l64", 9001, 9002)
    p.bits = {0: [62, 63], 1: [63]}
    out.append(Case("limit_64", "a call that sums to exactly 64 bits is planned on the device",
                    [pad_single("l64", 62), p], swap_mask=0))
    p = _probe2("l65", 9001, 9002, extra=(9003,))
    p.status, p.want, p.twin_pods, p.twin_want = FB, [], None, None
    out.append(Case("limit_65", "one more port on the last candidate: it alone falls back",
                    [pad_single("l65", 62), p], swap_mask=0))
    over = Cand("over", [wp("a-lro", 9001, 9002, 9003), wp("b-lro", 9003)], [], status=FB)
    p = _probe2("lre", 9001, 9002)
    p.bits = {0: [62, 63], 1: [63]}
    out.append(Case("limit_reuse", "a later candidate reuses groups the overflowing one introduced and had undone: "
                    "numbered afresh at 62, 63", [pad_single("lre", 62), over, p], swap_mask=0))
    over = Cand("over_mid", [wp("a-lmo", *range(9010, 9015)), wp("b-lmo", 9010)], [], status=FB)
    p1, p2 = _probe2("lm1", 9001, 9002), _probe2("lm2", 9003, 9004)
    p1.bits, p2.bits = {0: [60, 61], 1: [61]}, {0: [62, 63], 1: [63]}
    out.append(Case("limit_middle", "a candidate in the middle overflows (60 + 5), the ones behind it still fit",
                    [pad_single("lmi", 60), over, p1, p2], swap_mask=0))
    return out


def _base_cases() -> List[Case]:
    """Base conflicts are static atoms addressed by the bit that stands for the query (bit_query)."""
    out = []
    out.append(Case("base_single_63", "node 0's base pod holds the port whose bit is 63: both probe pods skip it",
                    [pad_single("b63", 63), Cand("probe_b63", [wp("a-b63", 9063), wp("b-b63", 9063)], [1, 2],
                                                 bits={0: [63], 1: [63]})],
                    swap_mask=0, base={0: [wp("base-b63", 9063)]}, twin_base={0: [plain("base-b63")]}))
    out[-1].cands[1].twin_pods, out[-1].cands[1].twin_want = out[-1].cands[1].pods, [0, 1]
    # The probe's disk is pair 31, bits (62, 63).  (A disk that every pod of the call mounts read-write is a
    # single bit, like a wildcard-only port: the read-only third pod of `w` is what makes it a pair.)
    D = "iqn.base:31"
    probe = Cand("probe_bdw", [dsk("a-bdw", (D, False)), dsk("b-bdw", (D, False)), dsk("c-bdw", (D, True))], [1, 2, 0],
                 bits={0: [62, 63], 1: [62, 63], 2: [63]})
    probe.twin_pods, probe.twin_want = probe.pods, [0, 1, 2]
    out.append(Case("base_disk_w", "read-write mounts (W, bit 62) of a disk node 0 holds read-only skip node 0 and "
                    "each other; the read-only mount shares node 0",
                    [pad_disk("bdw", 31), probe], swap_mask=FULL, base={0: [dsk("base-bdw", (D, True))]},
                    twin_base={0: [plain("base-bdw")]}))
    probe = Cand("probe_bds", [dsk("a-bds", (D, True)), dsk("b-bds", (D, True))], [1, 1], bits={0: [63], 1: [63]})
    probe.twin_pods, probe.twin_want = probe.pods, [0, 0]
    out.append(Case("base_disk_s", "read-only mounts (S, bit 63) of a disk node 0 holds read-write skip node 0 and "
                    "share node 1", [pad_disk("bds", 31), probe], swap_mask=FULL,
                    base={0: [dsk("base-bds", (D, False))]}, twin_base={0: [plain("base-bds")]}))
    return out


def _two_positions(tag, make, **kw) -> Case:
    """A call with the candidate `make(tag, port)` builds at bit 33 and again at bit 63."""
    c33, c63 = make(tag + "33", 9033, 33), make(tag + "63", 9063, 63)
    return Case("form_" + tag, kw.pop("rule"), [pad_single(tag + "a", 33), c33, pad_single(tag + "b", 29, first=21000),
                                                c63], swap_mask=0, **kw)


def _form_cases() -> List[Case]:
    out = []

    def big(n_fill):
        def make(t, port, bit):
            fill = [plain("f-%s-%d" % (t, i)) for i in range(n_fill)]
            return Cand("big_" + t, fill + [wp("a-" + t, port), wp("b-" + t, port)], [0] * n_fill + [0, 1],
                        bits={n_fill: [bit], n_fill + 1: [bit]},
                        twin_pods=fill + [wp("a-" + t, port), plain("b-" + t)], twin_want=[0] * (n_fill + 2))
        return make

    out.append(_two_positions("g1", big(64), rule="a 66-pod candidate decided at pods 64 / 65 (pod group 1)"))
    out.append(_two_positions("g2", big(128), rule="a 130-pod candidate decided at pods 128 / 129 (pod group 2)"))

    def excl(n):
        # every pod lists the port: the exclusive step places a pod group per window visit against the nodes
        # taken so far and hands the placed pods' bits to their nodes afterwards, so pod group 1 (2) meets the
        # bits of the groups before it on nodes 0..63 (0..127) and moves on to node 64 (128)
        def make(t, port, bit):
            pods = [wp("e%d-%s" % (i, t), port) for i in range(n)]
            return Cand("excl%d_%s" % (n, t), pods, list(range(n)), bits={0: [bit], 63: [bit], n - 2: [bit], n - 1: [bit]},
                        twin_pods=pods[:-1] + [plain("e%d-%s" % (n - 1, t))], twin_want=list(range(n - 1)) + [0])
        return make

    out.append(_two_positions("excl66", excl(66), rule="66 pods on one port, one node each: pods 64 / 65 pass the "
                              "64 nodes the first pod group took", n_nodes=70))
    out.append(_two_positions("excl130", excl(130), rule="130 pods on one port: pods 128 / 129 pass 128 taken nodes",
                              n_nodes=134))

    def p260(t, port, bit):
        # a -> 0, b -> 1 (the port); 256 port-less pods fill nodes 0..5 to 40 pods and put 18 on node 6;
        # c meets a on 0, b on 1 (and both are full): node 6; d meets c there: node 7
        fill = [plain("f-%s-%d" % (t, i)) for i in range(256)]
        want = [0, 1] + [0] * 39 + [1] * 39 + [2] * 40 + [3] * 40 + [4] * 40 + [5] * 40 + [6] * 18 + [6, 7]
        pods = [wp("a-" + t, port), wp("b-" + t, port)] + fill + [wp("c-" + t, port), wp("d-" + t, port)]
        # the twin: b and d without the port; b joins a, every filler moves one place up, c and d share node 6
        twin = [pods[0], plain("b-" + t)] + fill + [pods[-2], plain("d-" + t)]
        twant = [0, 0] + [0] * 38 + [1] * 40 + [2] * 40 + [3] * 40 + [4] * 40 + [5] * 40 + [6] * 18 + [6, 6]
        return Cand("p260_" + t, pods, want, bits={0: [bit], 1: [bit], 258: [bit], 259: [bit]}, twin_pods=twin,
                    twin_want=twant)

    # (a pad is one pod on node 0: each of the four candidates starts from the base state)
    out.append(_two_positions("p260", p260, rule="a 260-pod candidate (pod order), decided at pods 0 / 1 and 258 / "
                              "259; 8 nodes with room for 40 pods, so touched nodes are rechecked",
                              n_nodes=8, node_pods=40))

    def ext(t, port, bit):
        init = Pod("i-" + t, containers=[Container(cpu_milli=_CPU)], init_containers=[Container(cpu_milli=500)])
        return Cand("ext_" + t, [init, wp("a-" + t, port), wp("b-" + t, port)], [0, 0, 1], bits={1: [bit], 2: [bit]},
                    twin_pods=[init, wp("a-" + t, port), plain("b-" + t)], twin_want=[0, 0, 0])

    out.append(_two_positions("ext", ext, rule="an init-container pod first: the extension-record kernels", ext=True))

    def dom(t, port, bit):
        # z1, z2 refuse each other's zone (nodes 0, 1 are zone z0): the candidate takes the domain path
        zs = [plain("z%d-%s" % (i, t), labels={"zz": t}, pod_anti_affinity=[term(Z, zz=t)]) for i in (1, 2)]
        return Cand("dom_" + t, [wp("a-" + t, port), wp("b-" + t, port)] + zs, [0, 1, 0, 2], bits={0: [bit], 1: [bit]},
                    twin_pods=[wp("a-" + t, port), plain("b-" + t)] + zs, twin_want=[0, 0, 0, 2])

    out.append(_two_positions("dom", dom, rule="zone anti-affinity among its pods (the domain path) and the port "
                              "conflict", zones=True))

    def wide(t, port, bit):
        # 2^40 + 1 bytes on nodes of 2^52: the call's memory unit is one byte and the request has no 32-bit form
        def mk(n, *ports):
            return Pod(n, containers=[Container(cpu_milli=_CPU, memory=(1 << 40) + 1,
                                                ports=[ContainerPort(p) for p in ports])])
        return Cand("wide_" + t, [mk("a-" + t, port), mk("b-" + t, port)], [0, 1], bits={0: [bit], 1: [bit]},
                    twin_pods=[mk("a-" + t, port), mk("b-" + t)], twin_want=[0, 0])

    out.append(_two_positions("wide64", wide, rule="a request the scaled 32-bit form cannot hold: 64-bit values",
                              memory=1 << 52))

    def far(t, port, bit):
        return Cand("far_" + t, [wp("a-" + t, port), wp("b-" + t, port)], [127, 128], bits={0: [bit], 1: [bit]},
                    twin_pods=[wp("a-" + t, port), plain("b-" + t)], twin_want=[127, 127])

    case = _two_positions("pool130", far, rule="130 nodes, only 127 and 128 open: the conflict is met in window 1, "
                          "the pod lands in window 2", n_nodes=130, closed=tuple(set(range(130)) - {127, 128}))
    for c in case.cands:
        if c.name.startswith("pad_"):
            c.want = [127]
    out.append(case)
    return out


def _build_cases() -> List[Case]:
    cases = [_singles_call("excl"), _singles_call("mid"), _low_call()]
    cases += _ip_cases() + _pair_cases() + _anti_cases() + [_mixed()] + _limit_cases() + _base_cases() + _form_cases()
    return cases


def _low_call() -> Case:
    """The `low` form: its position-0 probe lists port 20000 first, so 20000 is bit 0 and the probe's own port bit
    1; the pad behind it starts at 20001 and ends one position earlier."""
    cands, at = [], 0
    for s in SINGLE_POS:
        t = "low%d" % s
        if s == 0:
            c = Cand("low_0", [wp("a-" + t, 20000, 9000), wp("b-" + t, 9000), wp("c-" + t, 20000)], [0, 1, 1],
                     bits={0: [0, 1], 1: [1], 2: [0]},
                     twin_pods=[wp("a-" + t, 20000, 9000), plain("b-" + t), wp("c-" + t, 20000)], twin_want=[0, 0, 1])
            cands.append(c)
            at = 2
            continue
        if s > at:
            cands.append(pad_single(t, s - at, first=20000 + at))
        port = 9000 + s
        cands.append(Cand("low_%d" % s, [wp("a-" + t, 20000, port), wp("b-" + t, port), wp("c-" + t, 20000)],
                          [0, 1, 1], bits={0: [0, s], 1: [s], 2: [0]},
                          twin_pods=[wp("a-" + t, 20000, port), plain("b-" + t), wp("c-" + t, 20000)],
                          twin_want=[0, 0, 1]))
        at = s + 1
    return Case("singles_low", "a lists a second, low port (bit 0) that a third pod shares: b moves for the high bit "
                "alone, c for the low one", cands, swap_mask=0)


def _tick_case() -> Case:
    """The call of the tick script (TICKS): thirty disk pairs and one single in front of a probe whose group has
    a specific IP: pair 30 at (60, 61), the pad's single at 62, I(ip) at 63."""
    a, b = ipp("a-tick", 7000), ipp("b-tick", 7000, IP1)
    probe = Cand("probe_tick", [a, b], [0, 1], bits={0: [60, 61], 1: [61, 63]}, twin_pods=[a, plain("b-tick")],
                 twin_want=[0, 0])
    return Case("ticks", "pads, then 0.0.0.0 and an IP on one port: pair (60, 61), I(ip) at 63",
                [pad_disk("tick", 30), pad_single("tick", 1), probe], swap_mask=(1 << 62) - 1,
                extra=[wp("filler-tick", 7000)], n_nodes=16)  # (16 nodes: one changed node is no pool rebuild)


CASES: Dict[str, Case] = {}
for _c in _build_cases() + [_tick_case()]:
    assert _c.name not in CASES, _c.name
    CASES[_c.name] = _c
# cases with an init-container candidate: a launch with extension records has no cooperative blocks
EXT_CASES = tuple(n for n, c in CASES.items() if c.ext)


# ------------------------------------------------------------------ the encoded input
class Input:
    """One case's cluster, built once per process: nodes, base pods, every candidate's pods and the extra pods as
    unbound pods, with pod stamps.  A call is the case's candidate list, or that list without some candidates
    (`drop`: the same cluster, a shorter list)."""

    def __init__(self, case: Case, twin: bool = False):
        self.case = case
        self.all_cands = list(case.cands)
        self.all_pods = [(c.twin_pods if twin and c.twin_pods is not None else c.pods) for c in self.all_cands]
        base = case.twin_base if twin and case.twin_base is not None else case.base
        nodes, spot_pods = [], []
        for n in range(case.n_nodes):
            labels = {H: "s%d" % n}
            if case.zones:
                labels[Z] = "z%d" % (n // 2)
            nodes.append(Node("s%d" % n, cpu_milli=64000, memory=case.memory, pods=case.node_pods, labels=labels))
            ps = list(base.get(n, []))
            if n in case.closed:
                ps.append(Pod("full%d" % n, containers=[Container(cpu_milli=64000)]))
            spot_pods.append(ps)
        flat = [p for ps in self.all_pods for p in ps]
        n_pods = sum(len(ps) for ps in spot_pods) + len(flat) + len(case.extra)
        tag = zlib.crc32(("state-word-%s-%d" % (case.name, twin)).encode())
        stamps = [(1 << 63) | (tag << 24) | (i + 1) for i in range(n_pods)]
        self.sc = Scenario(nodes, spot_pods, flat + list(case.extra), stamps=stamps)
        self.extra_pod = [self.sc.qidx(len(flat) + k) for k in range(len(case.extra))]
        self._oracle = {}
        self.cands, self.pods, self.cand_off, self.cand_pods = self.arrays()

    def arrays(self, drop: Tuple[str, ...] = ()):
        """(candidates, their pods, cand_off, cand_pods) of the call without the candidates named in `drop`."""
        first = np.cumsum([0] + [len(ps) for ps in self.all_pods])
        keep = [i for i, c in enumerate(self.all_cands) if c.name not in drop]
        cand_off = np.cumsum([0] + [len(self.all_pods[i]) for i in keep]).astype(np.int32)
        cand_pods = np.concatenate([np.arange(self.sc.qidx(first[i]), self.sc.qidx(first[i + 1])) for i in keep])
        return ([self.all_cands[i] for i in keep], [self.all_pods[i] for i in keep], cand_off,
                cand_pods.astype(np.int32))

    def oracle(self, drop: Tuple[str, ...] = (), fillers: Tuple[Tuple[int, int], ...] = ()):
        """The oracle's plan of the call (computed once, never changed); `fillers`: (pod, spot position) added to
        the snapshot first."""
        key = (drop, fillers)
        if key not in self._oracle:
            from oracle_lib import load_oracle, oracle_plan
            _, _, cand_off, cand_pods = self.arrays(drop)
            snap = self.sc.oracle_snapshot()
            for pod, pos in fillers:
                load_oracle().oracle_snapshot_add_pod(snap.h, self.sc.ptr, pod, pos)
            self._oracle[key] = oracle_plan(snap, self.sc.ptr, cand_off, cand_pods, mode=1)
        return self._oracle[key]


_inputs: Dict[tuple, Input] = {}


def get_input(name: str, twin: bool = False) -> Input:
    if (name, twin) not in _inputs:
        _inputs[(name, twin)] = Input(CASES[name], twin)
    return _inputs[(name, twin)]


def expected(cands: List[Cand], want: Optional[Dict[str, List[int]]] = None):
    """(status, node_of_pod, first_ok, first_fallback, winner, fallback_pods) of a call, from the hand-derived
    plans alone (`want`: other nodes for the named candidates); a fallback candidate's pods have no node (-1)."""
    want = want or {}
    status = np.array([c.status for c in cands], np.int32)
    nodes = np.concatenate([np.array(want.get(c.name, c.want) if c.status != FB else [-1] * len(c.pods), np.int32)
                            for c in cands])
    ok = [i for i, c in enumerate(cands) if c.status == OK]
    fb = [i for i, c in enumerate(cands) if c.status == FB]
    first_ok, first_fb = (ok[0] if ok else -1), (fb[0] if fb else -1)
    winner = first_ok if first_ok >= 0 and (first_fb < 0 or first_fb > first_ok) else -1
    return status, nodes, first_ok, first_fb, winner, sum(len(cands[i].pods) for i in fb)


# ------------------------------------------------------------------ across calls on one planner
# The script on the `ticks` case, one planner: (candidates dropped from the call, the filler pod on node 1?, the
# probe's nodes, the probe's bits, swap_mask).  Tick 2 is the probe alone: its pair is (0, 1), I(ip) bit 2 and
# swap_mask 3.  Tick 3 is tick 1's call after node 1 gained a base pod that holds the probe's port on 0.0.0.0:
# b skips node 0 (a's W) and node 1 (the base conflict, addressed by I(ip), bit 63).
TICK_PADS = ("pad_disk_tick", "pad_single_tick")
TICKS = [
    ((), False, [0, 1], {0: [60, 61], 1: [61, 63]}, (1 << 62) - 1),
    (TICK_PADS, False, [0, 1], {0: [0, 1], 1: [1, 2]}, 3),
    ((), True, [0, 2], {0: [60, 61], 1: [61, 63]}, (1 << 62) - 1),
]
TICK_FILLER_NODE = 1
TICK_SCRIPT = (0, 1, 0, 0, 0, 2, 2)  # indices into TICKS, in call order


def sequence_case():
    """sr_plan_sequence over a pad, a probe and a second probe on the same port (bit 63): the pad drains onto
    node 0, the first probe onto nodes 0 and 1, whose UsedPorts then hold the port: the second probe's pods take
    nodes 2 and 3.  Returns (nodes, base pods, candidates, node_of_pod, drained)."""
    nodes = [Node("s%d" % n, cpu_milli=64000, memory=1 << 36, pods=300, labels={H: "s%d" % n}) for n in range(6)]
    cands = [pad_single("seq", 63).pods, [wp("a-seq1", 9063), wp("b-seq1", 9063)],
             [wp("a-seq2", 9063), wp("b-seq2", 9063)]]
    return nodes, [[] for _ in nodes], cands, [0, 0, 1, 2, 3], [0, 1, 2]
