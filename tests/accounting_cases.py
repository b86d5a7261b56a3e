"""Accounting cases for sr_blockers_plan and sr_evacuate_plan: the group's own use of memory and ephemeral storage,
accounting apart from the fit request, 64-bit sums, the sorted list of k_blockers with memory and ephemeral values
in it, and the undo of k_evacuate from scenario to scenario.

The loop both calls follow is stated here in plain Python integers (`loop`): first fit over the nodes in position
order; per node free[d], the pod slack and the group's own used[d] / added; per pod req[3], acc[3] and "all-zero
request"; a lost set.  The statement keeps the group's own placements the way k_blockers does, as a list sorted by
node, which for a right loop is the dense table of k_evacuate.  It has named WRONG variants (`WRONG`), each what a
kernel with one slip would compute; a case group names the variants it is meant to catch, and
tests/test_accounting_cases_reference.py asserts on the CPU that the right answer is the oracle's and that the
answer under each named variant differs from it -- so an input is known to discriminate before a GPU sees it.

Pools have 65, 130 and 257 nodes (two, three and five row words, n_pad != n_spot).  Node values differ per
dimension in unit and magnitude -- cpu in millicores below 4,000, memory in GiB plus an odd byte count, ephemeral
storage in other odd sizes -- so a mixed-up dimension or stride changes a placement.  Every group without a lost
set is a candidate of sr_blockers_plan and a nothing-lost scenario of sr_evacuate_plan.

tests/test_gpu_blockers_accounting.py and tests/test_gpu_evacuate_accounting.py run the cases through the C ABI."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

from explain_cases import CPU, EPHEMERAL, MEMORY, PODS
from explain_plan_cases import BATCHED, SINGLE, pool
from known_answer import P, used
from spotplanner.model import Container, GiB, Pod

JUDGED, NOT_PLAIN = 1, 3
CAP = 256                      # SR_BLOCKERS_BATCH_PODS
BLOCK_THREADS = 256            # the default block of k_evacuate: 4 waves
BITS = (CPU, MEMORY, EPHEMERAL)
FIELD = ("cpu_milli", "memory", "ephemeral")
QUANTITY_END = 1 << 62

# ---------------------------------------------------------------------------------------------------------------
# the loop, and what a kernel with one slip would compute instead

WRONG = ("own_use_dim0_only", "account_req", "dims_swapped", "trunc32", "stale_deltas", "undo_first",
         "undo_dim0_only", "shift_dim0_only")


def _w32(x: int) -> int:
    """x as a signed 32-bit value."""
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


@dataclass
class MPod:
    req: Tuple[int, int, int]
    acc: Tuple[int, int, int]
    zero: bool                 # fitsRequest returns after the pod count


def mpod(p: Pod) -> MPod:
    req = tuple(int(v) for v in p.scheduler_request())
    acc = tuple(int(v) for v in p.node_accounting()[:3])
    return MPod(req, acc, not any(req) and not p.scalar_request())


def loop(free: Sequence[Sequence[int]], slack: Sequence[int], groups, wrong: Optional[str] = None, T: int = 0):
    """The groups (pods, lost) in the order one block takes them.  Returns per group (node_of_pod, rows): rows maps a
    pod that fits nowhere to {SR_WHY bit: nodes} over the nodes that are not lost.

    `ent` is the group's own placements [node, pods, acc0, acc1, acc2], sorted by node; a right loop clears it
    behind every group.  wrong:
      own_use_dim0_only  the group's own use of memory and ephemeral storage is ignored in the compares
      account_req        req is accounted in place of acc
      dims_swapped       the memory and ephemeral deltas are exchanged
      trunc32            sums and compares are taken in 32 bits
      stale_deltas       nothing is cleared between consecutive groups
      undo_first         only the nodes of a group's first T pods are cleared
      undo_dim0_only     the clearing leaves the memory and ephemeral sums
      shift_dim0_only    an insert below held entries moves their node, pod count and acc0 up by one and leaves
                         acc1 / acc2 where they were: the values stay behind while the nodes move"""
    assert wrong is None or wrong in WRONG
    n = len(free)
    ent: List[List[int]] = []
    by_node: Dict[int, List[int]] = {}     # node -> its entry of ent
    out = []
    for pods, lost in groups:
        gone = set(lost)
        mapping, rows = [], {}
        for k, p in enumerate(pods):
            at, row = -1, {}
            for j in range(n):
                if j in gone:
                    continue
                e = by_node.get(j)
                added, own = (e[1], e[2:5]) if e else (0, [0, 0, 0])
                if wrong == "own_use_dim0_only":
                    own = [own[0], 0, 0]
                mask = PODS if slack[j] - added < 1 else 0
                if not p.zero:
                    for d in range(3):
                        if wrong == "trunc32":
                            refuses = _w32(p.req[d]) > _w32(_w32(free[j][d]) - _w32(own[d]))
                        else:
                            refuses = p.req[d] > free[j][d] - own[d]
                        if refuses:
                            mask |= BITS[d]
                if mask == 0:
                    at = j
                    break
                for bit in (PODS,) + BITS:
                    if mask & bit:
                        row[bit] = row.get(bit, 0) + 1
            mapping.append(at)
            if at < 0:
                rows[k] = row
                continue
            a = list(p.req if wrong == "account_req" else p.acc)
            if wrong == "dims_swapped":
                a = [a[0], a[2], a[1]]
            e = by_node.get(at)
            if e is not None:
                e[1] += 1
                for d in range(3):
                    e[2 + d] += a[d]
            else:
                pos = sum(1 for x in ent if x[0] < at)
                old = [list(x) for x in ent]
                ent.insert(pos, [at, 1] + a)
                by_node[at] = ent[pos]
                if wrong == "shift_dim0_only":
                    for i in range(pos + 1, len(ent)):
                        ent[i][3:5] = old[i][3:5] if i < len(old) else [0, 0]
            if wrong == "trunc32":
                for x in ent:
                    x[2:5] = [_w32(v) for v in x[2:5]]
        out.append((mapping, rows))
        if wrong == "stale_deltas":
            continue
        for j in (mapping[:T] if wrong == "undo_first" else mapping):
            e = by_node.get(j)
            if e is not None:
                e[1] = e[2] = 0
                if wrong != "undo_dim0_only":
                    e[3] = e[4] = 0
        ent = [x for x in ent if any(x[1:])]
        by_node = {x[0]: x for x in ent}
    return out


# ---------------------------------------------------------------------------------------------------------------
# cases

@dataclass
class Group:
    name: str
    pods: List[Pod]
    lost: List[int] = field(default_factory=list)
    catches: Tuple[str, ...] = ()          # the wrong variants under which this group's answer must differ
    want: Optional[List[int]] = None       # node_of_pod written out by hand (-1: fits nowhere)
    rows: Dict[int, Dict[int, int]] = field(default_factory=dict)  # pod -> {SR_WHY bit: nodes}, by hand
    how_b: int = BATCHED                   # sr_blockers_plan's way (groups without a lost set)
    how_e: int = JUDGED                    # sr_evacuate_plan's word


@dataclass
class ACase:
    name: str
    nodes: list
    base: list
    groups: List[Group]
    all_rows: bool = True                  # GPU: check every row against sr_explain_candidate (False: the pinned ones)
    orders: Tuple[Tuple[int, ...], ...] = ()   # the undo case: scenario orders of one block, beside the list itself
    seq_catches: Tuple[str, ...] = ()      # ... and the variants every such order must expose


def alloc(j):
    """Allocatable of node j: another unit and another magnitude per dimension."""
    return dict(cpu=1000 + 7 * j, mem=(2 + j % 5) * GiB + 2 * j + 1, eph=5_000_000_001 + 1_000_003 * j, pods=110)


def build_pool(n, free, over=None):
    """n nodes with one base pod each that leaves free(j) = (cpu, memory, ephemeral); a negative value is a node
    overcommitted from the base.  over: {j: dict(cpu=, mem=, eph=, pods=)} where alloc(j) is not what the node
    has."""
    over = over or {}
    kw = {}
    for j in range(n):
        kw[j] = alloc(j)
        kw[j].update(over.get(j, {}))
    nodes = pool(n, over=kw)
    base = []
    for j in range(n):
        f = free(j)
        a = kw[j]
        base.append([used(cpu=a["cpu"] - f[0], mem=a["mem"] - f[1], eph=a["eph"] - f[2], name="u%d" % j)])
    return nodes, base


def one(name, d, x, floor=0):
    """A pod asking x in dimension d alone (and `floor` in the two others)."""
    v = [floor, floor, floor]
    v[d] = x
    return P(name, cpu=v[0], mem=v[1], eph=v[2])


def with_init(name, d, containers, init):
    """Containers asking `containers` and an init container asking `init` in dimension d."""
    return Pod(name, containers=[Container(**{FIELD[d]: containers})], init_containers=[Container(**{FIELD[d]: init})])


def edges(n):
    """The deciding nodes: the first, the last lane of a row word, the first lane of the next, the last node."""
    return sorted({0, 63, 64, n - 1})


def four(n):
    return edges(n) if n > 65 else [0, 1, 63, 64]


def closed3(j):
    """Free values below every request of the cases (3 or more), different per dimension."""
    return (j % 3, (j + 1) % 3, (j + 2) % 3)


OPEN_FREE = ((900, 37), (GiB + 12345, 2), (3_000_000_007, 11))  # (value at the first open node, step) per dimension


def open_free(i):
    return tuple(v + s * i for v, s in OPEN_FREE)


def _dimensions_apart(n):
    """The same first-fit ladder in memory only, in ephemeral storage only and in cpu only.  Open nodes 0, 63, 64
    and the last; every other node has less than 3 left in every dimension.  Per open node o_i with F_i free: three
    pods fill it to q_i below full; a pod of q_i + 1, one over, moves on to o_{i+1} (the last one's fits nowhere);
    a pod of q_i fills o_i exactly.  One more pod of 3 fits nowhere."""
    opens = edges(n)
    at = {o: i for i, o in enumerate(opens)}
    nodes, base = build_pool(n, lambda j: open_free(at[j]) if j in at else closed3(j))
    groups = []
    for d, dim in ((1, "memory"), (2, "ephemeral"), (0, "cpu")):
        pods, want, rows, carry = [], [], {}, 0
        for i, o in enumerate(opens):
            q = 5 + i
            run = open_free(i)[d] - carry - q
            a, b = run // 3, run // 4
            for x in (a, b, run - a - b):
                pods.append(one("%s%d" % (dim[0], len(pods)), d, x))
                want.append(o)
            pods.append(one("%s%d" % (dim[0], len(pods)), d, q + 1))
            want.append(opens[i + 1] if i + 1 < len(opens) else -1)
            pods.append(one("%s%d" % (dim[0], len(pods)), d, q))
            want.append(o)
            carry = q + 1
        pods.append(one("%s%d" % (dim[0], len(pods)), d, 3))
        want.append(-1)
        for k, j in enumerate(want):
            if j < 0:
                rows[k] = {BITS[d]: n}
        groups.append(Group("ladder_" + dim, pods, catches=("own_use_dim0_only", "dims_swapped") if d else (),
                            want=want, rows=rows))
    return ACase("dimensions_apart_%d" % n, nodes, base, groups, all_rows=n < 257)


def _crossed(n):
    """One candidate asking in all three dimensions.  Open nodes A = 0, B = 63, C = 64, D = last (0, 1, 63, 64 on 65 nodes); every other node
    j is full from the base in dimension j % 3 alone and has too little in the others for the four large pods.  The
    large pods exhaust A in cpu, B in memory, C in ephemeral storage and D in memory and ephemeral storage; the last
    pod asks 3 of each and is the blocker: CPU, MEMORY and EPHEMERAL each count their own nodes, D in two."""
    A, B, C, D = four(n)
    at = {o: i for i, o in enumerate((A, B, C, D))}

    def free(j):
        if j in at:
            return open_free(at[j])
        f = [50 + j % 7, 1000 + j, 2000 + j]
        f[j % 3] = (j // 3) % 3
        return tuple(f)
    nodes, base = build_pool(n, free)
    fa, fb, fc, fd = (open_free(i) for i in range(4))
    pods = [P("xa", cpu=fa[0], mem=3, eph=3), P("xb", cpu=3, mem=fb[1], eph=3), P("xc", cpu=3, mem=3, eph=fc[2]),
            P("xd", cpu=3, mem=fd[1], eph=fd[2]), P("xe", cpu=3, mem=3, eph=3)]
    shut = [j for j in range(n) if j not in at]
    row = {CPU: sum(1 for j in shut if j % 3 == 0) + 1, MEMORY: sum(1 for j in shut if j % 3 == 1) + 2,
           EPHEMERAL: sum(1 for j in shut if j % 3 == 2) + 2}
    g = Group("crossed", pods, catches=("own_use_dim0_only", "dims_swapped"), want=[A, B, C, D, -1], rows={4: row})
    return ACase("crossed_%d" % n, nodes, base, [g], all_rows=n < 257)


def _acc_apart_from_req(n):
    """One open node X; everything else has less than 3 left.  In memory and in ephemeral storage: an init container
    that asks nearly the whole node while the containers ask a fifth (the pod behind it fills the node and would not
    fit were req accounted); a pod with overhead (accounted and requested); and the converse pair, a first pod whose
    small acc matters because the later pod's init container asks one more than, or exactly, what is left."""
    X = {65: 63, 130: 64, 257: 256}[n]
    F = open_free(1)
    nodes, base = build_pool(n, lambda j: F if j == X else closed3(j))
    groups = []
    for d, dim in ((1, "memory"), (2, "ephemeral")):
        f, t = F[d], dim[0]
        m1 = f // 5 | 1
        groups.append(Group("init_container_" + dim,
                            [with_init(t + "i0", d, m1, f - 7), one(t + "i1", d, f - m1), one(t + "i2", d, 3)],
                            catches=("account_req", "own_use_dim0_only"), want=[X, X, -1], rows={2: {BITS[d]: n}}))
        c, o = f // 7, f // 9 | 1
        ov = Pod(t + "o0", containers=[Container(**{FIELD[d]: c})], overhead=Container(**{FIELD[d]: o}))
        groups.append(Group("overhead_" + dim, [ov, one(t + "o1", d, f - c - o), one(t + "o2", d, 3)],
                            catches=("own_use_dim0_only",), want=[X, X, -1], rows={2: {BITS[d]: n}}))
        groups.append(Group("later_init_refuses_" + dim,
                            [with_init(t + "r0", d, m1, 3), with_init(t + "r1", d, 3, f - m1 + 1)],
                            catches=("own_use_dim0_only",), want=[X, -1], rows={1: {BITS[d]: n}}))
        groups.append(Group("later_init_fits_" + dim,
                            [with_init(t + "f0", d, m1, 3), with_init(t + "f1", d, 3, f - m1),
                             one(t + "f2", d, f - m1 - 3), one(t + "f3", d, 3)],
                            catches=("account_req", "own_use_dim0_only"), want=[X, X, X, -1], rows={3: {BITS[d]: n}}))
    return ACase("acc_apart_from_req_%d" % n, nodes, base, groups, all_rows=n < 257)


def _zero_and_partial(n):
    """Zero and partial requests on nodes overcommitted from the base.  Only four nodes have a pod slot: X (three
    slots, memory FX), O2 behind it (one slot, cpu and memory overcommitted), Oc = n - 2 (one slot, cpu
    overcommitted, memory ample) and O = n - 1 (two slots, memory overcommitted, cpu ample).  Every other node has
    no slot and less than 3 of anything."""
    X = 64 if n > 70 else 32
    O2, Oc, O = X + 1, n - 2, n - 1
    FX = GiB + 4097
    special = {X: (2, FX, 2), O2: (-5, -7, 2), Oc: (-4, GiB + 77, 2), O: (500, -9, 2)}
    slots = {X: 3, O2: 1, Oc: 1, O: 2}
    over = {j: dict(pods=1 + slots.get(j, 0)) for j in range(n)}
    nodes, base = build_pool(n, lambda j: special.get(j, closed3(j)), over)

    def z(name):
        return P(name, cpu=0)
    groups = [
        # the group's own pods fill X to the byte; an all-zero pod still takes X's last slot and the next one the
        # overcommitted O2: fitsRequest returns before the compares
        Group("zero_after_fill", [one("zf0", 1, FX - 11), one("zf1", 1, 11), z("zf2"), z("zf3")],
              want=[X, X, X, O2]),
        # a cpu-only pod: O has the cpu and is refused for MEMORY alone (0 > free); O2 for CPU and MEMORY
        Group("cpu_only_on_overcommitted", [one("co0", 0, 5)], want=[-1],
              rows={0: {PODS: n - 4, CPU: n - 1, MEMORY: 2}}),
        # ... with own pods there: six all-zero pods take every slot but O's second
        Group("cpu_only_behind_own_pods", [z("cb%d" % k) for k in range(6)] + [one("cb6", 0, 5)],
              want=[X, X, X, O2, Oc, O, -1], rows={6: {PODS: n - 1, CPU: n - 1, MEMORY: 2}}),
        # a memory-only pod behind one that filled X: Oc has the memory and is refused for CPU alone
        Group("memory_only_on_overcommitted", [one("mo0", 1, FX), one("mo1", 1, 5)], want=[X, -1],
              catches=("own_use_dim0_only",), rows={1: {PODS: n - 4, MEMORY: n - 1, CPU: 2}}),
        Group("memory_only_behind_own_pods", [one("mb0", 1, FX)] + [z("mb%d" % k) for k in range(1, 5)] + [one("mb5", 1, 5)],
              want=[X, X, X, O2, Oc, -1], catches=("own_use_dim0_only",),
              rows={5: {PODS: n - 1, MEMORY: n - 1, CPU: 2}}),
    ]
    return ACase("zero_and_partial_%d" % n, nodes, base, groups, all_rows=n < 257)


LIST_N = 257
LIST_TARGETS = (1, 3, 63, 65, 127, 129, 139, 141, 191, 193, 219, 0, 2, 64, 128, 140, 192)
LIST_OVER = (10, 12, 62, 66, 126, 130, 136, 142, 150, 160, 170, 180, 194, 200, 202, 204, 210, 212, 214)


def _the_list(d):
    """k_blockers' sorted list with values in dimension d (memory or ephemeral storage), on 257 nodes.  Odd nodes
    have B_j left, even ones S_j < B_j; a big pod for node j asks B_j - r_j and fits untouched odd nodes only, a
    small one asks S_j - r_j, and r_j = 1000 + 3 j grows with j.  70 big pods take the odd nodes 1..139 (appends),
    70 small ones the even nodes 0..138: each is inserted between held entries, the first at position 0 under 70
    entries, the last under the 140th -- 32 of these shifts take an entry from lane 63 of slot 0 to lane 0 of slot
    1, six from slot 1 to slot 2.  40 big pods (141..219) and 40 small ones (140..218) do it again above 128
    entries, 14 times from slot 2 to slot 3.  The tail of 36 pods returns to held entries, most of them on odd nodes, which every later insert below
    them shifted: a pod of r_t fits node t and no lower one by that entry's sum alone; a pod of r_u + 1 is one over
    and moves up.  256 pods: the capacity.  `past` is the same
    list and one more pod, which goes the SINGLE way; `twenty` updates one entry in place twenty times."""
    n, dim = LIST_N, ("cpu", "memory", "ephemeral")[d]
    big0, small0 = ((3 * GiB, GiB), (3_000_000_001, 1_000_000_007))[d - 1]

    def left(j):
        return (big0 + 7 * j) if j % 2 else (small0 + 5 * j)

    def r(j):
        return 1000 + 3 * j

    def free(j):
        f = [500 + 3 * j, GiB + 2 * j + 1, 1_000_000_007 + 6 * j]
        f[d] = left(j)
        return tuple(f)
    nodes, base = build_pool(n, free, {j: dict(mem=4 * GiB + 2 * j + 1) for j in range(n)})
    order = list(range(1, 140, 2)) + list(range(0, 140, 2)) + list(range(141, 220, 2)) + list(range(140, 220, 2))
    assert len(order) == 220 and len(set(order)) == 220
    asks = [left(j) - r(j) for j in order] + [r(t) for t in LIST_TARGETS] + [r(u) + 1 for u in LIST_OVER]
    assert len(asks) == CAP
    t = dim[0]
    at_cap = [one("%sc%d" % (t, k), d, x) for k, x in enumerate(asks)]
    past = [one("%sp%d" % (t, k), d, x) for k, x in enumerate(asks + [3])]
    s0 = left(0)
    twenty = [one("%st%d" % (t, k), d, s0 // 20) for k in range(19)] + [one("%st19" % t, d, s0 - 19 * (s0 // 20))]
    twenty.append(one("%st20" % t, d, 3))
    catches = ("shift_dim0_only", "own_use_dim0_only")
    groups = [Group("at_capacity", at_cap, catches=catches),
              Group("past_capacity", past, catches=catches, how_b=SINGLE),
              Group("twenty_in_place", twenty, catches=("own_use_dim0_only",), want=[0] * 20 + [1])]
    # the head of the answer, by construction
    for g in groups[:2]:
        g.want = None
    return ACase("the_list_in_%s" % dim, nodes, base, groups, all_rows=False), order, list(LIST_TARGETS)


def _sums_of_64_bits(n):
    """Sums past 2^32, 2^53 and 2^60.  H has 2^61 + 3096 bytes of memory left, H2 behind it 2^60 - 100, He
    2^45 + 12301 bytes of ephemeral storage, Hc 3 * 2^32 + 770 millicores; T is a full node whose Requested memory,
    2^60 + 333, is the pool's largest; every other node has nothing left in any dimension, so a pod of one byte is
    a probe."""
    H, H2, He, Hc, T = {65: (63, 64, 0, 1, 2), 130: (64, 129, 63, 0, 65)}[n]
    FH, FH2, FE, FC = (1 << 61) + 3096, (1 << 60) - 100, (1 << 45) + 12301, 3 * (1 << 32) + 770
    top = (1 << 60) + 333
    over = {H: dict(mem=FH + 1001), H2: dict(mem=FH2 + 105), He: dict(eph=FE + 46), Hc: dict(cpu=FC + 7), T: dict(mem=top)}
    special = {H: (0, FH, 0), H2: (0, FH2, 0), He: (0, 0, FE), Hc: (FC, 0, 0)}
    nodes, base = build_pool(n, lambda j: special.get(j, (0, 0, 0)), over)
    G = 1 << 32

    def seq(t, d, xs):
        return [one("%s%d" % (t, k), d, x) for k, x in enumerate(xs)]
    total = QUANTITY_END - 1 - top        # the largest total acc the plain rule takes in memory
    pa = (1 << 61) + 3000
    pb = total - pa
    assert 0 < pb < FH2 and pb > FH - pa
    groups = [
        Group("past_2_32", seq("a", 1, [G + 5, 2 * G + 7, FH - (3 * G + 12), G]), catches=("trunc32",),
              want=[H, H, H, H2]),
        # 2^53 + 1 is the first integer a double does not hold: the byte behind it decides
        Group("past_2_53", seq("b", 1, [1 << 53, 1, FH - (1 << 53) - 1, 1]), catches=("trunc32",), want=[H, H, H, H2]),
        Group("past_2_60", seq("c", 1, [(1 << 59) + 3, (1 << 59) + 5, 5 * G + 1, FH - (1 << 60) - 5 * G - 9, 1]),
              catches=("trunc32",), want=[H, H, H, H, H2]),
        Group("ephemeral_2_40_to_2_45", seq("e", 2, [(1 << 40) + 1, (1 << 41) + 3, (1 << 44) + 5, 3 * G,
                                                       FE - (1 << 40) - (1 << 41) - (1 << 44) - 3 * G - 9, 1, G]),
              catches=("trunc32",), want=[He] * 5 + [-1, -1], rows={5: {EPHEMERAL: n}, 6: {EPHEMERAL: n}}),
        Group("cpu_2_33", seq("m", 0, [G + 1, G + 3, FC - 2 * G - 4, G, 1]), catches=("trunc32",),
              want=[Hc, Hc, Hc, -1, -1], rows={3: {CPU: n}, 4: {CPU: n}}),
        # the limit as a limit: the largest Requested plus the group's total acc is 2^62 - 1
        Group("at_the_quantity_limit", seq("l", 1, [pa, pb]), want=[H, H2]),
        # ... and one byte more: the pods still land on different nodes, no node's Requested leaves the range
        Group("past_the_quantity_limit", seq("o", 1, [pa, pb + 1]), want=[H, H2], how_b=SINGLE, how_e=NOT_PLAIN),
        Group("neighbour", seq("n", 1, [G + 5, FH - G - 5, 7]), catches=("trunc32",), want=[H, H, H2]),
    ]
    return ACase("sums_of_64_bits_%d" % n, nodes, base, groups)


def _the_undo(n):
    """Three scenarios for one block of k_evacuate, in this order.

    The pool: S = 0 (two pod slots, 50m cpu, 200 GiB + 1 of memory left), M = 64 (49m, 64 GiB + 3), E = n - 1 (48m,
    2^37 + 5 bytes of ephemeral storage); every other node has ample cpu, room for c_j memory pods and e_j ephemeral
    pods of X, and nothing near what S, M and E have.
    X loses nodes 1 and 65 and moves 300 pods.  Pods 0..255 ask 100m of cpu, so S, M and E never take one; they ask
    memory, ephemeral storage or both and fill the pool through its last row word; every 50th asks 500 GiB and is
    stranded.  Pods 256.. ask 1m: two take S's slots, one fills M's memory to the byte, one E's ephemeral storage,
    the rest pile on low nodes -- all of them behind the first 256 pods, which is what the undo's second stride
    visits with the default block.
    Y's pods fit only where X left nothing: y_s on S by the pod count alone, y_m on M by memory alone, y_e on E by
    ephemeral storage alone.  Cpu is ample for them everywhere.
    Z loses M and node 2 and moves four pods."""
    S, M, E = 0, 64, n - 1
    FS, FM, FE = 200 * GiB + 1, 64 * GiB + 3, (1 << 37) + 5
    UM, UE = 900 * (1 << 20), 700_000_001
    if n == 130:
        cm, ce = (lambda j: 1 + j % 2), (lambda j: 1)
    else:
        cm, ce = (lambda j: int(j % 4 != 3)), (lambda j: j % 2)

    def free(j):
        if j == S:
            return (50, FS, 11)
        if j == M:
            return (49, FM, 13)
        if j == E:
            return (48, 15, FE)
        return (990 + 6 * j, cm(j) * (UM + 1000) + 2 * j + 1, ce(j) * (UE + 1000) + 2 * j + 3)
    over = {j: dict(mem=256 * GiB + 2 * j + 1, eph=(1 << 38) + 1_000_003 * j) for j in range(n)}
    over[S]["pods"] = 3
    nodes, base = build_pool(n, free, over)
    x = []
    for k in range(BLOCK_THREADS):
        kind = k % 4
        mem = UM + 2 * k + 1 if kind in (0, 2, 3) else 0
        eph = UE + 2 * k + 1 if kind in (1, 2) else 0
        if k % 50 == 49:
            mem, eph = 500 * GiB, 0
        x.append(P("x%d" % k, cpu=100, mem=mem, eph=eph))
    x += [P("x256", cpu=1), P("x257", cpu=1), P("x258", cpu=1, mem=FM), P("x259", cpu=1, eph=FE)]
    x += [P("x%d" % k, cpu=1, mem=7 + k) for k in range(260, 299)] + [P("x299", cpu=1, mem=500 * GiB)]
    assert len(x) == 300
    y = [P("ys", cpu=1, mem=FS - 5), P("ym", cpu=1, mem=FM), P("ye", cpu=1, eph=FE)]
    z = [P("z0", cpu=1, mem=FM), P("z1", cpu=1, eph=FE), P("z2", cpu=1, mem=150 * GiB), P("z3", cpu=100, mem=UM + 1)]
    groups = [Group("X", x, lost=[1, 65]),
              Group("Y", y, want=[S, M, E]),
              Group("Z", z, lost=[M, 2], want=[S, E, -1, 1], rows={2: {MEMORY: n - 2}})]
    return ACase("the_undo_%d" % n, nodes, base, groups, all_rows=n < 257,
                 orders=((0, 1, 2), (2, 1, 0), (0, 1, 0, 1)), seq_catches=("stale_deltas", "undo_first", "undo_dim0_only"))


UNDO_T = BLOCK_THREADS  # undo_first's T: what the first stride of the default block visits


def cases() -> List[ACase]:
    out = []
    for n in (65, 130, 257):
        out += [_dimensions_apart(n), _crossed(n), _acc_apart_from_req(n), _zero_and_partial(n)]
    out += [_the_list(1)[0], _the_list(2)[0]]
    out += [_sums_of_64_bits(65), _sums_of_64_bits(130)]
    out += [_the_undo(130), _the_undo(257)]
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
    """A case as one cluster: the scenario, the loop's inputs in plain integers, the right answer of every group
    on its own, and the arrays of both calls."""

    def __init__(self, case: ACase):
        import numpy as np
        from helpers import Scenario
        self.case = case
        self.n_spot = len(case.nodes)
        flat = [p for g in case.groups for p in g.pods]
        self.sc = Scenario(case.nodes, case.base, flat)
        self.ids, i = [], 0
        for g in case.groups:
            self.ids.append([self.sc.qidx(i + k) for k in range(len(g.pods))])
            i += len(g.pods)
        self.free = []
        for nd, ps in zip(case.nodes, case.base):
            use = [sum(p.node_accounting()[d] for p in ps) for d in range(3)]
            self.free.append((nd.cpu_milli - use[0], nd.memory - use[1], nd.ephemeral - use[2]))
        self.slack = [nd.pods - len(ps) for nd, ps in zip(case.nodes, case.base)]
        self.mpods = [[mpod(p) for p in g.pods] for g in case.groups]
        self.right = [loop(self.free, self.slack, [(self.mpods[i], g.lost)])[0] for i, g in enumerate(case.groups)]
        for g, (mapping, rows) in zip(case.groups, self.right):
            if g.want is not None:
                assert mapping == g.want, (case.name, g.name, mapping)
            for k, row in g.rows.items():
                assert rows[k] == row, (case.name, g.name, k, rows[k])
        # sr_blockers_plan: the groups without a lost set, in order
        self.cands = [i for i, g in enumerate(case.groups) if not g.lost]
        self.cand_off = np.zeros(len(self.cands) + 1, np.int32)
        self.cand_off[1:] = np.cumsum([len(self.ids[i]) for i in self.cands])
        self.cand_pods = np.array([p for i in self.cands for p in self.ids[i]], np.int32)
        self.ask = np.zeros(len(self.cands), np.int32)
        self.how_b = np.array([case.groups[i].how_b for i in self.cands], np.uint8)

    def wrong(self, i, variant, T=UNDO_T):
        """Group i on its own under a wrong variant."""
        return loop(self.free, self.slack, [(self.mpods[i], self.case.groups[i].lost)], variant, T)[0]

    def sequence(self, order, variant=None, T=UNDO_T):
        """The groups `order` as one block takes them."""
        return loop(self.free, self.slack, [(self.mpods[i], self.case.groups[i].lost) for i in order], variant, T)

    def scen_args(self, order=None, nothing_lost=False):
        """(scen_off, scen_pods, lost_off, lost_pos) for the groups `order` (default: all, in order)."""
        from evacuate_ref import scenarios
        order = list(range(len(self.case.groups))) if order is None else list(order)
        lost = [[] if nothing_lost else self.case.groups[i].lost for i in order]
        return scenarios(self.sc, lost, moved=[self.ids[i] for i in order])

    def pinned(self, order=None):
        """flat pod index (in the arrays of scen_args(order)) -> counts row, for the rows written out by hand."""
        order = list(range(len(self.case.groups))) if order is None else list(order)
        out, p0 = {}, 0
        for i in order:
            for k, row in self.case.groups[i].rows.items():
                out[p0 + k] = why_row(row)
            p0 += len(self.ids[i])
        return out

    def pinned_cands(self):
        out, p0 = {}, 0
        for i in self.cands:
            for k, row in self.case.groups[i].rows.items():
                out[p0 + k] = why_row(row)
            p0 += len(self.ids[i])
        return out
