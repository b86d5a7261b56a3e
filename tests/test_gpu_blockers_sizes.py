"""sr_blockers_plan at the smallest shapes at which the kernel can go wrong: pools of 1, 63, 64, 65, 129 and 257
nodes (one lane, a ragged word whose pad lanes must stay out, a full word, one node past it, a third and a
fifth word); the only feasible node last, in the last lane of a word and in the first lane of the next; the
context list grown in and out of node order over a word boundary, at its capacity and one pod past it (which
must go the SINGLE way with the same answer); every placement on one node against one node each; more waves
than one block; a blocker refused for a non-resource reason beside a resource-only one.  The reference is the
contract's loop over the oracle (tests/blockers_ref.py); where the answer is short it is also written out."""
import numpy as np
import pytest

import blockers_cases as B
from blockers_ref import oracle_blockers_plan
from explain_plan_cases import pool
from helpers import Scenario
from known_answer import P, used
from spotplanner import capi
from spotplanner.model import Container, Pod
from spotplanner.rescheduler import blockers_plan_arrays
from test_gpu_blockers import check_rows
from test_gpu_shortfall import snapshot

pytestmark = pytest.mark.gpu

POOLS = (1, 63, 64, 65, 129, 257)
CAP = capi.SR_BLOCKERS_BATCH_PODS
CPU_R, AFF_R = capi.WHY_NAMES.index("CPU"), capi.WHY_NAMES.index("NODE_AFFINITY")


def build(nodes, base, cands):
    flat = [p for c in cands for p in c]
    sc = Scenario(nodes, base, flat)
    cand_off = np.zeros(len(cands) + 1, np.int32)
    cand_off[1:] = np.cumsum([len(c) for c in cands])
    cand_pods = np.array([sc.qidx(i) for i in range(len(flat))], np.int32)
    return sc, cand_off, cand_pods


def run(checker, sc, cand_off, cand_pods, rows=True):
    """The call with and without counts, against the oracle loop; every blocker's row against
    sr_explain_candidate on the compacted list."""
    n, n_spot = len(cand_off) - 1, len(sc.spot)
    ask = np.zeros(n, np.int32)
    with snapshot(sc) as h:
        res = blockers_plan_arrays(checker, h, sc.ptr, cand_off, cand_pods, ask)
        bare = blockers_plan_arrays(checker, h, sc.ptr, cand_off, cand_pods, ask, counts=False)
        if rows:
            for c in range(n):
                check_rows(checker, h, sc, cand_off, cand_pods, res, c)
    ref = oracle_blockers_plan(sc, sc.oracle_snapshot(), cand_off, cand_pods, ask, n_spot)
    for f in ("blockers", "first", "node_of_pod", "fallback"):
        assert np.array_equal(getattr(res, f), ref[f]), f
        assert np.array_equal(getattr(res, f), getattr(bare, f)), f
    assert np.array_equal(res.how, bare.how)
    return res


def open_nodes(n):
    """The single open node of a pool otherwise full: the last one, and around the first word boundary."""
    return sorted({n - 1} | ({63, 64} if n > 64 else set()))


@pytest.mark.parametrize("n", POOLS)
def test_the_only_feasible_node(checker, n):
    """Every node but one is full.  600m goes there, 600m more fits nowhere (cpu on all n nodes), 400m fills it,
    one milli more fits nowhere; a candidate of one pod beside it."""
    for at in open_nodes(n):
        base = [[used(cpu=1000)] if j != at else [] for j in range(n)]
        cands = [[P("a0", cpu=600), P("a1", cpu=600), P("a2", cpu=400), P("a3", cpu=1)], [P("b0", cpu=1000)],
                 [P("c0", cpu=1001)]]
        sc, cand_off, cand_pods = build(pool(n), base, cands)
        res = run(checker, sc, cand_off, cand_pods)
        assert list(res.node_of_pod) == [at, -1, at, -1, at, -1], (n, at)
        assert list(res.blockers) == [2, 0, 1] and list(res.first) == [1, -1, 0]
        assert (res.how == B.BATCHED).all()
        for i in (1, 3, 5):
            assert res.counts[i][CPU_R] == n and res.counts[i].sum() == n, (n, at, i)


@pytest.mark.parametrize("n", POOLS)
def test_one_node_against_one_node_each(checker, n):
    """Twenty 1m pods all land on node 0 (one entry, updated in place); twenty 600m pods take a node each in
    order (appends), the ones past the pool are blockers."""
    cands = [[P("s%d" % k, cpu=1) for k in range(20)], [P("l%d" % k, cpu=600) for k in range(20)]]
    sc, cand_off, cand_pods = build(pool(n), [[] for _ in range(n)], cands)
    res = run(checker, sc, cand_off, cand_pods)
    assert list(res.node_of_pod[:20]) == [0] * 20
    assert list(res.node_of_pod[20:]) == [k if k < n else -1 for k in range(20)]
    assert list(res.blockers) == [0, max(0, 20 - n)]


def zigzag(n, pods):
    """A pool whose first ten nodes have 350m left and the rest 1000m, and `pods` pods alternating 600m / 300m:
    a large pod opens the next fresh node from 10 on, a small one goes to the lowest node with 300m left -- the
    half-full early nodes first, in front of everything the list holds."""
    base = [[used(cpu=650)] if j < 10 else [] for j in range(n)]
    return pool(n), base, [P("z%d" % k, cpu=600 if k % 2 == 0 else 300) for k in range(pods)]


def first_fit_cpu(free, pods):
    out = []
    for cpu in pods:
        at = next((j for j, f in enumerate(free) if f >= cpu), -1)
        out.append(at)
        if at >= 0:
            free[at] -= cpu
    return out


@pytest.mark.parametrize("n", (65, 129, 257))
def test_the_list_at_its_capacity_and_past_it(checker, n):
    """Capacity pods and capacity + 1, placed out of node order, so entries are inserted in front of and between
    the ones the list holds: the longer candidate goes the SINGLE way and gets the same answer."""
    nodes, base, at_cap = zigzag(n, CAP)
    _, _, past = zigzag(n, CAP + 1)
    # a node each, the ten half-full ones first: with 257 nodes the list grows to exactly CAP entries
    tail_cpu = [350] * 10 + [990] * (CAP - 10)
    tail = [P("t%d" % k, cpu=cpu) for k, cpu in enumerate(tail_cpu)]
    sc, cand_off, cand_pods = build(nodes, base, [at_cap, past, tail])
    res = run(checker, sc, cand_off, cand_pods, rows=n == 65)
    assert list(res.how) == [B.BATCHED, B.SINGLE, B.BATCHED]
    free = [350 if j < 10 else 1000 for j in range(n)]
    want = first_fit_cpu(list(free), [600 if k % 2 == 0 else 300 for k in range(CAP + 1)])
    assert list(res.node_of_pod[:CAP]) == want[:CAP]
    assert list(res.node_of_pod[CAP:2 * CAP + 1]) == want
    assert list(res.node_of_pod[2 * CAP + 1:]) == first_fit_cpu(list(free), tail_cpu)
    assert res.blockers[0] == want[:CAP].count(-1) and res.blockers[1] == want.count(-1)
    assert res.blockers[2] == max(0, CAP - n)  # the pool runs out: blockers behind a list over every word
    if n > CAP:
        assert len(set(res.node_of_pod[2 * CAP + 1:])) == CAP and res.node_of_pod[-1] == CAP - 1


def test_more_waves_than_one_block(checker):
    """300 candidates of one pod on 65 nodes with one open node (64): the pods of 1001m are blockers."""
    n = 65
    base = [[used(cpu=1000)] if j != 64 else [] for j in range(n)]
    cands = [[P("p%d" % c, cpu=1001 if c % 7 == 3 else 10 + c)] for c in range(300)]
    sc, cand_off, cand_pods = build(pool(n), base, cands)
    res = run(checker, sc, cand_off, cand_pods, rows=False)
    assert list(res.node_of_pod) == [-1 if c % 7 == 3 else 64 for c in range(300)]
    assert list(res.blockers) == [int(c % 7 == 3) for c in range(300)]
    assert all(res.counts[c][CPU_R] == n for c in range(300) if c % 7 == 3)
    assert not any(res.counts[c].any() for c in range(300) if c % 7 != 3)


@pytest.mark.parametrize("n", (63, 129))
def test_a_non_resource_blocker_beside_a_resource_one(checker, n):
    """A pod pinned by a selector no node carries is refused everywhere by NODE_AFFINITY alone; the 1001m pod
    behind it by cpu alone; a pinned pod that is also too large by both.  The placed pods around them do not
    care."""
    def pinned(name, cpu):
        return Pod(name, containers=[Container(cpu_milli=cpu)], node_selector={"disk": "nvme"})
    cands = [[P("a0", cpu=600), pinned("a1", 10), P("a2", cpu=1001), pinned("a3", 1001), P("a4", cpu=400)]]
    sc, cand_off, cand_pods = build(pool(n), [[] for _ in range(n)], cands)
    res = run(checker, sc, cand_off, cand_pods)
    assert list(res.node_of_pod) == [0, -1, -1, -1, 0] and list(res.blockers) == [3] and res.how[0] == B.BATCHED
    rows = res.counts
    assert rows[1][AFF_R] == n and rows[1].sum() == n
    assert rows[2][CPU_R] == n and rows[2].sum() == n
    assert rows[3][AFF_R] == n and rows[3][CPU_R] == n and rows[3].sum() == 2 * n
