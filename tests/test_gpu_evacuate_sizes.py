"""sr_evacuate_plan at the smallest shapes at which the kernel can go wrong: pools of 1, 63, 64, 65, 130 and 257
nodes (one lane, a ragged word whose pad lanes must stay out, a full word, one node past it, a third word, and
64 W + 1 for the default W = 4 waves a block: a second round of row words); lost positions at bit 0, bit 63, bit
64 and the last node, alone and together, none and all; a lost node that is the only one admitting a pod; one
scenario of 300 pods, past sr_blockers_plan's batch limit, with the same answer as that call's SINGLE way; more
scenarios than blocks (SR_EVAC_GRID=1), the scenario list reversed, and 1, 2 and the default number of waves a
block.  The reference is the oracle on really reduced snapshots (tests/evacuate_ref.py); where the answer is short
it is also worked out here."""
import numpy as np
import pytest

import evacuate_cases as E
from evacuate_ref import oracle_evacuate_plan, scenarios
from explain_plan_cases import pool
from helpers import Scenario
from known_answer import P, used
from spotplanner import capi
from spotplanner.rescheduler import blockers_plan_arrays, evacuate_plan_arrays
from test_gpu_evacuate import check_rows, same_but_counts
from test_gpu_shortfall import snapshot

pytestmark = pytest.mark.gpu

DEFAULT_WAVES = 4  # kEvacWaves (csrc/evacuate.hpp)
POOLS = (1, 63, 64, 65, 130, 64 * DEFAULT_WAVES + 1)
CPU_R, PODS_R = capi.WHY_NAMES.index("CPU"), capi.WHY_NAMES.index("PODS")


def edge_positions(n):
    return sorted({0, n - 1} | ({63} if n > 63 else set()) | ({64} if n > 64 else set()))


def first_fit_cpu(free, pods, lost):
    free, out = list(free), []
    for cpu in pods:
        at = next((j for j, f in enumerate(free) if j not in lost and f >= cpu), -1)
        out.append(at)
        if at >= 0:
            free[at] -= cpu
    return out


def run(checker, sc, args, rows=True):
    """The call with and without counts against the reduced-snapshot oracle; every stranded pod's row against
    sr_explain_candidate on the reduced product snapshot."""
    scen_off, scen_pods, lost_off, lost_pos = args
    with snapshot(sc) as h:
        res = evacuate_plan_arrays(checker, h, sc.ptr, *args)
        bare = evacuate_plan_arrays(checker, h, sc.ptr, *args, counts=False)
    same_but_counts(res, bare)
    ref = oracle_evacuate_plan(sc, *args)
    assert (res.how == E.JUDGED).all()
    for f in ("stranded", "first", "node_of_pod"):
        assert np.array_equal(getattr(res, f), ref[f]), f
    if rows:
        for s in range(len(scen_off) - 1):
            check_rows(checker, sc, scen_off, scen_pods, lost_pos[int(lost_off[s]):int(lost_off[s + 1])], res, s)
    return res


@pytest.mark.parametrize("n", POOLS)
def test_lost_positions_at_the_word_edges(checker, n):
    """Even nodes have 400m left, odd ones 1000m.  Each edge position lost alone, all of them together, none and
    all; every scenario moves the same five pods, so only the lost set decides."""
    free = [400 if j % 2 == 0 else 1000 for j in range(n)]
    base = [[used(cpu=600, name="u%d" % j)] if j % 2 == 0 else [] for j in range(n)]
    cpus = [700, 300, 300, 700, 1001]
    moved = [P("m%d" % k, cpu=c) for k, c in enumerate(cpus)]
    sc = Scenario(pool(n), base, moved)
    edges = edge_positions(n)
    lost_sets = [[j] for j in edges] + [list(reversed(edges)), [], list(range(n))]
    args = scenarios(sc, lost_sets, moved=[[sc.qidx(k) for k in range(len(moved))]] * len(lost_sets))
    res = run(checker, sc, args)
    for s, lost in enumerate(lost_sets):
        want = first_fit_cpu(free, cpus, set(lost))
        assert list(res.node_of_pod[5 * s:5 * s + 5]) == want, (n, lost)
        assert res.stranded[s] == want.count(-1)
        # the 1001m pod meets cpu on every surviving node, and no other node is counted
        row = res.counts[5 * s + 4]
        assert row[CPU_R] == n - len(lost) and row.sum() == n - len(lost), (n, lost)


@pytest.mark.parametrize("n", POOLS)
def test_the_lost_node_is_the_only_one_admitting(checker, n):
    """Every node but one is full.  Losing that one strands the pod (cpu on all n - 1 survivors); losing another
    one, or none, leaves it where it fits."""
    for at in edge_positions(n):
        base = [[used(cpu=1000, name="u%d" % j)] if j != at else [] for j in range(n)]
        pod = P("a0", cpu=600)
        sc = Scenario(pool(n), base, [pod])
        other = next((j for j in (0, n - 1) if j != at), None)
        lost_sets = [[at], []] + ([[other]] if other is not None else [])
        args = scenarios(sc, lost_sets, moved=[[sc.qidx(0)]] * len(lost_sets))
        res = run(checker, sc, args, rows=n <= 65)
        assert list(res.node_of_pod) == [-1, at] + ([at] if other is not None else []), (n, at)
        assert res.counts[0][CPU_R] == n - 1 and res.counts[0].sum() == n - 1


@pytest.mark.parametrize("n", (65, 64 * DEFAULT_WAVES + 1))
def test_three_hundred_pods_as_sr_blockers_plan_places_them(checker, n):
    """One scenario of 300 pods with nothing lost is sr_blockers_plan's loop on the snapshot as it is: that call
    takes its SINGLE way past SR_BLOCKERS_BATCH_PODS, this one judges it, and every output is the same."""
    count = 300
    assert count > capi.SR_BLOCKERS_BATCH_PODS
    nodes = pool(n, over={j: dict(pods=4) for j in range(0, n, 3)})
    base = [[used(cpu=650, name="u%d" % j)] if j < 10 else [] for j in range(n)]
    pods = [P("z%d" % k, cpu=(600, 300, 0, 1001)[k % 4] if k % 50 else 990) for k in range(count)]
    sc = Scenario(nodes, base, pods)
    ids = [sc.qidx(k) for k in range(count)]
    args = scenarios(sc, [[]], moved=[ids])
    with snapshot(sc) as h:
        ev = evacuate_plan_arrays(checker, h, sc.ptr, *args)
        bl = blockers_plan_arrays(checker, h, sc.ptr, args[0], args[1], np.zeros(1, np.int32))
    assert list(bl.how) == [capi.SR_EXPLAIN_SINGLE] and list(ev.how) == [E.JUDGED]
    assert np.array_equal(ev.node_of_pod, bl.node_of_pod)
    assert list(ev.stranded) == list(bl.blockers) and list(ev.first) == list(bl.first)
    assert np.array_equal(ev.counts, bl.counts)
    assert ev.stranded[0] >= count // 4 and (ev.node_of_pod >= 0).sum() > 100  # both kinds in numbers
    assert ev.counts[:, PODS_R].max() > 0  # pod slots ran out on the way
    # ... and with the first and the last node lost the reduced-snapshot oracle agrees
    run(checker, sc, scenarios(sc, [[0, n - 1]], moved=[ids]), rows=False)


def reuse_input():
    """130 nodes with 0, 300, 600 or 900m left, 40 scenarios: node 3 s lost (with node 129 - s from the tenth on),
    each moving its lost nodes' pods and three pods of its own."""
    n = 130
    base = [[used(cpu=100 + 300 * (j % 4), name="u%d" % j)] for j in range(n)]
    extra = [P("x%d" % k, cpu=(250, 550, 1001)[k % 3]) for k in range(3)]
    sc = Scenario(pool(n), base, extra)
    lost_sets = [[3 * s] + ([129 - s] if s >= 10 else []) for s in range(40)]
    moved = [[sc.node_pod_idx[sc.node_pod_off[j]] for j in sorted(lost)] + [sc.qidx(k) for k in range(3)] for lost in lost_sets]
    return sc, lost_sets, moved


def test_more_scenarios_than_blocks_any_order_any_waves(checker, monkeypatch):
    """A block that takes scenario after scenario must hand each one a clean slice: one block for all forty,
    against the default grid; the list reversed; 1, 2 and the default number of waves a block."""
    sc, lost_sets, moved = reuse_input()
    args = scenarios(sc, lost_sets, moved=moved)
    res = run(checker, sc, args, rows=False)
    assert (res.stranded > 0).all() and (res.node_of_pod >= 0).sum() >= 80
    n = len(lost_sets)

    def call(a):
        with snapshot(sc) as h:
            return evacuate_plan_arrays(checker, h, sc.ptr, *a)

    def same(a, b):
        same_but_counts(a, b)
        assert np.array_equal(a.counts, b.counts)
    monkeypatch.setenv("SR_EVAC_GRID", "1")
    same(call(args), res)
    monkeypatch.setenv("SR_EVAC_GRID", "3")
    same(call(args), res)
    monkeypatch.delenv("SR_EVAC_GRID")
    for waves in (1, 2, 16):
        monkeypatch.setenv("SR_EVAC_WAVES", str(waves))
        same(call(args), res)
        monkeypatch.setenv("SR_EVAC_GRID", "1")
        same(call(args), res)
        monkeypatch.delenv("SR_EVAC_GRID")
    monkeypatch.delenv("SR_EVAC_WAVES")
    # reversed: scenario s of the reversed list is scenario n - 1 - s
    back = scenarios(sc, lost_sets[::-1], moved=moved[::-1])
    for grid in (None, "1"):
        if grid:
            monkeypatch.setenv("SR_EVAC_GRID", grid)
        rev = call(back)
        for s in range(n):
            t = n - 1 - s
            assert rev.stranded[t] == res.stranded[s] and rev.first[t] == res.first[s] and rev.how[t] == res.how[s]
            a, b = slice(int(res.scen_off[s]), int(res.scen_off[s + 1])), slice(int(rev.scen_off[t]), int(rev.scen_off[t + 1]))
            assert np.array_equal(res.node_of_pod[a], rev.node_of_pod[b]) and np.array_equal(res.counts[a], rev.counts[b])
    # the same context afterwards: the default shape again
    monkeypatch.delenv("SR_EVAC_GRID")
    same(call(args), res)
