"""sr_evacuate_plan on the GPU: the hand cases of tests/evacuate_cases.py through the C ABI, random clusters
against the oracle on really reduced snapshots (tests/evacuate_ref.py) and, stranded pod by stranded pod, against
sr_explain_candidate on a product snapshot built without the lost nodes; optional outputs, argument errors, the
Pod / Node mirror with its ranking, and planning around a call."""
import ctypes

import numpy as np
import pytest

import evacuate_cases as E
from evacuate_ref import compacted, oracle_evacuate_plan, reduced_product
from spotplanner import capi
from spotplanner.rescheduler import PlannerError, evacuate_plan_arrays, explain_candidate_arrays, plan_arrays
from test_evacuate_reference import RUN_IDS, RUNS, random_scenarios
from test_gpu_explain import _node_states, _steady_scenario
from test_gpu_k2_dispatch import make_checker

pytestmark = pytest.mark.gpu

CASES = E.cases()


def same_but_counts(a, b):
    for f in ("stranded", "first", "node_of_pod", "how"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def check_rows(checker, sc, scen_off, scen_pods, lost, res, s):
    """Every stranded pod's counts row of scenario s is sr_explain_candidate's for the compacted list on a product
    snapshot built without the lost nodes (positions remapped); every other row is zero."""
    base = int(scen_off[0])
    lo, hi = int(scen_off[s]), int(scen_off[s + 1])
    row = res.node_of_pod[lo - base:hi - base]
    if res.stranded[s] <= 0:
        assert not res.counts[lo - base:hi - base].any(), s
        return
    h, keep = reduced_product(sc, lost)
    back = {j: i for i, j in enumerate(keep)}
    try:
        for k in range(hi - lo):
            if row[k] >= 0:
                assert not res.counts[lo - base + k].any(), (s, k)
                continue
            pods, mapping, at = compacted(scen_pods[lo:hi], row, k)
            mapping = [back[j] if j >= 0 else -1 for j in mapping]
            one = explain_candidate_arrays(checker, h, sc.ptr, np.array(pods, np.int32), np.array(mapping, np.int32), at,
                                           node_mask=False)
            assert one.fallback[0] == 0 and one.feasible[0] == 0 and one.first[0] == -1, (s, k)
            assert np.array_equal(res.counts[lo - base + k], one.counts[0]), (s, k)
    finally:
        capi.load_planner().sr_snapshot_destroy(h)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_hand_cases(checker, case):
    b = E.Built(case)
    lib = capi.load_planner()
    h = b.sc.product_snapshot()
    try:
        before = _node_states(lib, h, b.n_spot)
        res = evacuate_plan_arrays(checker, h, b.sc.ptr, b.scen_off, b.scen_pods, b.lost_off, b.lost_pos)
        bare = evacuate_plan_arrays(checker, h, b.sc.ptr, b.scen_off, b.scen_pods, b.lost_off, b.lost_pos, counts=False)
        assert _node_states(lib, h, b.n_spot) == before
        assert list(res.how) == list(b.how)
        assert list(res.node_of_pod) == list(b.node_of_pod)
        assert list(res.stranded) == list(b.stranded) and list(res.first) == list(b.first)
        assert bare.counts is None
        same_but_counts(res, bare)
        for i, row in b.pinned.items():
            assert list(res.counts[i]) == row, i
        for s, sn in enumerate(case.scens):
            check_rows(checker, b.sc, b.scen_off, b.scen_pods, sn.lost, res, s)
    finally:
        lib.sr_snapshot_destroy(h)


@pytest.mark.parametrize("kind,seed", RUNS, ids=RUN_IDS)
def test_random_clusters(checker, kind, seed):
    """Every spot node lost alone and the two pools: each judged scenario is the reduced-snapshot oracle's, and the
    stranded pods' rows are sr_explain_candidate's on the reduced product snapshot."""
    sc, scen_off, scen_pods, lost_off, lost_pos = random_scenarios(kind, seed)
    n_spot, n = len(sc.spot), len(scen_off) - 1
    lib = capi.load_planner()
    h = sc.product_snapshot()
    try:
        before = _node_states(lib, h, n_spot)
        res = evacuate_plan_arrays(checker, h, sc.ptr, scen_off, scen_pods, lost_off, lost_pos)
        assert _node_states(lib, h, n_spot) == before
        same_but_counts(res, evacuate_plan_arrays(checker, h, sc.ptr, scen_off, scen_pods, lost_off, lost_pos, counts=False))
    finally:
        lib.sr_snapshot_destroy(h)
    ref = oracle_evacuate_plan(sc, scen_off, scen_pods, lost_off, lost_pos)
    judged = [s for s in range(n) if res.how[s] == E.JUDGED]
    rows = 0
    for s in range(n):
        lo, hi = int(scen_off[s]), int(scen_off[s + 1])
        if res.how[s] != E.JUDGED:
            assert res.how[s] in (E.NOT_PLAIN, E.FALLBACK)
            if res.how[s] == E.FALLBACK:
                assert ref["fallback"][s] == 1
            assert res.stranded[s] == -1 and res.first[s] == -1
            assert (res.node_of_pod[lo:hi] == -1).all() and not res.counts[lo:hi].any()
            continue
        assert ref["fallback"][s] == 0
        assert res.stranded[s] == ref["stranded"][s] and res.first[s] == ref["first"][s], s
        assert np.array_equal(res.node_of_pod[lo:hi], ref["node_of_pod"][lo:hi]), s
        lost = lost_pos[int(lost_off[s]):int(lost_off[s + 1])]
        check_rows(checker, sc, scen_off, scen_pods, lost, res, s)  # (zero rows where nothing is stranded)
        rows += int(res.stranded[s] > 0)
    print(kind, seed, "scenarios", n, "judged", len(judged), "stranding", int(np.sum(res.stranded > 0)), "stranded pods",
          int(res.stranded[res.stranded > 0].sum()), "rows checked in", rows)
    assert rows == sum(1 for s in judged if res.stranded[s] > 0)
    assert any(res.stranded[s] > 0 for s in judged) and any(res.stranded[s] == 0 and scen_off[s + 1] > scen_off[s] for s in judged)
    if kind == "inter_pod":
        assert (res.how == E.NOT_PLAIN).any()


def test_a_slice_and_unasked_optional_outputs(checker):
    """cand_pod_off[0] > 0 and lost_off[0] > 0: the outputs are relative to them; counts and how may be NULL."""
    b = E.Built(next(c for c in CASES if c.name == "lost_node_was_the_first_fit"))
    lib = capi.load_planner()
    h = b.sc.product_snapshot()
    try:
        whole = evacuate_plan_arrays(checker, h, b.sc.ptr, b.scen_off, b.scen_pods, b.lost_off, b.lost_pos)
        part = evacuate_plan_arrays(checker, h, b.sc.ptr, b.scen_off[1:].copy(), b.scen_pods, b.lost_off[1:].copy(), b.lost_pos)
        lo = int(b.scen_off[1])
        assert np.array_equal(part.node_of_pod, whole.node_of_pod[lo:]) and np.array_equal(part.counts, whole.counts[lo:])
        assert np.array_equal(part.stranded, whole.stranded[1:]) and np.array_equal(part.how, whole.how[1:])
        n, total = len(b.scen_off) - 1, len(b.scen_pods)
        stranded, first, mapping = np.full(n, 77, np.int32), np.full(n, 77, np.int32), np.full(total, 77, np.int32)
        o = capi.sr_evacuate_out(capi.ptr(stranded, capi.P32), capi.ptr(first, capi.P32), capi.ptr(mapping, capi.P32), None, None)
        scen = capi.sr_candidates(n, capi.ptr(b.scen_off, capi.P32), capi.ptr(b.scen_pods, capi.P32), None)
        assert lib.sr_evacuate_plan(checker.handle, h, b.sc.ptr, ctypes.byref(scen), capi.ptr(b.lost_off, capi.P32),
                                    capi.ptr(b.lost_pos, capi.P32), ctypes.byref(o)) == capi.SR_OK, checker.last_error()
        assert np.array_equal(stranded, whole.stranded) and np.array_equal(first, whole.first)
        assert np.array_equal(mapping, whole.node_of_pod)
    finally:
        lib.sr_snapshot_destroy(h)


def test_the_rule_s_clauses_beyond_the_hand_cases(checker):
    """A pod of unknown scalars on the lost node, and a negative accounted request: NOT_PLAIN through the C ABI."""
    from helpers import Scenario
    from known_answer import P
    from explain_plan_cases import pool
    from evacuate_ref import scenarios
    from test_evacuate_reference import unknown_scalars_input
    lib = capi.load_planner()
    sc, bare, args = unknown_scalars_input()
    h = ctypes.c_void_p()
    assert lib.sr_snapshot_create(ctypes.byref(bare), capi.ptr(sc.spot, capi.P32), len(sc.spot),
                                  capi.ptr(sc.node_pod_off, capi.P32), capi.ptr(sc.node_pod_idx, capi.P32),
                                  ctypes.byref(h)) == capi.SR_OK
    try:
        res = evacuate_plan_arrays(checker, h, sc.ptr, *args)
        assert list(res.how) == [E.NOT_PLAIN, E.JUDGED] and list(res.stranded) == [-1, 0]
        assert list(res.node_of_pod) == [-1, 0] and not res.counts.any()
    finally:
        lib.sr_snapshot_destroy(h)
    sc = Scenario(pool(3), [[], [], []], [P("a0", cpu=100), P("a1", cpu=100)])
    args = scenarios(sc, [[0], [0]], moved=[[sc.qidx(0), sc.qidx(1)], [sc.qidx(1)]])
    sc.enc.a["acc_cpu"][sc.qidx(0)] = -1
    h = sc.product_snapshot()
    try:
        res = evacuate_plan_arrays(checker, h, sc.ptr, *args)
        assert list(res.how) == [E.NOT_PLAIN, E.JUDGED] and list(res.node_of_pod) == [-1, -1, 1]
    finally:
        lib.sr_snapshot_destroy(h)


def test_no_scenarios_and_no_spot_nodes(checker):
    from helpers import Scenario
    from known_answer import P
    sc = Scenario([], [], [P("a0", cpu=10), P("a1", cpu=20)])
    pods = np.array([sc.qidx(0), sc.qidx(1)], np.int32)
    lib = capi.load_planner()
    h = sc.product_snapshot()
    try:
        none = evacuate_plan_arrays(checker, h, sc.ptr, np.zeros(1, np.int32), pods, np.zeros(1, np.int32), np.zeros(0, np.int32))
        assert len(none.stranded) == 0 and none.ranking() == []
        res = evacuate_plan_arrays(checker, h, sc.ptr, np.array([0, 2], np.int32), pods, np.zeros(2, np.int32),
                                   np.zeros(0, np.int32))
        assert list(res.how) == [E.JUDGED] and list(res.stranded) == [2] and list(res.first) == [0]
        assert list(res.node_of_pod) == [-1, -1] and not res.counts.any()
    finally:
        lib.sr_snapshot_destroy(h)


def test_ranking_and_mirror(checker):
    """rescheduler.evacuatePlan on Pod / Node objects with the scenarios evacuation_scenarios builds, and the ranking
    an operator reads."""
    from known_answer import N, P, used
    from spotplanner import nodes as NM
    from spotplanner.rescheduler import evacuatePlan, evacuation_scenarios
    nodes = [N("n%d" % i, cpu=1000, labels={"pool": "m5.a" if i < 2 else "c5.b"}) for i in range(4)]
    base = [[used(cpu=600, name="b0"), used(cpu=300, name="b0x")], [used(cpu=700, name="b1")], [used(cpu=200, name="b2")],
            [used(cpu=900, name="b3")]]
    infos = NM.NodeInfoArray(NM.NodeInfo(n, ps, 0, 0) for n, ps in zip(nodes, base))
    snapshot = infos.GetClusterSnapshot()
    try:
        names, lost = evacuation_scenarios(infos, pool_key="pool")
        assert names == ["node:n0", "node:n1", "node:n2", "node:n3", "pool:m5.a", "pool:c5.b"]
        assert lost == [[0], [1], [2], [3], [0, 1], [2, 3]]
        states = [snapshot.node_state(n.name) for n in nodes]
        res = evacuatePlan(checker, snapshot, infos, lost)
        assert [snapshot.node_state(n.name) for n in nodes] == states
        assert (res.how == E.JUDGED).all()
        # free: 100, 300, 800, 100.  n0: 600 -> n2, 300 -> n1.  n1: 700 -> n2.  n2: 200 -> n1.  n3: 900 nowhere.
        # m5.a: 600 -> n2, 300 nowhere (n2 has 200 left, n3 100), 700 nowhere.  c5.b: 200 -> n1, 900 nowhere.
        assert list(res.node_of_pod) == [2, 1, 2, 1, -1, 2, -1, -1, 1, -1]
        assert list(res.stranded) == [0, 0, 0, 1, 2, 1] and list(res.first) == [-1, -1, -1, 0, 1, 1]
        assert res.ranking() == [4, 3, 5] and res.stranded_pods(4) == [1, 2] and res.not_answered() == []
        cpu = capi.WHY_NAMES.index("CPU")
        assert res.counts[4][cpu] == 3 and res.counts[6][cpu] == 2 and res.counts[6].sum() == 2
        assert evacuatePlan(checker, snapshot, infos, lost, counts=False).counts is None
    finally:
        snapshot.close()


def test_argument_errors_leave_the_snapshot_alone(checker):
    b = E.Built(CASES[0])
    lib = capi.load_planner()
    h = b.sc.product_snapshot()
    try:
        before = _node_states(lib, h, b.n_spot)
        args = (b.scen_off, b.scen_pods, b.lost_off, b.lost_pos)
        good = evacuate_plan_arrays(checker, h, b.sc.ptr, *args)

        def refused(scen_off, scen_pods, lost_off, lost_pos):
            with pytest.raises(PlannerError) as e:
                evacuate_plan_arrays(checker, h, b.sc.ptr, scen_off, scen_pods, lost_off, lost_pos)
            assert e.value.status == capi.SR_ERR_INVALID_ARG
            assert _node_states(lib, h, b.n_spot) == before
        pods = b.scen_pods.copy()
        pods[1] = 10 ** 6
        refused(b.scen_off, pods, b.lost_off, b.lost_pos)
        for value in (-1, b.n_spot):
            pos = b.lost_pos.copy()
            pos[-1] = value
            refused(b.scen_off, b.scen_pods, b.lost_off, pos)
        s = next(i for i, sn in enumerate(b.case.scens) if len(sn.lost) >= 2)
        pos = b.lost_pos.copy()
        pos[b.lost_off[s] + 1] = pos[b.lost_off[s]]
        refused(b.scen_off, b.scen_pods, b.lost_off, pos)
        off = b.lost_off.copy()
        off[1], off[2] = off[2] + 1, off[1]
        refused(b.scen_off, b.scen_pods, off, b.lost_pos)
        # a valid call afterwards is what it was
        same_but_counts(evacuate_plan_arrays(checker, h, b.sc.ptr, *args), good)
        assert lib.sr_snapshot_fork(h) == capi.SR_OK
        with pytest.raises(PlannerError) as e:
            evacuate_plan_arrays(checker, h, b.sc.ptr, *args)
        assert e.value.status == capi.SR_ERR_STATE
        assert lib.sr_snapshot_revert(h) == capi.SR_OK
        assert _node_states(lib, h, b.n_spot) == before
    finally:
        lib.sr_snapshot_destroy(h)


def test_plans_around_a_call_are_identical():
    """The third plan of one input on a fresh context, with and without an sr_evacuate_plan call before it: statuses,
    mapping and the steady prepare's upload are the same."""
    sc, cand_off, cand_pods, _ = _steady_scenario()
    lib = capi.load_planner()
    n_spot = len(sc.spot)
    # the last four nodes lose their 950m pod each; the four lost together
    lost = [[j] for j in range(4, 8)] + [[4, 5, 6, 7]]
    from evacuate_ref import scenarios
    args = scenarios(sc, lost)
    seen = []
    for ask in (False, True):
        ck = make_checker()
        h = sc.product_snapshot()
        try:
            for _ in range(2):
                first = plan_arrays(ck, h, sc.ptr, cand_off, cand_pods)
            if ask:
                before = _node_states(lib, h, n_spot)
                res = evacuate_plan_arrays(ck, h, sc.ptr, *args)
                assert _node_states(lib, h, n_spot) == before
                assert list(res.how) == [E.JUDGED] * 5 and list(res.stranded) == [0, 0, 0, 0, 0]
                assert list(res.node_of_pod) == [0, 0, 0, 0, 0, 1, 2, 3]
            p = plan_arrays(ck, h, sc.ptr, cand_off, cand_pods)
            t = ck.timing()
            seen.append((list(p.status), list(p.node_of_pod), p.winner, list(p.winner_map), int(t.bytes_uploaded),
                         int(t.enc_reused), int(t.k0_columns)))
            assert list(first.status) == list(p.status) and list(first.node_of_pod) == list(p.node_of_pod)
        finally:
            lib.sr_snapshot_destroy(h)
            ck.close()
    print("third plan without / with an sr_evacuate_plan call before it:", seen)
    assert seen[0] == seen[1]
    assert seen[0][5] == 1  # a steady prepare: the candidate side was reused
