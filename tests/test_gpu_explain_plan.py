"""sr_explain_plan on the GPU: the hand cases of tests/explain_plan_cases.py
through the C ABI, random clusters planned by sr_plan against the
per-candidate loop (sr_explain_candidate) and the oracle, argument errors, and
planning around a call."""
import numpy as np
import pytest

import explain_plan_cases as C
from known_answer import N, P, used
from oracle_lib import load_oracle
from spotplanner import capi
from spotplanner.rescheduler import (PlannerError, explain_arrays, explain_candidate_arrays, explain_plan_arrays,
                                     plan_arrays)
from test_explain_plan_reference import RANDOM, RUN_IDS, RUNS, count_ways, random_input
from test_gpu_explain import _check_sums, _node_states, _steady_scenario
from test_gpu_k2_dispatch import make_checker

pytestmark = pytest.mark.gpu

CASES = C.cases()


def _same(res, c, one):
    """Candidate c of an explain_plan result equals a one-pod ExplainResult, field for field."""
    assert res.fallback[c] == one.fallback[0], c
    assert res.feasible[c] == one.feasible[0] and res.first[c] == one.first[0], (c, res.first[c], one.first[0])
    assert np.array_equal(res.counts[c], one.counts[0]), c
    assert np.array_equal(res.node_mask[c], one.node_mask[0]), c


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_hand_cases(checker, case):
    b = C.Built(case)
    lib = capi.load_planner()
    h = b.sc.product_snapshot()
    try:
        before = _node_states(lib, h, b.n_spot)
        res = explain_plan_arrays(checker, h, b.sc.ptr, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
        bare = explain_plan_arrays(checker, h, b.sc.ptr, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod,
                                   node_mask=False)
        assert _node_states(lib, h, b.n_spot) == before
        assert [int(x) for x in res.how] == [cd.how for cd in case.cands]
        assert bare.node_mask is None and np.array_equal(bare.how, res.how)
        assert np.array_equal(bare.counts, res.counts) and np.array_equal(bare.feasible, res.feasible)
        assert np.array_equal(bare.first, res.first) and np.array_equal(bare.fallback, res.fallback)
        for c, cd in enumerate(case.cands):
            assert res.fallback[c] == 0
            if cd.how == C.NONE:
                assert res.feasible[c] == -1 and res.first[c] == -1
                assert not res.counts[c].any() and not res.node_mask[c].any()
                continue
            _check_sums(res, c, case.expected(c))
            if cd.first is not None:
                assert res.first[c] == cd.first
            lo, hi = int(b.cand_off[c]), int(b.cand_off[c + 1])
            _same(res, c, explain_candidate_arrays(checker, h, b.sc.ptr, b.cand_pods[lo:hi], b.node_of_pod[lo:hi],
                                                   cd.at_pod))
    finally:
        lib.sr_snapshot_destroy(h)


@pytest.mark.parametrize("kind,seed", RUNS, ids=RUN_IDS)
def test_random_plans(checker, kind, seed):
    """Every stuck candidate of an sr_plan tick in one call: equal to the per-candidate loop and the
    oracle's yes / no, nothing feasible in context where the base snapshot often still shows nodes."""
    kw, floors = RANDOM[kind]
    sc, cand_off, cand_pods = random_input(seed, kw)
    n_spot, n = len(sc.spot), len(cand_off) - 1
    lib = capi.load_planner()
    osnap = sc.oracle_snapshot()
    h = sc.product_snapshot()
    try:
        plan = plan_arrays(checker, h, sc.ptr, cand_off, cand_pods)
        before = _node_states(lib, h, n_spot)
        at_pod, mapping = np.array(plan.status, np.int32), np.array(plan.node_of_pod, np.int32)
        res = explain_plan_arrays(checker, h, sc.ptr, cand_off, cand_pods, at_pod, mapping)
        assert _node_states(lib, h, n_spot) == before
        bare = explain_plan_arrays(checker, h, sc.ptr, cand_off, cand_pods, at_pod, mapping, node_mask=False)
        assert np.array_equal(bare.counts, res.counts) and np.array_equal(bare.feasible, res.feasible)
        assert np.array_equal(bare.first, res.first) and np.array_equal(bare.how, res.how)
        failing = [c for c in range(n) if at_pod[c] >= 0]
        stop_pods = np.array([cand_pods[cand_off[c] + at_pod[c]] for c in failing], np.int32)
        base = explain_arrays(checker, h, sc.ptr, stop_pods, node_mask=False)
        looks_feasible = want_feasible = 0
        ora = load_oracle()
        for i, c in enumerate(failing):
            lo, hi = int(cand_off[c]), int(cand_off[c + 1])
            assert res.how[c] in (C.BATCHED, C.SINGLE)
            _same(res, c, explain_candidate_arrays(checker, h, sc.ptr, cand_pods[lo:hi], mapping[lo:hi],
                                                   int(at_pod[c])))
            assert res.fallback[c] == 0  # (sr_plan planned the candidate)
            assert res.feasible[c] == 0 and res.first[c] == -1 and (res.node_mask[c] != 0).all(), c
            fits, bits = C.oracle_in_context(sc, osnap, cand_pods[lo:hi], mapping[lo:hi], int(at_pod[c]), n_spot)
            assert [int(m == 0) for m in res.node_mask[c]] == fits, c
            assert [int(m) & C.RESOURCE_BITS for m in res.node_mask[c]] == bits, c
            # against the base snapshot the same pod often still shows nodes: the oracle says where
            if not base.fallback[i]:
                looks_feasible += int(base.feasible[i] > 0)
                want_feasible += int(any(ora.oracle_check_predicates(osnap.h, sc.ptr, int(stop_pods[i]), j)
                                         for j in range(n_spot)))
        for c in range(n):
            if at_pod[c] < 0:
                assert res.how[c] == C.NONE and res.feasible[c] == -1 and not res.node_mask[c].any()
        assert _node_states(lib, h, n_spot) == before
        ways = count_ways(res.how, at_pod, res.fallback)
        print(kind, seed, "failing", len(failing), "at k > 0: batched, single", ways,
              "feasible against the base snapshot", looks_feasible)
        assert ways[0] >= floors[0] and ways[1] >= floors[1], ways
        # the fact this entry point exists for, on every seed; and exactly where the oracle says
        assert looks_feasible >= 1
        assert looks_feasible == want_feasible
        # drained candidates asked at their last pod: the plan's node for it
        last = np.array([cand_off[c + 1] - cand_off[c] - 1 if plan.status[c] == capi.SR_CAND_OK else -1
                         for c in range(n)], np.int32)
        drained = [c for c in range(n) if last[c] >= 0]
        res = explain_plan_arrays(checker, h, sc.ptr, cand_off, cand_pods, last, mapping)
        for c in drained:
            assert res.fallback[c] == 0 and res.first[c] == mapping[cand_off[c] + last[c]], c
            fits, _ = C.oracle_in_context(sc, osnap, cand_pods[cand_off[c]:cand_off[c + 1]],
                                          mapping[cand_off[c]:cand_off[c + 1]], int(last[c]), n_spot)
            assert [int(m == 0) for m in res.node_mask[c]] == fits, c
        assert len(drained) >= 1 and _node_states(lib, h, n_spot) == before
    finally:
        lib.sr_snapshot_destroy(h)


def test_the_base_snapshot_answer_is_wrong_in_context(checker):
    """A planned tick whose stuck candidate stops at its fifth pod: sr_explain_pods still shows the four open
    nodes for that pod, sr_explain_plan none -- the earlier four pods of the candidate took them."""
    sc, cand_off, cand_pods, _ = _steady_scenario()
    lib = capi.load_planner()
    h = sc.product_snapshot()
    try:
        plan = plan_arrays(checker, h, sc.ptr, cand_off, cand_pods)
        assert list(plan.status) == [capi.SR_CAND_OK, capi.SR_CAND_OK, 4]
        stop = cand_pods[cand_off[2] + 4: cand_off[2] + 5]
        base = explain_arrays(checker, h, sc.ptr, stop)
        assert base.feasible[0] == 4 and base.first[0] == 0
        res = explain_plan_arrays(checker, h, sc.ptr, cand_off, cand_pods, plan.status, plan.node_of_pod)
        assert list(res.how) == [C.NONE, C.NONE, C.BATCHED]
        assert res.feasible[2] == 0 and res.first[2] == -1
        _check_sums(res, 2, [C.CPU] * 8)
    finally:
        lib.sr_snapshot_destroy(h)


def test_port_bits_exhausted(checker):
    """A batch whose stop pods ask for more distinct host ports than one encode's state word holds: the pods
    past the 64th come back from the batched encode as fallback, are asked again alone and are inside the
    encoded set there; a PVC pod is outside it whichever way it went."""
    case = C.port_bits_case()
    b = C.Built(case)
    lib = capi.load_planner()
    h = b.sc.product_snapshot()
    try:
        before = _node_states(lib, h, b.n_spot)
        res = explain_plan_arrays(checker, h, b.sc.ptr, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
        assert _node_states(lib, h, b.n_spot) == before
        assert [int(x) for x in res.how] == [cd.how for cd in case.cands]
        pvc = C.N_PORT_PODS
        assert [int(x) for x in res.fallback] == [int(c == pvc) for c in range(len(case.cands))]
        for c, cd in enumerate(case.cands):
            lo, hi = int(b.cand_off[c]), int(b.cand_off[c + 1])
            _same(res, c, explain_candidate_arrays(checker, h, b.sc.ptr, b.cand_pods[lo:hi], b.node_of_pod[lo:hi],
                                                   cd.at_pod))
            if c == pvc:
                assert res.feasible[c] == -1 and res.first[c] == -1 and not res.node_mask[c].any()
            else:
                _check_sums(res, c, case.expected(c))
        # without the map: no asked candidate has an earlier pod, and the re-asked ones still go through
        off, pods, at, _ = C.sliced(b, 0)
        at[-1] = -1
        lone = explain_plan_arrays(checker, h, b.sc.ptr, off, pods, at, None)
        assert np.array_equal(lone.how[:-1], res.how[:-1]) and np.array_equal(lone.node_mask[:-1], res.node_mask[:-1])
        # alone in its batch the PVC pod stays BATCHED, fallback all the same
        off, pods, at, m = C.sliced(b, pvc)
        at[1:] = -1
        one = explain_plan_arrays(checker, h, b.sc.ptr, off, pods, at, m)
        assert list(one.how) == [C.BATCHED, C.NONE] and list(one.fallback) == [1, 0] and one.feasible[0] == -1
    finally:
        lib.sr_snapshot_destroy(h)


@pytest.mark.parametrize("name,first", [("cpu_last_milli", 1), ("two_pods_merge_on_one_node", 2),
                                        ("hostname_anti_affinity_both_ways", 1), ("seventy_earlier_pods", 1)])
def test_a_slice_of_a_larger_candidate_list(checker, name, first):
    """cand_pod_off[0] > 0: node_of_pod is read relative to it, on the batched and on the single path."""
    case = next(c for c in CASES if c.name == name)
    b = C.Built(case)
    off, pods, at, m = C.sliced(b, first)
    assert off[0] > 0
    lib = capi.load_planner()
    h = b.sc.product_snapshot()
    try:
        res = explain_plan_arrays(checker, h, b.sc.ptr, off, pods, at, m)
        whole = explain_plan_arrays(checker, h, b.sc.ptr, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
    finally:
        lib.sr_snapshot_destroy(h)
    for i, c in enumerate(range(first, len(case.cands))):
        assert res.how[i] == case.cands[c].how == whole.how[c]
        _check_sums(res, i, case.expected(c))
        assert np.array_equal(res.node_mask[i], whole.node_mask[c]) and res.first[i] == whole.first[c]


def test_explain_plan_mirror(checker):
    """rescheduler.explainPlan on Pod / Node objects: a plan over a ClusterSnapshot explained in one call, equal
    to explainCandidate for every stuck candidate."""
    from spotplanner import nodes as NM
    from spotplanner.rescheduler import explainCandidate, explainPlan
    nodes = [N("n%d" % i, cpu=1000) for i in range(8)]
    base = [[] for _ in range(4)] + [[used(cpu=950, name="b%d" % i)] for i in range(4)]
    cands = [[P("c0-0", cpu=600)], [P("c1-%d" % k, cpu=600) for k in range(5)], [],
             [P("c3-0", cpu=300), P("c3-1", cpu=300), P("c3-2", cpu=300), P("c3-3", cpu=1001)]]
    infos = NM.NodeInfoArray(NM.NodeInfo(n, ps, 0, 0) for n, ps in zip(nodes, base))
    snapshot = infos.GetClusterSnapshot()
    try:
        flat = [p for c in cands for p in c]
        enc = snapshot.encode_pods(flat)
        cand_off = np.zeros(len(cands) + 1, np.int32)
        cand_off[1:] = np.cumsum([len(c) for c in cands])
        plan = plan_arrays(checker, snapshot.handle, enc.ptr, cand_off, np.arange(len(flat), dtype=np.int32))
        assert list(plan.status) == [capi.SR_CAND_OK, 4, capi.SR_CAND_EMPTY, 3]
        states = [snapshot.node_state(n.name) for n in nodes]
        res = explainPlan(checker, snapshot, infos, cands, plan)
        assert [snapshot.node_state(n.name) for n in nodes] == states
        assert list(res.how) == [C.NONE, C.BATCHED, C.NONE, C.BATCHED]
        _check_sums(res, 1, [C.CPU] * 8)
        _check_sums(res, 3, [C.CPU] * 8)
        assert res.summary(1) == "0/8 nodes are available: 8 CPU."
        for c in (1, 3):
            k = int(plan.status[c])
            names = [nodes[int(j)].name for j in plan.node_of_pod[cand_off[c]:cand_off[c] + k]]
            _same(res, c, explainCandidate(checker, snapshot, infos, cands[c], names + [""] * (len(cands[c]) - k), k))
    finally:
        snapshot.close()


def test_argument_errors_leave_the_snapshot_alone(checker):
    b = C.Built(CASES[0])  # cpu_last_milli: candidates of 2, 2, 2 and 1 pods
    lib = capi.load_planner()
    h = b.sc.product_snapshot()
    try:
        before = _node_states(lib, h, b.n_spot)

        def call(at_pod=b.at_pod, mapping=b.node_of_pod):
            return explain_plan_arrays(checker, h, b.sc.ptr, b.cand_off, b.cand_pods, np.array(at_pod, np.int32),
                                       np.array(mapping, np.int32))
        m = b.node_of_pod
        for kw in (dict(at_pod=[1, 1, 2, 0]), dict(at_pod=[1, 1, 1, 1]), dict(mapping=[-1] + list(m[1:])),
                   dict(mapping=[b.n_spot] + list(m[1:])), dict(mapping=list(m[:4]) + [b.n_spot] + list(m[5:]))):
            with pytest.raises(PlannerError) as e:
                call(**kw)
            assert e.value.status == capi.SR_ERR_INVALID_ARG, kw
            assert _node_states(lib, h, b.n_spot) == before
        assert [int(x) for x in call().how] == [cd.how for cd in CASES[0].cands]
        assert lib.sr_snapshot_fork(h) == capi.SR_OK
        with pytest.raises(PlannerError) as e:
            call()
        assert e.value.status == capi.SR_ERR_STATE
        assert lib.sr_snapshot_revert(h) == capi.SR_OK
        assert _node_states(lib, h, b.n_spot) == before
    finally:
        lib.sr_snapshot_destroy(h)


def test_plans_around_a_call_are_identical():
    """The third plan of one input on a fresh context, with and without an sr_explain_plan call before it:
    statuses, mapping and the steady prepare's upload are the same."""
    sc, cand_off, cand_pods, _ = _steady_scenario()
    lib = capi.load_planner()
    seen = []
    for explain in (False, True):
        ck = make_checker()
        h = sc.product_snapshot()
        try:
            for _ in range(2):
                first = plan_arrays(ck, h, sc.ptr, cand_off, cand_pods)
            if explain:
                res = explain_plan_arrays(ck, h, sc.ptr, cand_off, cand_pods, first.status, first.node_of_pod)
                # the five 600m pods of the last candidate meet four open nodes: it stops at its fifth pod
                assert list(first.status) == [capi.SR_CAND_OK, capi.SR_CAND_OK, 4]
                assert list(res.how) == [C.NONE, C.NONE, C.BATCHED]
                _check_sums(res, 2, [C.CPU] * 8)
            p = plan_arrays(ck, h, sc.ptr, cand_off, cand_pods)
            t = ck.timing()
            seen.append((list(p.status), list(p.node_of_pod), p.winner, list(p.winner_map), int(t.bytes_uploaded),
                         int(t.enc_reused), int(t.k0_columns)))
            assert list(first.status) == list(p.status) and list(first.node_of_pod) == list(p.node_of_pod)
        finally:
            lib.sr_snapshot_destroy(h)
            ck.close()
    print("third plan without / with an sr_explain_plan call before it:", seen)
    assert seen[0] == seen[1]
    assert seen[0][5] == 1  # a steady prepare: the candidate side was reused
