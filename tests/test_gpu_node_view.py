"""sr_node_view_pods / sr_node_view_plan on the GPU: the hand cases of tests/node_view_sizes.py through the C ABI,
random clusters against node_view_ref.fold of the sibling calls' per-query arrays from the same context (whose
masks and shortfalls test_gpu_shortfall.py holds against the oracle), out_how and the untouched snapshot, the
Pod / Node layer, alternating calls on one context, planning around the calls, and the argument errors."""
import ctypes

import numpy as np
import pytest

import explain_plan_cases as C
import node_view_ref as V
import node_view_sizes as NS
from oracle_lib import oracle_plan
from spotplanner import capi
from spotplanner.rescheduler import (explain_plan_arrays, node_view_arrays, node_view_plan_arrays, plan_arrays,
                                     shortfall_arrays, shortfall_plan_arrays)
from test_gpu_explain import _node_states, _steady_scenario
from test_gpu_k2_dispatch import make_checker
from test_gpu_shortfall import snapshot
from test_shortfall_reference import RUN_IDS, RUNS, random_reference

pytestmark = pytest.mark.gpu

CASES = NS.cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_hand_cases(checker, case):
    b = C.Built(case.plan)
    want = case.expanded()
    lib = capi.load_planner()
    with snapshot(b.sc) as h:
        before = _node_states(lib, h, b.n_spot)
        res = node_view_plan_arrays(checker, h, b.sc.ptr, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
        assert _node_states(lib, h, b.n_spot) == before
        V.same(V.as_dict(res), want, case.name)
        assert [int(x) for x in res.how] == [cd.how for cd in case.plan.cands]
        assert [int(x) for x in res.fallback] == case.expected_fallback()
        if case.as_pods:
            res = node_view_arrays(checker, h, b.sc.ptr, b.cand_pods)
            V.same(V.as_dict(res), want, case.name)
            assert not res.fallback.any()


def test_no_pods_at_all(checker):
    b = C.Built(NS.hand_tick().plan)
    with snapshot(b.sc) as h:
        res = node_view_arrays(checker, h, b.sc.ptr, np.zeros(0, np.int32))
    assert res.judged == 0 and not res.admits.any() and not res.refuses.any() and (res.sole_at == -1).all()


@pytest.mark.parametrize("kind,seed", RUNS, ids=RUN_IDS)
def test_random_clusters(checker, kind, seed):
    ref, cand_off, cand_pods = random_reference(kind, seed)
    with snapshot(ref.sc) as h:
        why, short = shortfall_arrays(checker, h, ref.sc.ptr, cand_pods)
        res = node_view_arrays(checker, h, ref.sc.ptr, cand_pods)
    want = V.fold_pods(why, short, ref.n_spot)
    V.same(V.as_dict(res), want, (kind, seed))
    assert np.array_equal(res.fallback, why.fallback) and want["judged"] >= 1


@pytest.mark.parametrize("kind,seed", RUNS, ids=RUN_IDS)
def test_random_plans(checker, kind, seed):
    """The oracle's plan: every stuck candidate, batched or one at a time, folded per node equals the fold of
    sr_shortfall_plan's per-candidate arrays; out_how is its; the snapshot is as it was."""
    ref, cand_off, cand_pods = random_reference(kind, seed)
    sc, n_spot = ref.sc, ref.n_spot
    lib = capi.load_planner()
    plan = oracle_plan(ref.osnap, sc.ptr, cand_off, cand_pods, mode=1)
    at_pod = np.ascontiguousarray(plan["status"], np.int32)
    mapping = np.ascontiguousarray(plan["node_of_pod"], np.int32)
    with snapshot(sc) as h:
        before = _node_states(lib, h, n_spot)
        why, short = shortfall_plan_arrays(checker, h, sc.ptr, cand_off, cand_pods, at_pod, mapping)
        res = node_view_plan_arrays(checker, h, sc.ptr, cand_off, cand_pods, at_pod, mapping)
        assert _node_states(lib, h, n_spot) == before
    want = V.fold_plan(why, short, at_pod, n_spot)
    V.same(V.as_dict(res), want, (kind, seed))
    assert np.array_equal(res.how, why.how) and np.array_equal(res.fallback, why.fallback)
    ways = [int((why.how == C.BATCHED).sum()), int((why.how == C.SINGLE).sum())]
    print(kind, seed, "judged", want["judged"], "batched, single:", ways)
    assert want["judged"] >= 1


def test_pod_and_node_layer(checker):
    """rescheduler.nodeViewPods / nodeViewPlan on Pod / Node objects against the array functions."""
    from known_answer import N, P, used
    from spotplanner import nodes as NM
    from spotplanner.rescheduler import nodeViewPlan, nodeViewPods
    nodes = [N("n%d" % i, cpu=1000) for i in range(8)]
    base = [[] for _ in range(4)] + [[used(cpu=950, name="b%d" % i)] for i in range(4)]
    cands = [[P("c0-0", cpu=600)], [P("c1-%d" % k, cpu=600) for k in range(5)], [],
             [P("c3-0", cpu=300), P("c3-1", cpu=300), P("c3-2", cpu=300), P("c3-3", cpu=1001)]]
    infos = NM.NodeInfoArray(NM.NodeInfo(n, ps, 0, 0) for n, ps in zip(nodes, base))
    snap = infos.GetClusterSnapshot()
    try:
        flat = [p for c in cands for p in c]
        enc = snap.encode_pods(flat)
        cand_off = np.zeros(len(cands) + 1, np.int32)
        cand_off[1:] = np.cumsum([len(c) for c in cands])
        idx = np.arange(len(flat), dtype=np.int32)
        plan = plan_arrays(checker, snap.handle, enc.ptr, cand_off, idx)
        assert list(plan.status) == [capi.SR_CAND_OK, 4, capi.SR_CAND_EMPTY, 3]
        states = [snap.node_state(n.name) for n in nodes]
        res = nodeViewPlan(checker, snap, infos, cands, plan)
        arr = node_view_plan_arrays(checker, snap.handle, enc.ptr, cand_off, idx, plan.status, plan.node_of_pod)
        assert [snap.node_state(n.name) for n in nodes] == states
        V.same(V.as_dict(res), V.as_dict(arr))
        assert list(res.how) == [C.NONE, C.BATCHED, C.NONE, C.BATCHED] and res.judged == 2
        # candidate 1: every open node 200m short after its four pods, the closed ones 550m; candidate 3: 1001m
        # after three 300m pods on node 0: 901m short there, 1m on the open nodes 1 .. 3, 951m on the closed ones
        assert res.sole_reasons(0) == {"CPU": 2} and res.closest(0) == {"CPU": (200, 1)}
        assert res.closest(1) == {"CPU": (1, 3)} and res.closest(4) == {"CPU": (550, 1)}
        assert not res.admits.any() and list(res.near) == [2] * 8
        pr = nodeViewPods(checker, snap, infos, flat)
        pa = node_view_arrays(checker, snap.handle, enc.ptr, idx)
        V.same(V.as_dict(pr), V.as_dict(pa))
        # against the snapshot as it is: the open nodes take every pod but the 1001m one, which is 1m short (slot 9)
        assert pr.judged == len(flat) and pr.admits[0] == len(flat) - 1 and pr.closest(0) == {"CPU": (1, 9)}
        assert pr.closest(4) == {"CPU": (250, 6)} and pr.sole_reasons(4) == {"CPU": len(flat)}
    finally:
        snap.close()


def test_one_context_alternating_calls():
    """Plan, explain, shortfall and node-view calls in turn on one context: every round gives what the first
    gave, and the node view is the fold of the shortfall call beside it."""
    sc, cand_off, cand_pods, _ = _steady_scenario()
    ck = make_checker()
    h = sc.product_snapshot()
    try:
        rounds = []
        for _ in range(3):
            plan = plan_arrays(ck, h, sc.ptr, cand_off, cand_pods)
            v1 = node_view_arrays(ck, h, sc.ptr, cand_pods)
            w1, s1 = shortfall_arrays(ck, h, sc.ptr, cand_pods)
            v2 = node_view_plan_arrays(ck, h, sc.ptr, cand_off, cand_pods, plan.status, plan.node_of_pod)
            e2 = explain_plan_arrays(ck, h, sc.ptr, cand_off, cand_pods, plan.status, plan.node_of_pod)
            w2, s2 = shortfall_plan_arrays(ck, h, sc.ptr, cand_off, cand_pods, plan.status, plan.node_of_pod)
            V.same(V.as_dict(v1), V.fold_pods(w1, s1, 8))
            V.same(V.as_dict(v2), V.fold_plan(w2, s2, plan.status, 8))
            assert np.array_equal(e2.node_mask, w2.node_mask) and np.array_equal(v2.how, e2.how)
            rounds.append((list(plan.status), list(plan.node_of_pod), V.as_dict(v1), V.as_dict(v2)))
        assert rounds[1] == rounds[0] and rounds[2] == rounds[0]
        # the one stuck candidate (five 600m pods): the open nodes 200m short after its four pods, the closed 550m
        assert rounds[0][3]["judged"] == 1 and rounds[0][3]["sole_min"][0] == [200, 0, 0, 0]
        assert rounds[0][3]["sole_min"][4] == [550, 0, 0, 0] and rounds[0][3]["sole_at"][4] == [2, -1, -1, -1]
    finally:
        capi.load_planner().sr_snapshot_destroy(h)
        ck.close()


def test_plans_around_the_calls_are_identical():
    """The third plan of one input on a fresh context, with and without node-view calls before it: statuses,
    mapping and the steady prepare's upload are the same."""
    sc, cand_off, cand_pods, _ = _steady_scenario()
    lib = capi.load_planner()
    seen = []
    for ask in (False, True):
        ck = make_checker()
        h = sc.product_snapshot()
        try:
            for _ in range(2):
                first = plan_arrays(ck, h, sc.ptr, cand_off, cand_pods)
            if ask:
                res = node_view_plan_arrays(ck, h, sc.ptr, cand_off, cand_pods, first.status, first.node_of_pod)
                assert list(res.how) == [C.NONE, C.NONE, C.BATCHED] and res.judged == 1
                assert res.closest(0) == {"CPU": (200, 2)} and res.closest(7) == {"CPU": (550, 2)}
                r2 = node_view_arrays(ck, h, sc.ptr, cand_pods)
                assert r2.judged == len(cand_pods) and r2.admits[0] == len(cand_pods) and r2.closest(4) == {"CPU": (550, 0)}
            p = plan_arrays(ck, h, sc.ptr, cand_off, cand_pods)
            t = ck.timing()
            seen.append((list(p.status), list(p.node_of_pod), p.winner, list(p.winner_map), int(t.bytes_uploaded),
                         int(t.enc_reused), int(t.k0_columns)))
            assert list(first.status) == list(p.status) and list(first.node_of_pod) == list(p.node_of_pod)
        finally:
            lib.sr_snapshot_destroy(h)
            ck.close()
    print("third plan without / with node-view calls before it:", seen)
    assert seen[0] == seen[1]
    assert seen[0][5] == 1  # a steady prepare: the candidate side was reused


def _raw_out(n_spot, **missing):
    def i32(k):  # (the struct keeps the arrays its pointers came from: capi._KeepsArrays)
        return capi.ptr(np.zeros(k * max(n_spot, 1), np.int32), capi.P32)
    o = capi.sr_node_view_out(i32(1), i32(1), i32(1), i32(capi.SR_WHY_COUNT), i32(capi.SR_WHY_COUNT),
                              capi.ptr(np.zeros(4 * max(n_spot, 1), np.int64), capi.P64), i32(4), None)
    for k in missing:
        setattr(o, k, None)
    return o


def test_null_required_arrays(checker):
    b = C.Built(NS.hand_tick().plan)
    lib = capi.load_planner()
    cands = capi.sr_candidates(1, capi.ptr(b.cand_off, capi.P32), capi.ptr(b.cand_pods, capi.P32), None)
    with snapshot(b.sc) as h:
        before = _node_states(lib, h, b.n_spot)
        for missing in ("judged", "admits", "near", "refuses", "sole", "sole_min", "sole_at"):
            o = _raw_out(b.n_spot, **{missing: True})
            assert lib.sr_node_view_pods(checker.handle, h, b.sc.ptr, capi.ptr(b.cand_pods, capi.P32), 1,
                                         ctypes.byref(o)) == capi.SR_ERR_INVALID_ARG, missing
            assert lib.sr_node_view_plan(checker.handle, h, b.sc.ptr, ctypes.byref(cands), capi.ptr(b.at_pod, capi.P32),
                                         capi.ptr(b.node_of_pod, capi.P32), ctypes.byref(o),
                                         None) == capi.SR_ERR_INVALID_ARG, missing
        assert _node_states(lib, h, b.n_spot) == before
        # fallback and out_how are optional
        res = node_view_plan_arrays(checker, h, b.sc.ptr, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
        o = _raw_out(b.n_spot)
        assert lib.sr_node_view_plan(checker.handle, h, b.sc.ptr, ctypes.byref(cands), capi.ptr(b.at_pod, capi.P32),
                                     capi.ptr(b.node_of_pod, capi.P32), ctypes.byref(o), None) == capi.SR_OK
        assert o.judged[0] == 1 and [o.sole_min[4 * j] for j in range(4)] == [200] * 4 and res.judged == 1


def test_forked_snapshot_is_refused_and_untouched(checker):
    b = C.Built(NS.hand_tick().plan)
    lib = capi.load_planner()
    with snapshot(b.sc) as h:
        assert lib.sr_snapshot_fork(h) == capi.SR_OK
        assert lib.sr_snapshot_add_pod(h, b.sc.ptr, int(b.cand_pods[0]), 1) == capi.SR_OK
        before = _node_states(lib, h, b.n_spot)
        with pytest.raises(Exception) as e:
            node_view_plan_arrays(checker, h, b.sc.ptr, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
        assert e.value.status == capi.SR_ERR_STATE
        assert _node_states(lib, h, b.n_spot) == before
        assert lib.sr_snapshot_revert(h) == capi.SR_OK
        res = node_view_plan_arrays(checker, h, b.sc.ptr, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
        V.same(V.as_dict(res), NS.hand_tick().expanded())
