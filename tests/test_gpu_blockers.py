"""sr_blockers_plan on the GPU: the hand cases of tests/blockers_cases.py through the C ABI, random clusters
planned by sr_plan against the contract's loop over the oracle (tests/blockers_ref.py) and, blocker by
blocker, against sr_explain_candidate on the compacted list; what is not asked, optional outputs, argument
errors, and planning around a call."""
import ctypes

import numpy as np
import pytest

import blockers_cases as B
from blockers_ref import compacted, oracle_blockers_plan
from spotplanner import capi
from spotplanner.rescheduler import (PlannerError, blockers_plan_arrays, explain_candidate_arrays, explain_plan_arrays,
                                     plan_arrays)
from test_blockers_reference import RUN_IDS, RUNS, stops_later
from test_explain_plan_reference import RANDOM, random_input
from test_gpu_explain import _node_states, _steady_scenario
from test_gpu_k2_dispatch import make_checker

pytestmark = pytest.mark.gpu

CASES = B.cases()


def same_but_counts(a, b):
    for f in ("blockers", "first", "node_of_pod", "fallback", "how"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def check_rows(checker, h, sc, cand_off, cand_pods, res, c):
    """Every blocker's counts row of candidate c is sr_explain_candidate's for the compacted list; every other
    row is zero."""
    base = int(cand_off[0])
    lo, hi = int(cand_off[c]), int(cand_off[c + 1])
    row = res.node_of_pod[lo - base:hi - base]
    for k in range(hi - lo):
        if row[k] >= 0 or res.blockers[c] < 0:
            assert not res.counts[lo - base + k].any(), (c, k)
            continue
        pods, mapping, at = compacted(cand_pods[lo:hi], row, k)
        one = explain_candidate_arrays(checker, h, sc.ptr, np.array(pods, np.int32), np.array(mapping, np.int32), at,
                                       node_mask=False)
        assert one.fallback[0] == 0 and one.feasible[0] == 0 and one.first[0] == -1, (c, k)
        assert np.array_equal(res.counts[lo - base + k], one.counts[0]), (c, k)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_hand_cases(checker, case):
    b = B.Built(case)
    lib = capi.load_planner()
    h = b.sc.product_snapshot()
    try:
        before = _node_states(lib, h, b.n_spot)
        res = blockers_plan_arrays(checker, h, b.sc.ptr, b.cand_off, b.cand_pods, b.ask)
        bare = blockers_plan_arrays(checker, h, b.sc.ptr, b.cand_off, b.cand_pods, b.ask, counts=False)
        assert _node_states(lib, h, b.n_spot) == before
        assert list(res.how) == list(b.how)
        assert list(res.node_of_pod) == list(b.node_of_pod)
        assert list(res.blockers) == list(b.blockers) and list(res.first) == list(b.first)
        assert list(res.fallback) == list(b.fallback)
        assert bare.counts is None
        same_but_counts(res, bare)
        for i, row in b.pinned.items():
            assert list(res.counts[i]) == row, i
        for c in range(len(case.cands)):
            check_rows(checker, h, b.sc, b.cand_off, b.cand_pods, res, c)
        assert _node_states(lib, h, b.n_spot) == before
    finally:
        lib.sr_snapshot_destroy(h)


@pytest.mark.parametrize("kind,seed", RUNS, ids=RUN_IDS)
def test_random_plans(checker, kind, seed):
    """sr_plan, then sr_blockers_plan(ask = status): the first blocker is the plan's stop pod, the pods before it
    are where the plan put them, the whole mapping is the oracle loop's and every blocker's row is
    sr_explain_candidate's on the compacted list."""
    sc, cand_off, cand_pods = random_input(seed, RANDOM[kind][0])
    n_spot, n = len(sc.spot), len(cand_off) - 1
    lib = capi.load_planner()
    osnap = sc.oracle_snapshot()
    h = sc.product_snapshot()
    try:
        plan = plan_arrays(checker, h, sc.ptr, cand_off, cand_pods)
        status, mapping = np.array(plan.status, np.int32), np.array(plan.node_of_pod, np.int32)
        before = _node_states(lib, h, n_spot)
        res = blockers_plan_arrays(checker, h, sc.ptr, cand_off, cand_pods, status)
        assert _node_states(lib, h, n_spot) == before
        same_but_counts(res, blockers_plan_arrays(checker, h, sc.ptr, cand_off, cand_pods, status, counts=False))
        ref = oracle_blockers_plan(sc, osnap, cand_off, cand_pods, status, n_spot)
        assert np.array_equal(res.node_of_pod, ref["node_of_pod"])
        assert np.array_equal(res.blockers, ref["blockers"]) and np.array_equal(res.first, ref["first"])
        assert not res.fallback.any()  # (sr_plan planned every asked candidate)
        for c in range(n):
            lo, hi = int(cand_off[c]), int(cand_off[c + 1])
            if status[c] < 0:  # not asked
                assert res.how[c] == B.NONE and res.blockers[c] == -1 and res.first[c] == -1
                assert (res.node_of_pod[lo:hi] == -1).all() and not res.counts[lo:hi].any()
                continue
            assert res.how[c] in (B.BATCHED, B.SINGLE)
            assert res.first[c] == status[c] and res.blockers[c] >= 1
            assert np.array_equal(res.node_of_pod[lo:lo + status[c]], mapping[lo:lo + status[c]])
            check_rows(checker, h, sc, cand_off, cand_pods, res, c)
        later = stops_later(status)
        ways = (sum(1 for c in later if res.how[c] == B.BATCHED), sum(1 for c in later if res.how[c] == B.SINGLE))
        print(kind, seed, "stuck", int(np.sum(status >= 0)), "at k > 0: batched, single", ways, "blockers",
              sorted(int(x) for x in res.blockers[res.blockers > 0]))
        assert ways[0] >= 1 and ways[1] >= 1 and (res.blockers >= 2).any()
        # the first blocker's row is what sr_explain_plan says about the stop pod
        why = explain_plan_arrays(checker, h, sc.ptr, cand_off, cand_pods, status, mapping, node_mask=False)
        for c in range(n):
            if status[c] >= 0:
                assert np.array_equal(res.counts[int(cand_off[c]) + status[c]], why.counts[c]), c
        # asked for the candidates the plan drained: no blocker, the plan's mapping
        ok = np.where(status == capi.SR_CAND_OK, 0, -1).astype(np.int32)
        drained = blockers_plan_arrays(checker, h, sc.ptr, cand_off, cand_pods, ok)
        assert (ok == 0).any()
        for c in range(n):
            lo, hi = int(cand_off[c]), int(cand_off[c + 1])
            if ok[c] == 0:
                assert drained.blockers[c] == 0 and drained.first[c] == -1 and drained.fallback[c] == 0
                assert np.array_equal(drained.node_of_pod[lo:hi], mapping[lo:hi])
                assert not drained.counts[lo:hi].any()
            else:
                assert drained.how[c] == B.NONE and drained.blockers[c] == -1
        assert _node_states(lib, h, n_spot) == before
    finally:
        lib.sr_snapshot_destroy(h)


def test_a_slice_of_a_larger_candidate_list(checker):
    """cand_pod_off[0] > 0: node_of_pod and counts are relative to it, on both ways."""
    for name in ("blocker_first_middle_last", "two_port_pods"):
        case = next(c for c in CASES if c.name == name)
        b = B.Built(case)
        lo = int(b.cand_off[1])
        lib = capi.load_planner()
        h = b.sc.product_snapshot()
        try:
            res = blockers_plan_arrays(checker, h, b.sc.ptr, b.cand_off[1:].copy(), b.cand_pods, b.ask[1:].copy())
            whole = blockers_plan_arrays(checker, h, b.sc.ptr, b.cand_off, b.cand_pods, b.ask)
        finally:
            lib.sr_snapshot_destroy(h)
        assert np.array_equal(res.node_of_pod, whole.node_of_pod[lo:]) and np.array_equal(res.counts, whole.counts[lo:])
        assert np.array_equal(res.blockers, whole.blockers[1:]) and np.array_equal(res.how, whole.how[1:])
        assert list(res.node_of_pod) == list(b.node_of_pod[lo:])


def test_no_spot_nodes(checker):
    """The pinned edge: without spot nodes every pod of an asked candidate is a blocker with a zero row, as
    sr_explain_plan reports feasible 0, first -1 and zero counts there."""
    from helpers import Scenario
    from known_answer import P
    flat = [P("a0", cpu=10), P("a1", cpu=20), P("b0", cpu=10)]
    sc = Scenario([], [], flat)
    cand_off = np.array([0, 2, 3], np.int32)
    cand_pods = np.array([sc.qidx(i) for i in range(3)], np.int32)
    lib = capi.load_planner()
    h = sc.product_snapshot()
    try:
        why = explain_plan_arrays(checker, h, sc.ptr, cand_off, cand_pods, np.zeros(2, np.int32), None, node_mask=False)
        assert list(why.feasible) == [0, 0] and list(why.first) == [-1, -1] and not why.counts.any()
        res = blockers_plan_arrays(checker, h, sc.ptr, cand_off, cand_pods, np.zeros(2, np.int32))
        assert list(res.blockers) == [2, 1] and list(res.first) == [0, 0]
        assert list(res.node_of_pod) == [-1, -1, -1] and not res.counts.any() and not res.fallback.any()
    finally:
        lib.sr_snapshot_destroy(h)


def test_nothing_asked_and_no_candidates(checker):
    b = B.Built(CASES[0])
    lib = capi.load_planner()
    h = b.sc.product_snapshot()
    try:
        res = blockers_plan_arrays(checker, h, b.sc.ptr, b.cand_off, b.cand_pods, np.full(len(b.ask), -1, np.int32))
        assert (res.how == B.NONE).all() and (res.blockers == -1).all() and (res.first == -1).all()
        assert (res.node_of_pod == -1).all() and not res.counts.any() and not res.fallback.any()
        none = blockers_plan_arrays(checker, h, b.sc.ptr, np.zeros(1, np.int32), np.zeros(0, np.int32),
                                    np.zeros(0, np.int32))
        assert len(none.blockers) == 0 and none.ranking() == []
    finally:
        lib.sr_snapshot_destroy(h)


def test_ranking_and_mirror(checker):
    """rescheduler.blockersPlan on Pod / Node objects, and the ranking an operator reads."""
    from known_answer import N, P, used
    from spotplanner import nodes as NM
    from spotplanner.rescheduler import blockersPlan
    nodes = [N("n%d" % i, cpu=1000) for i in range(4)]
    base = [[], [], [used(cpu=950, name="b2")], [used(cpu=950, name="b3")]]
    cands = [[P("c0-0", cpu=600)],
             [P("c1-%d" % k, cpu=600) for k in range(4)],                      # two fit, two do not
             [],
             [P("c3-0", cpu=300), P("c3-1", cpu=1001), P("c3-2", cpu=300)],     # one blocker in the middle
             [P("c4-%d" % k, cpu=1001 + k) for k in range(3)]]                  # three blockers
    infos = NM.NodeInfoArray(NM.NodeInfo(n, ps, 0, 0) for n, ps in zip(nodes, base))
    snapshot = infos.GetClusterSnapshot()
    try:
        flat = [p for c in cands for p in c]
        enc = snapshot.encode_pods(flat)
        cand_off = np.zeros(len(cands) + 1, np.int32)
        cand_off[1:] = np.cumsum([len(c) for c in cands])
        plan = plan_arrays(checker, snapshot.handle, enc.ptr, cand_off, np.arange(len(flat), dtype=np.int32))
        assert list(plan.status) == [capi.SR_CAND_OK, 2, capi.SR_CAND_EMPTY, 1, 0]
        states = [snapshot.node_state(n.name) for n in nodes]
        res = blockersPlan(checker, snapshot, infos, cands, plan)
        assert [snapshot.node_state(n.name) for n in nodes] == states
        assert list(res.blockers) == [-1, 2, -1, 1, 3] and list(res.first) == [-1, 2, -1, 1, 0]
        assert res.ranking() == [3, 1, 4]
        assert res.blocker_pods(1) == [2, 3] and res.blocker_pods(3) == [1] and res.blocker_pods(0) == []
        assert list(res.node_of_pod[cand_off[3]:cand_off[4]]) == [0, -1, 0]
        assert blockersPlan(checker, snapshot, infos, cands, plan, counts=False).counts is None
    finally:
        snapshot.close()


def test_argument_errors_leave_the_snapshot_alone(checker):
    b = B.Built(CASES[0])
    lib = capi.load_planner()
    h = b.sc.product_snapshot()
    try:
        before = _node_states(lib, h, b.n_spot)
        n = len(b.ask)
        total = len(b.cand_pods)
        a, m = np.zeros(n, np.int32), np.zeros(total, np.int32)
        cands = capi.sr_candidates(n, capi.ptr(b.cand_off, capi.P32), capi.ptr(b.cand_pods, capi.P32), None)
        ASK = capi.ptr(b.ask, capi.P32)

        def out(**kw):
            f = dict(blockers=capi.ptr(a, capi.P32), first=capi.ptr(a, capi.P32), node_of_pod=capi.ptr(m, capi.P32))
            f.update(kw)
            return capi.sr_blockers_out(f["blockers"], f["first"], f["node_of_pod"], None, None)
        bad = capi.SR_ERR_INVALID_ARG
        o = out()
        assert lib.sr_blockers_plan(checker.handle, h, b.sc.ptr, ctypes.byref(cands), None, ctypes.byref(o), None) == bad
        for missing in ("blockers", "first", "node_of_pod"):
            o = out(**{missing: None})
            assert lib.sr_blockers_plan(checker.handle, h, b.sc.ptr, ctypes.byref(cands), ASK, ctypes.byref(o), None) == bad
        pods = b.cand_pods.copy()
        pods[1] = 10 ** 6
        with pytest.raises(PlannerError) as e:
            blockers_plan_arrays(checker, h, b.sc.ptr, b.cand_off, pods, b.ask)
        assert e.value.status == bad
        # ... but not in a candidate that is not asked
        skip = int(b.cand_off[5])
        pods = b.cand_pods.copy()
        pods[skip] = 10 ** 6
        assert b.ask[5] < 0
        assert list(blockers_plan_arrays(checker, h, b.sc.ptr, b.cand_off, pods, b.ask).blockers) == list(b.blockers)
        assert _node_states(lib, h, b.n_spot) == before
        assert lib.sr_snapshot_fork(h) == capi.SR_OK
        with pytest.raises(PlannerError) as e:
            blockers_plan_arrays(checker, h, b.sc.ptr, b.cand_off, b.cand_pods, b.ask)
        assert e.value.status == capi.SR_ERR_STATE
        assert lib.sr_snapshot_revert(h) == capi.SR_OK
        assert _node_states(lib, h, b.n_spot) == before
    finally:
        lib.sr_snapshot_destroy(h)


def test_plans_around_a_call_are_identical():
    """The third plan of one input on a fresh context, with and without an sr_blockers_plan call before it:
    statuses, mapping and the steady prepare's upload are the same; and a resident workload's sr_plan_run gives
    the same result after a call as before it."""
    sc, cand_off, cand_pods, _ = _steady_scenario()
    lib = capi.load_planner()
    seen = []
    for ask_blockers in (False, True):
        ck = make_checker()
        h = sc.product_snapshot()
        try:
            for _ in range(2):
                first = plan_arrays(ck, h, sc.ptr, cand_off, cand_pods)
            if ask_blockers:
                res = blockers_plan_arrays(ck, h, sc.ptr, cand_off, cand_pods, first.status)
                # the five 600m pods of the last candidate meet four open nodes: the fifth is its only blocker
                assert list(first.status) == [capi.SR_CAND_OK, capi.SR_CAND_OK, 4]
                assert list(res.how) == [B.NONE, B.NONE, B.BATCHED] and list(res.blockers) == [-1, -1, 1]
                assert list(res.node_of_pod[int(cand_off[2]):]) == [0, 1, 2, 3, -1]
            p = plan_arrays(ck, h, sc.ptr, cand_off, cand_pods)
            t = ck.timing()
            seen.append((list(p.status), list(p.node_of_pod), p.winner, list(p.winner_map), int(t.bytes_uploaded),
                         int(t.enc_reused), int(t.k0_columns)))
            assert list(first.status) == list(p.status) and list(first.node_of_pod) == list(p.node_of_pod)
            # the resident workload: run, call, run
            n = len(cand_off) - 1
            c = capi.sr_candidates(n, capi.ptr(cand_off, capi.P32), capi.ptr(cand_pods, capi.P32), None)
            assert lib.sr_plan_prepare(ck.handle, h, sc.ptr, ctypes.byref(c)) == capi.SR_OK, ck.last_error()
            runs = []
            for r in range(2):
                status, nodes = np.zeros(n, np.int32), np.zeros(len(cand_pods), np.int32)
                out = capi.sr_plan_out()
                out.status, out.node_of_pod = capi.ptr(status, capi.P32), capi.ptr(nodes, capi.P32)
                assert lib.sr_plan_run(ck.handle, ctypes.byref(out)) == capi.SR_OK, ck.last_error()
                runs.append((list(status), list(nodes), out.winner, out.first_ok))
                if r == 0 and ask_blockers:
                    blockers_plan_arrays(ck, h, sc.ptr, cand_off, cand_pods, first.status)
            assert runs[0] == runs[1] and runs[0][0] == list(p.status)
        finally:
            lib.sr_snapshot_destroy(h)
            ck.close()
    print("third plan without / with an sr_blockers_plan call before it:", seen)
    assert seen[0] == seen[1]
    assert seen[0][5] == 1  # a steady prepare: the candidate side was reused
