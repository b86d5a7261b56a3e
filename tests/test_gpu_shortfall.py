"""sr_shortfall_pods / sr_shortfall_plan on the GPU: random clusters against the oracle's arithmetic
(tests/shortfall_ref.py) per node and per reduction, `why` against sr_explain_pods / sr_explain_plan array for
array, the batched pass against the per-candidate loop (Fork, AddPod, sr_shortfall_pods, Revert), the hand tick
of DESIGN.md 1.2, the single path, fallback pods, planning around the calls, and the Pod / Node layer."""
import contextlib

import numpy as np
import pytest

import explain_plan_cases as C
import shortfall_ref as R
import shortfall_sizes as S
from helpers import Scenario
from known_answer import N, P, used
from oracle_lib import oracle_plan
from spotplanner import capi
from spotplanner.model import Container, Pod, Taint
from spotplanner.rescheduler import (explain_arrays, explain_plan_arrays, plan_arrays, shortfall_arrays,
                                     shortfall_plan_arrays)
from test_gpu_explain import _node_states, _steady_scenario
from test_gpu_k2_dispatch import make_checker
from test_shortfall_reference import NEAR_FLOOR, RUN_IDS, RUNS, random_reference

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def snapshot(sc):
    h = sc.product_snapshot()
    try:
        yield h
    finally:
        capi.load_planner().sr_snapshot_destroy(h)


def same_why(a, b):
    """Two ExplainResults, array for array."""
    for f in ("feasible", "first", "counts", "fallback", "node_mask"):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), f
    assert (a.how is None) == (b.how is None) and (a.how is None or np.array_equal(a.how, b.how))


def same_short(a, i, b, k=0, what=""):
    """Entry i of a ShortfallResult equals entry k of another, field for field."""
    assert a.near[i] == b.near[k], (what, i, a.near[i], b.near[k])
    for f in ("only_nodes", "only_min", "only_at", "node_short"):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None) and (x is None or np.array_equal(x[i], y[k])), (what, f, i)


def in_loop(ck, h, sc, pods, mapping, k):
    """What the per-candidate loop gives pods[k]: Fork, AddPod of pods[:k] at mapping[:k], sr_shortfall_pods,
    Revert."""
    lib = capi.load_planner()
    assert lib.sr_snapshot_fork(h) == capi.SR_OK
    try:
        for q in range(k):
            assert lib.sr_snapshot_add_pod(h, sc.ptr, int(pods[q]), int(mapping[q])) == capi.SR_OK
        return shortfall_arrays(ck, h, sc.ptr, np.array([pods[k]], np.int32))
    finally:
        assert lib.sr_snapshot_revert(h) == capi.SR_OK


@pytest.mark.parametrize("kind,seed", RUNS, ids=RUN_IDS)
def test_random_clusters(checker, kind, seed):
    ref, cand_off, cand_pods = random_reference(kind, seed)
    with snapshot(ref.sc) as h:
        why, short = shortfall_arrays(checker, h, ref.sc.ptr, cand_pods)
        same_why(why, explain_arrays(checker, h, ref.sc.ptr, cand_pods))
        _, bare = shortfall_arrays(checker, h, ref.sc.ptr, cand_pods, node_short=False, why=False)
    want = ref.check(why.node_mask, short.node_short, why.fallback)
    assert bare.node_short is None
    near = 0
    for i, w in enumerate(want):
        if w is None:
            R.check_none(short, i)
            R.check_none(bare, i)
            continue
        R.check_reduced(short, i, w)
        R.check_reduced(bare, i, w)
        near += int(w[0] >= 1)
    print(kind, seed, "judged pods with a near miss:", near)
    assert near >= NEAR_FLOOR


@pytest.mark.parametrize("kind,seed", RUNS, ids=RUN_IDS)
def test_random_plans(checker, kind, seed):
    """The oracle's plan: every stuck candidate in one call equals the per-candidate loop and, on the batched
    way, the oracle's arithmetic after the same fill; `why` and out_how are sr_explain_plan's."""
    ref, cand_off, cand_pods = random_reference(kind, seed)
    sc, osnap, n_spot = ref.sc, ref.osnap, ref.n_spot
    lib = capi.load_planner()
    plan = oracle_plan(osnap, sc.ptr, cand_off, cand_pods, mode=1)
    at_pod = np.ascontiguousarray(plan["status"], np.int32)
    mapping = np.ascontiguousarray(plan["node_of_pod"], np.int32)
    with snapshot(sc) as h:
        before = _node_states(lib, h, n_spot)
        why, short = shortfall_plan_arrays(checker, h, sc.ptr, cand_off, cand_pods, at_pod, mapping)
        assert _node_states(lib, h, n_spot) == before
        same_why(why, explain_plan_arrays(checker, h, sc.ptr, cand_off, cand_pods, at_pod, mapping))
        ways = [0, 0]
        for c in range(len(at_pod)):
            if at_pod[c] < 0:
                assert why.how[c] == C.NONE
                R.check_none(short, c)
                continue
            lo, k = int(cand_off[c]), int(at_pod[c])
            lw, ls = in_loop(checker, h, sc, cand_pods[lo:], mapping[lo:], k)
            assert np.array_equal(why.node_mask[c], lw.node_mask[0]) and why.fallback[c] == lw.fallback[0], c
            same_short(short, c, ls, 0, c)
            ways[int(why.how[c] == C.SINGLE)] += 1
            if why.fallback[c]:
                R.check_none(short, c)
                continue
            with R.context(sc, osnap, cand_pods[lo:], mapping[lo:], k):
                red = R.check_query(sc, osnap, cand_pods[lo + k], why.node_mask[c], short.node_short[c], n_spot, c)
            R.check_reduced(short, c, red, c)
        assert _node_states(lib, h, n_spot) == before
    print(kind, seed, "stuck candidates batched, single:", ways)
    assert ways[0] + ways[1] >= 1


def test_hand_tick(checker):
    """five 600m pods, four open 1000m nodes."""
    b = S.hand_tick()
    with snapshot(b.sc) as h:
        why, short = shortfall_arrays(checker, h, b.sc.ptr, b.cand_pods[4:5])
        assert why.feasible[0] == 4 and short.near[0] == 0
        assert not short.only_nodes[0].any() and not short.only_min[0].any() and list(short.only_at[0]) == [-1] * 4
        assert not short.node_short[0].any()
        why, short = shortfall_plan_arrays(checker, h, b.sc.ptr, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
    assert list(why.how) == [C.BATCHED] and why.feasible[0] == 0
    assert short.near[0] == 4 and list(short.only_nodes[0]) == [4, 0, 0, 0]
    assert list(short.only_min[0]) == [200, 0, 0, 0] and list(short.only_at[0]) == [0, -1, -1, -1]
    assert [list(r) for r in short.node_short[0]] == [[200, 0, 0, 0]] * 4


def test_single_path_host_port(checker):
    """A host-port stop pod after a host-port pod goes one at a time: node 7 holds the earlier pod's port (no near
    miss), node 3 is 100m short (500m taken of 1000m, 600m asked), node 5 has no slot left."""
    n = 63
    nodes = C.pool(n, over={5: dict(pods=1)})
    base = [[] for _ in range(n)]
    base[3] = [used(cpu=500)]
    base[5] = [used(cpu=1, name="f")]
    cand = C.Cand([C._hp("a0", 80), C._hp("a1", 80, cpu=600)], 1, [7, -1], C.SINGLE,
                  {3: C.CPU, 5: C.PODS, 7: C.PORTS})
    b = C.Built(C.PlanCase("single", nodes, base, [cand]))
    lib = capi.load_planner()
    with snapshot(b.sc) as h:
        before = _node_states(lib, h, n)
        why, short = shortfall_plan_arrays(checker, h, b.sc.ptr, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
        assert _node_states(lib, h, n) == before
        _, ls = in_loop(checker, h, b.sc, b.cand_pods, b.node_of_pod, 1)
    assert list(why.how) == [C.SINGLE] and [int(m) for m in why.node_mask[0]] == b.case.expected(0)
    same_short(short, 0, ls)
    assert short.near[0] == 2 and list(short.only_nodes[0]) == [1, 0, 0, 1]
    assert list(short.only_min[0]) == [100, 0, 0, 1] and list(short.only_at[0]) == [3, -1, -1, 5]
    want = np.zeros((n, 4), np.int64)
    want[3, 0], want[5, 3] = 100, 1
    assert np.array_equal(short.node_short[0], want)


def test_fallback_pod_in_a_batch_then_alone(checker):
    nodes = [N("a", cpu=1000), N("b", cpu=1000, taints=[Taint("k", "v", "NoSchedule")]), N("c", cpu=1000)]
    base = [[used(cpu=950)], [], []]
    sc = Scenario(nodes, base, [P("p0", cpu=100), Pod("fb", containers=[Container(cpu_milli=100)], has_pvc=True),
                                P("p2", cpu=0)])
    q = [sc.qidx(i) for i in range(3)]
    with snapshot(sc) as h:
        why, short = shortfall_arrays(checker, h, sc.ptr, np.array(q, np.int32))
        _, alone = shortfall_arrays(checker, h, sc.ptr, np.array(q[1:2], np.int32))
        # the same three as candidates of one pod each: the batch holds other pods, so the fallback pod is asked
        # again alone and stays outside the encoded set
        off = np.arange(4, dtype=np.int32)
        pw, ps = shortfall_plan_arrays(checker, h, sc.ptr, off, np.array(q, np.int32), np.zeros(3, np.int32), None)
    assert list(why.fallback) == [0, 1, 0]
    R.check_none(short, 1)
    R.check_none(alone, 0)
    assert short.near[0] == 1 and list(short.only_min[0]) == [50, 0, 0, 0] and list(short.only_at[0]) == [0, -1, -1, -1]
    assert [list(r) for r in short.node_short[0]] == [[50, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert short.near[2] == 0 and not short.node_short[2].any()
    assert list(pw.how) == [C.BATCHED, C.SINGLE, C.BATCHED] and list(pw.fallback) == [0, 1, 0]
    R.check_none(ps, 1)
    for i in (0, 2):
        same_short(ps, i, short, i)


def test_port_bits_exhausted(checker):
    """More host ports among the stop pods than one encode's state word holds: the pods handed back as fallback
    are asked again alone, and their shortfalls are the ones sr_shortfall_pods gives them alone."""
    case = C.port_bits_case()
    b = C.Built(case)
    with snapshot(b.sc) as h:
        why, short = shortfall_plan_arrays(checker, h, b.sc.ptr, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
        same_why(why, explain_plan_arrays(checker, h, b.sc.ptr, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod))
        assert [int(x) for x in why.how] == [cd.how for cd in case.cands]
        for c, cd in enumerate(case.cands):
            lo = int(b.cand_off[c])
            _, ls = in_loop(checker, h, b.sc, b.cand_pods[lo:], b.node_of_pod[lo:], cd.at_pod)
            same_short(short, c, ls, 0, c)
    R.check_none(short, C.N_PORT_PODS)
    last = len(case.cands) - 1
    assert short.near[last] == 1 and list(short.only_min[last]) == [1, 0, 0, 0] and short.only_at[last][0] == 62


def test_plans_around_the_calls_are_identical():
    """The third plan of one input on a fresh context, with and without shortfall calls before it: statuses,
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
                why, short = shortfall_plan_arrays(ck, h, sc.ptr, cand_off, cand_pods, first.status, first.node_of_pod)
                assert list(why.how) == [C.NONE, C.NONE, C.BATCHED]
                # four open nodes 200m short after the candidate's four pods, four closed ones 550m short
                assert short.near[2] == 8 and list(short.only_min[2]) == [200, 0, 0, 0] and short.only_at[2][0] == 0
                _, s2 = shortfall_arrays(ck, h, sc.ptr, cand_pods)
                assert s2.near[0] == 4 and list(s2.only_min[0]) == [550, 0, 0, 0] and s2.only_at[0][0] == 4
            p = plan_arrays(ck, h, sc.ptr, cand_off, cand_pods)
            t = ck.timing()
            seen.append((list(p.status), list(p.node_of_pod), p.winner, list(p.winner_map), int(t.bytes_uploaded),
                         int(t.enc_reused), int(t.k0_columns)))
            assert list(first.status) == list(p.status) and list(first.node_of_pod) == list(p.node_of_pod)
        finally:
            lib.sr_snapshot_destroy(h)
            ck.close()
    print("third plan without / with shortfall calls before it:", seen)
    assert seen[0] == seen[1]
    assert seen[0][5] == 1  # a steady prepare: the candidate side was reused


def test_one_context_alternating_calls():
    """Shortfall, explain and plan calls in turn on one context: every round gives what the first gave."""
    sc, cand_off, cand_pods, _ = _steady_scenario()
    ck = make_checker()
    h = sc.product_snapshot()
    try:
        rounds = []
        for _ in range(3):
            plan = plan_arrays(ck, h, sc.ptr, cand_off, cand_pods)
            w1, s1 = shortfall_arrays(ck, h, sc.ptr, cand_pods)
            e1 = explain_arrays(ck, h, sc.ptr, cand_pods)
            w2, s2 = shortfall_plan_arrays(ck, h, sc.ptr, cand_off, cand_pods, plan.status, plan.node_of_pod)
            e2 = explain_plan_arrays(ck, h, sc.ptr, cand_off, cand_pods, plan.status, plan.node_of_pod)
            same_why(w1, e1)
            same_why(w2, e2)
            rounds.append((list(plan.status), list(plan.node_of_pod), s1, s2, e1, e2))
        for r in rounds[1:]:
            assert r[:2] == rounds[0][:2]
            for k in (2, 3):
                for i in range(len(r[k].near)):
                    same_short(r[k], i, rounds[0][k], i)
            same_why(r[4], rounds[0][4])
            same_why(r[5], rounds[0][5])
    finally:
        capi.load_planner().sr_snapshot_destroy(h)
        ck.close()


def test_pod_and_node_layer(checker):
    """rescheduler.shortfallPods / shortfallPlan on Pod / Node objects against the array functions."""
    from spotplanner import nodes as NM
    from spotplanner.rescheduler import shortfallPlan, shortfallPods
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
        why, short = shortfallPlan(checker, snap, infos, cands, plan)
        aw, ash = shortfall_plan_arrays(checker, snap.handle, enc.ptr, cand_off, idx, plan.status, plan.node_of_pod)
        assert [snap.node_state(n.name) for n in nodes] == states
        same_why(why, aw)
        for c in range(len(cands)):
            same_short(short, c, ash, c)
        assert list(why.how) == [C.NONE, C.BATCHED, C.NONE, C.BATCHED]
        assert short.closest(1) == {"CPU": (200, 0)} and short.near[1] == 8
        # 1001m after three 300m pods on node 0: 901m short there, 1m on the open nodes 1 .. 3, 951m on the rest
        assert short.closest(3) == {"CPU": (1, 1)} and list(short.node_short[3][0]) == [901, 0, 0, 0]
        R.check_none(short, 0)
        pw, psh = shortfallPods(checker, snap, infos, flat)
        bw, bsh = shortfall_arrays(checker, snap.handle, enc.ptr, idx)
        same_why(pw, bw)
        for i in range(len(flat)):
            same_short(psh, i, bsh, i)
        assert psh.closest(0) == {"CPU": (550, 4)} and psh.closest(len(flat) - 1) == {"CPU": (1, 0)}
    finally:
        snap.close()
