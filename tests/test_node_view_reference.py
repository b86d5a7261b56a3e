"""sr_node_view_pods / sr_node_view_plan without a GPU: the interface, and everything but the kernels through the
host view (lib/libsrexplainview.so: sr_node_view_pods_view, sr_node_view_plan_view), which folds every judged
query into every node's row by node_view_fold -- the statement the kernels follow -- and takes the rows through
the device layout and the planner's unpacking.  The hand cases of tests/node_view_sizes.py and the twelve random
clusters of test_shortfall_reference, against node_view_ref.fold of masks and shortfalls the oracle has checked
(tests/shortfall_ref.py).  It also proves on the oracle what the GPU tests' random seeds rely on.
test_gpu_node_view.py and test_gpu_node_view_sizes.py run the C ABI."""
import ctypes

import numpy as np
import pytest

import explain_plan_cases as C
import node_view_ref as V
import node_view_sizes as NS
import shortfall_ref as R
from helpers import header_functions
from oracle_lib import oracle_plan
from spotplanner import capi
from test_shortfall_reference import RUN_IDS, RUNS, random_reference

CASES = NS.cases()
RESOURCE_REASONS = [capi.WHY_NAMES.index(n) for n in ("PODS", "CPU", "MEMORY", "EPHEMERAL")]


def test_entry_points_exported_and_bound():
    lib = capi.load_planner()
    for name, nargs in (("sr_node_view_pods", 6), ("sr_node_view_plan", 8)):
        assert name in capi.EXPORTED and name in header_functions()
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == nargs
    assert capi.SR_ABI_VERSION == 11 and lib.sr_abi_version() == 11
    assert [f for f, _ in capi.sr_node_view_out._fields_] == ["judged", "admits", "near", "refuses", "sole", "sole_min",
                                                              "sole_at", "fallback"]
    assert ctypes.sizeof(capi.sr_node_view_out) == 8 * ctypes.sizeof(ctypes.c_void_p)
    # no existing struct changed its layout
    assert [f for f, _ in capi.sr_explain_out._fields_] == ["feasible", "first", "counts", "node_mask", "fallback"]
    assert [f for f, _ in capi.sr_shortfall_out._fields_] == ["near", "only_nodes", "only_min", "only_at", "node_short"]


def test_null_arguments_are_refused_before_the_context_is_looked_at():
    lib = capi.load_planner()
    b = C.Built(NS.hand_tick().plan)
    sc = b.sc
    h = sc.product_snapshot()
    try:
        n = len(b.cand_off) - 1
        a32, a64 = np.zeros(64, np.int32), np.zeros(64, np.int64)
        how = np.zeros(n, np.uint8)
        P32, P64 = capi.ptr(a32, capi.P32), capi.ptr(a64, capi.P64)

        def out(**missing):
            o = capi.sr_node_view_out(P32, P32, P32, P32, P32, P64, P32, None)
            for k in missing:
                setattr(o, k, None)
            return o
        cands = capi.sr_candidates(n, capi.ptr(b.cand_off, capi.P32), capi.ptr(b.cand_pods, capi.P32), None)
        AT, MAP, HOW = capi.ptr(b.at_pod, capi.P32), capi.ptr(b.node_of_pod, capi.P32), capi.ptr(how, capi.PU8)
        PODS = capi.ptr(b.cand_pods, capi.P32)
        bad, fake = capi.SR_ERR_INVALID_ARG, ctypes.c_void_p(1)  # (never dereferenced: no context without a GPU)
        O, CN = ctypes.byref(out()), ctypes.byref(cands)
        assert lib.sr_node_view_pods(None, h, sc.ptr, PODS, 1, O) == bad
        assert lib.sr_node_view_pods(fake, None, sc.ptr, PODS, 1, O) == bad
        assert lib.sr_node_view_pods(fake, h, None, PODS, 1, O) == bad
        assert lib.sr_node_view_pods(fake, h, sc.ptr, None, 1, O) == bad
        assert lib.sr_node_view_pods(fake, h, sc.ptr, PODS, -1, O) == bad
        assert lib.sr_node_view_pods(fake, h, sc.ptr, PODS, 1, None) == bad
        assert lib.sr_node_view_plan(None, h, sc.ptr, CN, AT, MAP, O, HOW) == bad
        assert lib.sr_node_view_plan(fake, None, sc.ptr, CN, AT, MAP, O, HOW) == bad
        assert lib.sr_node_view_plan(fake, h, None, CN, AT, MAP, O, HOW) == bad
        assert lib.sr_node_view_plan(fake, h, sc.ptr, None, AT, MAP, O, HOW) == bad
        assert lib.sr_node_view_plan(fake, h, sc.ptr, CN, None, MAP, O, HOW) == bad
        assert lib.sr_node_view_plan(fake, h, sc.ptr, CN, AT, None, O, HOW) == bad
        assert lib.sr_node_view_plan(fake, h, sc.ptr, CN, AT, MAP, None, HOW) == bad
        for missing in ("judged", "admits", "near", "refuses", "sole", "sole_min", "sole_at"):
            o = out(**{missing: True})
            assert lib.sr_node_view_pods(fake, h, sc.ptr, PODS, 1, ctypes.byref(o)) == bad, missing
            assert lib.sr_node_view_plan(fake, h, sc.ptr, CN, AT, MAP, ctypes.byref(o), HOW) == bad, missing
        at_pod = b.at_pod.copy()  # at_pod >= the candidate's pods; a position below at_pod out of range
        at_pod[0] = 5
        assert lib.sr_node_view_plan(fake, h, sc.ptr, CN, capi.ptr(at_pod, capi.P32), MAP, O, HOW) == bad
        for pos in (-1, b.n_spot):
            m = b.node_of_pod.copy()
            m[0] = pos
            assert lib.sr_node_view_plan(fake, h, sc.ptr, CN, AT, capi.ptr(m, capi.P32), O, HOW) == bad
        assert lib.sr_snapshot_fork(h) == capi.SR_OK
        assert lib.sr_node_view_plan(fake, h, sc.ptr, CN, AT, MAP, O, HOW) == capi.SR_ERR_STATE
    finally:
        lib.sr_snapshot_destroy(h)


def test_fold_by_hand():
    """The reference itself on numbers small enough to fold in the head: two nodes, three queries."""
    CPU, TAINT = 1 << 4, 1 << 1
    masks = [[CPU, 0], [CPU, TAINT], [CPU | TAINT, 0]]
    shorts = [[[7, 0, 0, 0], [0] * 4], [[7, 0, 0, 0], [0] * 4], [[1, 0, 0, 0], [0] * 4]]
    got = V.fold(masks, shorts, [5, 2, 9], 2)
    assert got["judged"] == 3 and got["admits"] == [0, 2] and got["near"] == [2, 0]
    assert got["refuses"][0][4] == 3 and got["refuses"][0][1] == 1 and got["refuses"][1][1] == 1
    assert got["sole"][0][4] == 2 and got["sole"][0][1] == 0 and got["sole"][1][1] == 1
    assert got["sole_min"][0] == [7, 0, 0, 0] and got["sole_at"][0] == [2, -1, -1, -1]  # 1 is no sole shortfall
    assert got["sole_min"][1] == [0] * 4 and got["sole_at"][1] == [-1] * 4


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_hand_cases(case):
    """Every judged candidate's hand-written masks and shortfalls hold on the oracle in its context; their fold is
    the hand-written result; the view gives the hand-written masks' fold over the candidates it evaluates (the
    batched ones), and the hand-written result itself where no judged candidate goes one at a time."""
    b = C.Built(case.plan)
    osnap = b.sc.oracle_snapshot()
    n_spot, fb = b.n_spot, case.expected_fallback()
    judged = [c for c, cd in enumerate(case.plan.cands) if cd.at_pod >= 0 and not fb[c]]
    for c in judged:
        lo, k = int(b.cand_off[c]), case.plan.cands[c].at_pod
        with R.context(b.sc, osnap, b.cand_pods[lo:], b.node_of_pod[lo:], k):
            R.check_query(b.sc, osnap, b.cand_pods[lo + k], case.plan.expected(c), case.expected_shorts(c), n_spot,
                          (case.name, c))
    want = case.expanded()
    V.same(V.fold([case.plan.expected(c) for c in judged], [case.expected_shorts(c) for c in judged], judged, n_spot),
           want, case.name)
    got, fallback, how = V.view_plan(b.sc, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
    assert [int(x) for x in how] == [cd.how for cd in case.plan.cands]
    batched = [c for c in judged if case.plan.cands[c].how == C.BATCHED]
    sv = R.view_plan(b.sc, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
    for c in batched:
        assert [int(m) for m in sv["masks"][c]] == case.plan.expected(c), (case.name, c)
        assert [[int(x) for x in r] for r in sv["shorts"][c]] == case.expected_shorts(c), (case.name, c)
    V.same(got, V.fold([case.plan.expected(c) for c in batched], [case.expected_shorts(c) for c in batched], batched,
                       n_spot), case.name)
    if batched == judged:
        V.same(got, want, case.name)
        assert [int(x) for x in fallback] == [f if case.plan.cands[c].how == C.BATCHED else 0 for c, f in enumerate(fb)]
    if case.as_pods:
        assert all(cd.at_pod == 0 for cd in case.plan.cands)
        got, fallback = V.view_pods(b.sc, b.cand_pods)
        V.same(got, want, case.name)
        assert not fallback.any()


def test_cases_cover_the_issue():
    by = {c.name: c for c in CASES}
    assert by["hand_tick"].expanded()["sole_min"][2] == [200, 0, 0, 0] and by["hand_tick"].expanded()["sole_at"][2][0] == 0
    t = by["leftover_taint"].expanded()
    taint, cpu = capi.WHY_NAMES.index("TAINT"), capi.WHY_NAMES.index("CPU")
    assert t["sole"][0][taint] == 3 and t["refuses"][1][taint] == 3 and t["refuses"][1][cpu] == 3 and not any(t["sole"][1])
    assert by["tie_lower_slot"].expanded()["sole_at"][0][0] == 1
    s = by["tie_single_and_batched"]
    assert [cd.how for cd in s.plan.cands] == [C.SINGLE, C.BATCHED] and s.expanded()["sole_at"][0][0] == 0
    f = by["fallback_and_not_asked"]
    assert f.fallback == [0, 1, 0, 0] and f.plan.cands[2].at_pod < 0 and f.want["judged"] == 2
    p = by["pods_saturate"].expanded()
    assert p["sole_min"][0][3] == (1 << 63) - 1 and p["sole_min"][2][3] == (1 << 63) - 2 and p["sole_at"][2][3] == 1
    a = by["admits_and_refuses"].expanded()
    assert a["admits"][0] == 1 and a["refuses"][0][cpu] == 1
    z = by["none_judged"].expanded()
    assert z["judged"] == 0 and not any(z["admits"]) and all(r == [-1] * 4 for r in z["sole_at"])


def seed_conditions(want):
    """What the random inputs must show for the GPU run to prove anything: a node with a sole count in a reason
    that is no resource, a node with a sole shortfall, a node that both admits and refuses."""
    n = len(want["admits"])
    other = any(want["sole"][j][r] for j in range(n) for r in range(capi.SR_WHY_COUNT) if r not in RESOURCE_REASONS)
    short = any(x > 0 for j in range(n) for x in want["sole_min"][j])
    both = any(want["admits"][j] > 0 and any(want["refuses"][j]) for j in range(n))
    return other, short, both


@pytest.mark.parametrize("kind,seed", RUNS, ids=RUN_IDS)
def test_random_clusters_through_the_view(kind, seed):
    ref, cand_off, cand_pods = random_reference(kind, seed)
    sc, osnap, n_spot = ref.sc, ref.osnap, ref.n_spot
    v = R.view_pods(sc, cand_pods)
    ref.check(v["masks"], v["shorts"], v["fallback"])   # the oracle's word on every mask and shortfall
    q = [i for i in range(len(cand_pods)) if not v["fallback"][i]]
    want = V.fold([v["masks"][i] for i in q], [v["shorts"][i] for i in q], q, n_spot)
    got, fallback = V.view_pods(sc, cand_pods)
    V.same(got, want, (kind, seed))
    assert np.array_equal(fallback, v["fallback"])
    cond = seed_conditions(want)
    print(kind, seed, "judged", want["judged"], "sole in a non-resource reason, sole shortfall, admits and refuses:", cond)
    assert all(cond), (kind, seed, cond)
    # the oracle's plan: every batched stuck candidate in the context of its earlier pods, slot = candidate
    plan = oracle_plan(osnap, sc.ptr, cand_off, cand_pods, mode=1)
    at_pod = np.ascontiguousarray(plan["status"], np.int32)
    mapping = np.ascontiguousarray(plan["node_of_pod"], np.int32)
    pv = R.view_plan(sc, cand_off, cand_pods, at_pod, mapping)
    judged = []
    for c in range(len(at_pod)):
        if at_pod[c] < 0 or pv["how"][c] != C.BATCHED or pv["fallback"][c]:
            continue
        lo = int(cand_off[c])
        with R.context(sc, osnap, cand_pods[lo:], mapping[lo:], int(at_pod[c])):
            R.check_query(sc, osnap, cand_pods[lo + at_pod[c]], pv["masks"][c], pv["shorts"][c], n_spot, c)
        judged.append(c)
    assert judged
    got, fallback, how = V.view_plan(sc, cand_off, cand_pods, at_pod, mapping)
    V.same(got, V.fold([pv["masks"][c] for c in judged], [pv["shorts"][c] for c in judged], judged, n_spot), (kind, seed))
    assert np.array_equal(how, pv["how"]) and np.array_equal(fallback, pv["fallback"])
