"""sr_explain_plan without a GPU: the interface, and everything but the kernel
through the host view (lib/libsrexplainview.so, tools/explain_plan_view.cpp):
which way every asked candidate goes, the context lists, the nodes' pod slack,
and every batched query's per-node masks evaluated by the unit the kernel
follows (csrc/explain_plan.cpp), against the hand cases of
tests/explain_plan_cases.py and the oracle forked and filled the same way.
test_gpu_explain_plan.py runs the same inputs through the C ABI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import explain_plan_cases as C
from helpers import Scenario, header_functions
from oracle_lib import oracle_plan
from randcluster import rand_scenario
from spotplanner import capi

CASES = C.cases()
IDS = [c.name for c in CASES]
# rand_scenario arguments of the random inputs, and the floors on at_pod > 0 candidates per seed: (batched, single)
RANDOM = {"plain": (dict(), (10, 0)), "inter_pod": (dict(anti=0.3, valid_selectors=True), (2, 5))}
# Six seeds per kind.  These clusters are tight: on most seeds (30 - 35 among them, but for plain 35 and inter-pod
# 30, 31, 35) every stop pod fits nowhere even before its candidate's earlier pods, so the base snapshot
# never misleads there.  The seeds below are the first ones from 0 on which the floors hold AND at least two
# candidates stop at a pod k > 0 that the oracle still places on the base snapshot
# (test_the_base_snapshot_misleads_on_every_seed).
SEEDS = {"plain": [22, 24, 27, 41, 72, 76], "inter_pod": [0, 7, 24, 57, 145, 154]}
RUNS = [(kind, seed) for kind in sorted(SEEDS) for seed in SEEDS[kind]]
RUN_IDS = ["%s-%d" % r for r in RUNS]
VIEW_LIB = os.path.join(capi.LIB_DIR, "libsrexplainview.so")
_view = None


def load_view():
    global _view
    if _view is None:
        if not os.path.exists(VIEW_LIB):  # host only: builds without a GPU, like the oracle
            subprocess.run(["make", "-C", capi.PKG_ROOT, "lib/libsrexplainview.so"], check=True, capture_output=True)
        lib = ctypes.CDLL(VIEW_LIB)
        PC, VP = ctypes.POINTER(capi.sr_cluster), ctypes.c_void_p
        lib.sr_snapshot_create.argtypes = [PC, capi.P32, ctypes.c_int32, capi.P32, capi.P32, ctypes.POINTER(VP)]
        lib.sr_snapshot_create.restype = ctypes.c_int32
        lib.sr_snapshot_destroy.argtypes = [VP]
        lib.sr_snapshot_destroy.restype = None
        lib.sr_explain_plan_view.argtypes = [PC, VP, ctypes.POINTER(capi.sr_candidates), capi.P32, capi.P32, capi.PU8,
                                             capi.P32, capi.P32, capi.P32, capi.P64, ctypes.c_int32, capi.P32,
                                             capi.PU8, capi.PU16, capi.PU8]
        lib.sr_explain_plan_view.restype = ctypes.c_int32
        _view = lib
    return _view


def view(sc, cand_off, cand_pods, at_pod, node_of_pod):
    """dict(how, ctx: per candidate [(node, pods, (cpu, memory, ephemeral))], slack, atom0, masks, fallback)."""
    lib = load_view()
    n, n_spot, cap = len(cand_off) - 1, len(sc.spot), max(1, len(cand_pods))
    h = ctypes.c_void_p()
    assert lib.sr_snapshot_create(sc.ptr, capi.ptr(sc.spot, capi.P32), n_spot, capi.ptr(sc.node_pod_off, capi.P32),
                                  capi.ptr(sc.node_pod_idx, capi.P32), ctypes.byref(h)) == capi.SR_OK
    how, fb = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
    off = np.zeros(n + 1, np.int32)
    node, pods, acc = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros((cap, 3), np.int64)
    slack, atom0 = np.zeros(n_spot, np.int32), np.zeros(n_spot, np.uint8)
    masks = np.zeros((max(n, 1), n_spot), np.uint16)
    c = capi.sr_candidates(n, capi.ptr(cand_off, capi.P32), capi.ptr(cand_pods, capi.P32), None)
    try:
        st = lib.sr_explain_plan_view(sc.ptr, h, ctypes.byref(c), capi.ptr(at_pod, capi.P32),
                                      capi.ptr(node_of_pod, capi.P32), capi.ptr(how, capi.PU8), capi.ptr(off, capi.P32),
                                      capi.ptr(node, capi.P32), capi.ptr(pods, capi.P32), capi.ptr(acc, capi.P64), cap,
                                      capi.ptr(slack, capi.P32), capi.ptr(atom0, capi.PU8), capi.ptr(masks, capi.PU16),
                                      capi.ptr(fb, capi.PU8))
    finally:
        lib.sr_snapshot_destroy(h)
    assert st == capi.SR_OK, st
    ctx = [[(int(node[j]), int(pods[j]), tuple(int(x) for x in acc[j])) for j in range(off[i], off[i + 1])]
           for i in range(n)]
    return dict(how=how[:n], ctx=ctx, slack=slack, atom0=atom0, masks=masks[:n], fallback=fb[:n])


def test_entry_point_exported_and_bound():
    lib = capi.load_planner()
    assert "sr_explain_plan" in capi.EXPORTED and "sr_explain_plan" in header_functions()
    assert lib.sr_explain_plan.restype is ctypes.c_int32 and len(lib.sr_explain_plan.argtypes) == 8
    assert capi.SR_ABI_VERSION == 11 and lib.sr_abi_version() == 11
    assert (capi.SR_EXPLAIN_NONE, capi.SR_EXPLAIN_BATCHED, capi.SR_EXPLAIN_SINGLE) == (C.NONE, C.BATCHED, C.SINGLE)
    assert (capi.SR_CAND_OK, capi.SR_CAND_FALLBACK, capi.SR_CAND_EMPTY) == (C.OK, C.FALLBACK, C.EMPTY)


def test_null_arguments_are_refused_before_the_context_is_looked_at():
    lib = capi.load_planner()
    b = C.Built(CASES[0])
    sc = b.sc
    h = sc.product_snapshot()
    try:
        n = len(b.cand_off) - 1
        a = np.zeros(n * 12, np.int32)
        how = np.zeros(n, np.uint8)

        def out():
            return capi.sr_explain_out(capi.ptr(a, capi.P32), capi.ptr(a, capi.P32), capi.ptr(a, capi.P32), None, None)
        cands = capi.sr_candidates(n, capi.ptr(b.cand_off, capi.P32), capi.ptr(b.cand_pods, capi.P32), None)
        AT, MAP, HOW = capi.ptr(b.at_pod, capi.P32), capi.ptr(b.node_of_pod, capi.P32), capi.ptr(how, capi.PU8)
        o = out()
        bad = capi.SR_ERR_INVALID_ARG
        fake = ctypes.c_void_p(1)  # never dereferenced: no context exists without a GPU
        assert lib.sr_explain_plan(None, h, sc.ptr, ctypes.byref(cands), AT, MAP, ctypes.byref(o), HOW) == bad
        assert lib.sr_explain_plan(fake, None, sc.ptr, ctypes.byref(cands), AT, MAP, ctypes.byref(o), HOW) == bad
        assert lib.sr_explain_plan(fake, h, None, ctypes.byref(cands), AT, MAP, ctypes.byref(o), HOW) == bad
        assert lib.sr_explain_plan(fake, h, sc.ptr, None, AT, MAP, ctypes.byref(o), HOW) == bad
        assert lib.sr_explain_plan(fake, h, sc.ptr, ctypes.byref(cands), None, MAP, ctypes.byref(o), HOW) == bad
        assert lib.sr_explain_plan(fake, h, sc.ptr, ctypes.byref(cands), AT, None, ctypes.byref(o), HOW) == bad
        assert lib.sr_explain_plan(fake, h, sc.ptr, ctypes.byref(cands), AT, MAP, None, HOW) == bad
        for missing in ("feasible", "first", "counts"):
            o = out()
            setattr(o, missing, None)
            assert lib.sr_explain_plan(fake, h, sc.ptr, ctypes.byref(cands), AT, MAP, ctypes.byref(o), HOW) == bad
        o = out()
        for cand, at in ((0, 2), (3, 1)):  # at_pod >= the candidate's pods
            at_pod = b.at_pod.copy()
            at_pod[cand] = at
            assert lib.sr_explain_plan(fake, h, sc.ptr, ctypes.byref(cands), capi.ptr(at_pod, capi.P32), MAP,
                                       ctypes.byref(o), HOW) == bad
        for pos in (-1, b.n_spot):  # a position below at_pod
            m = b.node_of_pod.copy()
            m[0] = pos
            assert lib.sr_explain_plan(fake, h, sc.ptr, ctypes.byref(cands), AT, capi.ptr(m, capi.P32), ctypes.byref(o),
                                       HOW) == bad
        pods = b.cand_pods.copy()  # a pod index out of range
        pods[1] = sc.enc.a["req_cpu"].shape[0] + 5
        c2 = capi.sr_candidates(n, capi.ptr(b.cand_off, capi.P32), capi.ptr(pods, capi.P32), None)
        assert lib.sr_explain_plan(fake, h, sc.ptr, ctypes.byref(c2), AT, MAP, ctypes.byref(o), HOW) == bad
        assert lib.sr_snapshot_fork(h) == capi.SR_OK
        assert lib.sr_explain_plan(fake, h, sc.ptr, ctypes.byref(cands), AT, MAP, ctypes.byref(o),
                                   HOW) == capi.SR_ERR_STATE
    finally:
        lib.sr_snapshot_destroy(h)


def check_against_oracle(sc, osnap, cand_off, cand_pods, at_pod, node_of_pod, v, n_spot, c):
    """Candidate c's batched masks: the oracle's yes / no and fitsRequest's bits after the same fill."""
    k = int(at_pod[c])
    lo, hi = int(cand_off[c]), int(cand_off[c + 1])
    fits, bits = C.oracle_in_context(sc, osnap, cand_pods[lo:hi], node_of_pod[lo - int(cand_off[0]):], k, n_spot)
    row = v["masks"][c]
    assert [int(m == 0) for m in row] == fits, (c, k)
    assert [int(m) & C.RESOURCE_BITS for m in row] == bits, (c, k)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hand_cases_through_the_view(case):
    b = C.Built(case)
    v = view(b.sc, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
    osnap = b.sc.oracle_snapshot()
    assert [int(x) for x in v["how"]] == [cd.how for cd in case.cands]
    if (v["how"] == C.BATCHED).any():  # slack >= 1 is the atom-0 row, on every node
        assert [int(s >= 1) for s in v["slack"]] == [int(x) for x in v["atom0"]]
    for c, cd in enumerate(case.cands):
        if cd.how == C.BATCHED:
            assert v["fallback"][c] == 0
            assert v["ctx"][c] == cd.ctx, (c, v["ctx"][c])
            assert [int(m) for m in v["masks"][c]] == case.expected(c), c
            check_against_oracle(b.sc, osnap, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod, v, b.n_spot, c)
            if cd.first is not None:
                zero = np.flatnonzero(v["masks"][c] == 0)
                assert (int(zero[0]) if len(zero) else -1) == cd.first
        else:
            assert v["ctx"][c] == [] and not v["masks"][c].any()
        if cd.how == C.SINGLE:  # the hand mask of a context the view does not evaluate: the oracle agrees with it
            lo = int(b.cand_off[c])
            fits, _ = C.oracle_in_context(b.sc, osnap, b.cand_pods[lo:], b.node_of_pod[lo:], cd.at_pod, b.n_spot)
            assert fits == [int(m == 0) for m in case.expected(c)], c


def test_cases_cover_the_edges():
    sizes = {len(c.nodes) for c in CASES}
    assert {63, 64, 65, 257, 300} <= sizes
    touched = {(len(c.nodes), e[0]) for c in CASES for cd in c.cands if cd.how == C.BATCHED for e in cd.ctx}
    assert any(j % 64 == 0 for _, j in touched) and any(j % 64 == 63 for _, j in touched)
    assert (257, 256) in touched and (300, 299) in touched and (65, 64) in touched
    long = [cd for c in CASES for cd in c.cands if cd.how == C.BATCHED and len(cd.ctx) == 70]
    assert long and len({e[0] // 64 for e in long[0].ctx}) == 3
    assert any(cd.how == C.BATCHED and cd.ctx == [] for c in CASES if len(c.nodes) == 300 for cd in c.cands)
    assert any(e[1] == 2 for c in CASES for cd in c.cands if cd.how == C.BATCHED for e in cd.ctx)  # a merged entry
    single = [c.name for c in CASES if any(cd.how == C.SINGLE for cd in c.cands)]
    assert len(single) == 6
    assert {cd.how for c in CASES for cd in c.cands} == {C.NONE, C.BATCHED, C.SINGLE}


def random_input(seed, kw):
    """A random cluster planned by the oracle: (scenario, cand_off, cand_pods, the oracle's plan)."""
    nodes, spot_pods, cands = rand_scenario(seed, n_spot=70, n_cand=40, max_pods=12, **kw)
    flat = [p for c in cands for p in c]
    sc = Scenario(nodes, spot_pods, flat)
    cand_off = np.zeros(len(cands) + 1, np.int32)
    cand_off[1:] = np.cumsum([len(c) for c in cands])
    cand_pods = np.array([sc.qidx(i) for i in range(len(flat))], np.int32)
    return sc, cand_off, cand_pods


def count_ways(how, at_pod, fallback):
    """Candidates with at_pod > 0 that went (batched and judged, single)."""
    later = np.asarray(at_pod) > 0
    return (int(np.sum((how == C.BATCHED) & later & (np.asarray(fallback) == 0))),
            int(np.sum((how == C.SINGLE) & later)))


@pytest.mark.parametrize("kind,seed", RUNS, ids=RUN_IDS)
def test_random_clusters_through_the_view(kind, seed):
    kw, floors = RANDOM[kind]
    sc, cand_off, cand_pods = random_input(seed, kw)
    osnap = sc.oracle_snapshot()
    plan = oracle_plan(osnap, sc.ptr, cand_off, cand_pods, mode=1)
    at_pod = np.ascontiguousarray(plan["status"], np.int32)
    node_of_pod = np.ascontiguousarray(plan["node_of_pod"], np.int32)
    v = view(sc, cand_off, cand_pods, at_pod, node_of_pod)
    n_spot = len(sc.spot)
    assert [int(s >= 1) for s in v["slack"]] == [int(x) for x in v["atom0"]]
    judged = 0
    for c in range(len(at_pod)):
        if at_pod[c] < 0:
            assert v["how"][c] == C.NONE
            continue
        assert v["how"][c] in (C.BATCHED, C.SINGLE)
        if v["how"][c] != C.BATCHED or v["fallback"][c]:
            continue
        judged += 1
        # the oracle stopped here: in context no node takes the pod
        assert (v["masks"][c] != 0).all(), c
        check_against_oracle(sc, osnap, cand_off, cand_pods, at_pod, node_of_pod, v, n_spot, c)
    ways = count_ways(v["how"], at_pod, v["fallback"])
    print(kind, seed, "failing", int(np.sum(at_pod >= 0)), "at k > 0: batched, single", ways, "judged", judged)
    assert ways[0] >= floors[0] and ways[1] >= floors[1], ways


def misleading_on_base(sc, osnap, cand_off, cand_pods, status):
    """Candidates that stop at a pod k > 0 the oracle still places somewhere on the base snapshot."""
    from oracle_lib import load_oracle
    ora = load_oracle()
    return sum(1 for c in range(len(status)) if status[c] > 0 and any(
        ora.oracle_check_predicates(osnap.h, sc.ptr, int(cand_pods[cand_off[c] + status[c]]), j)
        for j in range(len(sc.spot))))


@pytest.mark.parametrize("kind,seed", RUNS, ids=RUN_IDS)
def test_the_base_snapshot_misleads_on_every_seed(kind, seed):
    """On the oracle alone: the inputs of the GPU test show the fact sr_explain_plan exists for."""
    sc, cand_off, cand_pods = random_input(seed, RANDOM[kind][0])
    osnap = sc.oracle_snapshot()
    status = oracle_plan(osnap, sc.ptr, cand_off, cand_pods, mode=1)["status"]
    assert misleading_on_base(sc, osnap, cand_off, cand_pods, status) >= 2


def test_port_bits_exhausted_through_the_view():
    """The batch's shared host-port bits run out: the view sends the same pods the SINGLE way as the planner."""
    case = C.port_bits_case()
    b = C.Built(case)
    v = view(b.sc, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
    assert [int(x) for x in v["how"]] == [cd.how for cd in case.cands]
    assert not v["fallback"].any()
    osnap = b.sc.oracle_snapshot()
    for c, cd in enumerate(case.cands):
        if cd.how == C.BATCHED:
            assert v["ctx"][c] == cd.ctx and [int(m) for m in v["masks"][c]] == case.expected(c), c
            check_against_oracle(b.sc, osnap, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod, v, b.n_spot, c)
    # alone in its batch a pod outside the encoded set stays BATCHED and is reported as fallback
    pvc = C.N_PORT_PODS
    off, pods, at, m = C.sliced(b, pvc)
    at[1:] = -1
    v = view(b.sc, off, pods, at, m)
    assert list(v["how"]) == [C.BATCHED, C.NONE] and list(v["fallback"]) == [1, 0]


@pytest.mark.parametrize("name,first", [("cpu_last_milli", 1), ("two_pods_merge_on_one_node", 2),
                                        ("hostname_anti_affinity_both_ways", 1)])
def test_a_slice_of_a_larger_candidate_list(name, first):
    """cand_pod_off[0] > 0: node_of_pod is read relative to it."""
    case = next(c for c in CASES if c.name == name)
    b = C.Built(case)
    off, pods, at, m = C.sliced(b, first)
    assert off[0] > 0
    v = view(b.sc, off, pods, at, m)
    for i, c in enumerate(range(first, len(case.cands))):
        cd = case.cands[c]
        assert v["how"][i] == cd.how
        if cd.how == C.BATCHED:
            assert v["ctx"][i] == cd.ctx and [int(x) for x in v["masks"][i]] == case.expected(c), c
