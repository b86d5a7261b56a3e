"""sr_blockers_plan without a GPU: the interface, the hand cases of tests/blockers_cases.py against the
contract's loop over the oracle (tests/blockers_ref.py), and everything but the kernel through the host view
(sr_blockers_plan_view of lib/libsrexplainview.so: the ways, the staging of the batched pass and
blockers_candidate, the statement the kernel follows) and bin/blockers_check.  The random inputs of
test_gpu_blockers.py are fixed here, with the conditions that test relies on asserted on the oracle alone."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import blockers_cases as B
import explain_plan_cases as C
from blockers_ref import compacted, oracle_blockers_plan
from helpers import Scenario, header_functions
from known_answer import P
from oracle_lib import oracle_plan
from spotplanner import capi
from test_explain_plan_reference import RANDOM, load_view, random_input

CASES = B.cases()
IDS = [c.name for c in CASES]
# Three seeds per kind of test_explain_plan_reference.random_input: the first ones from 0 on which the oracle
# finds a candidate with two or more blockers, one with a pod placed behind a blocker, and among the candidates
# that stop at a pod k > 0 one that is plain as a whole and one that is not (test_random_inputs_show_the_feature)
# (inter-pod seed 0 has no plain candidate among those that stop at k > 0)
SEEDS = {"plain": [0, 1, 2], "inter_pod": [1, 2, 3]}
RUNS = [(kind, seed) for kind in sorted(SEEDS) for seed in SEEDS[kind]]
RUN_IDS = ["%s-%d" % r for r in RUNS]
CHECK_BIN = os.path.join(capi.PKG_ROOT, "bin", "blockers_check")


def blockers_view(sc, cand_off, cand_pods, ask, counts=True):
    """sr_blockers_plan on the host: dict(blockers, first, node_of_pod, counts, fallback, how)."""
    lib = load_view()
    PC, VP = ctypes.POINTER(capi.sr_cluster), ctypes.c_void_p
    lib.sr_blockers_plan_view.argtypes = [PC, VP, ctypes.POINTER(capi.sr_candidates), capi.P32,
                                          ctypes.POINTER(capi.sr_blockers_out), capi.PU8]
    lib.sr_blockers_plan_view.restype = ctypes.c_int32
    n, total = len(cand_off) - 1, int(cand_off[-1] - cand_off[0])
    h = ctypes.c_void_p()
    assert lib.sr_snapshot_create(sc.ptr, capi.ptr(sc.spot, capi.P32), len(sc.spot), capi.ptr(sc.node_pod_off, capi.P32),
                                  capi.ptr(sc.node_pod_idx, capi.P32), ctypes.byref(h)) == capi.SR_OK
    blockers, first = np.full(max(n, 1), 77, np.int32), np.full(max(n, 1), 77, np.int32)
    mapping = np.full(max(total, 1), 77, np.int32)
    cnt = np.full((max(total, 1), capi.SR_WHY_COUNT), 77, np.int32)
    fb, how = np.full(max(n, 1), 77, np.uint8), np.zeros(max(n, 1), np.uint8)
    o = capi.sr_blockers_out(capi.ptr(blockers, capi.P32), capi.ptr(first, capi.P32), capi.ptr(mapping, capi.P32),
                             capi.ptr(cnt, capi.P32) if counts else None, capi.ptr(fb, capi.PU8))
    c = capi.sr_candidates(n, capi.ptr(cand_off, capi.P32), capi.ptr(cand_pods, capi.P32), None)
    try:
        st = lib.sr_blockers_plan_view(sc.ptr, h, ctypes.byref(c), capi.ptr(ask, capi.P32), ctypes.byref(o),
                                       capi.ptr(how, capi.PU8))
    finally:
        lib.sr_snapshot_destroy(h)
    assert st == capi.SR_OK, st
    return dict(blockers=blockers[:n], first=first[:n], node_of_pod=mapping[:total], counts=cnt[:total] if counts else None,
                fallback=fb[:n], how=how[:n])


def test_entry_point_exported_and_bound():
    lib = capi.load_planner()
    assert "sr_blockers_plan" in capi.EXPORTED and "sr_blockers_plan" in header_functions()
    assert lib.sr_blockers_plan.restype is ctypes.c_int32 and len(lib.sr_blockers_plan.argtypes) == 7
    assert capi.SR_ABI_VERSION == 11 and lib.sr_abi_version() == 11
    assert [f[0] for f in capi.sr_blockers_out._fields_] == ["blockers", "first", "node_of_pod", "counts", "fallback"]
    assert capi.SR_BLOCKERS_BATCH_PODS == 256


def test_null_arguments_are_refused_before_the_context_is_looked_at():
    lib = capi.load_planner()
    b = B.Built(CASES[0])
    sc = b.sc
    h = sc.product_snapshot()
    try:
        n, total = len(b.cand_off) - 1, len(b.cand_pods)
        a, m = np.zeros(n, np.int32), np.zeros(total * 12, np.int32)
        how = np.zeros(n, np.uint8)

        def out():
            return capi.sr_blockers_out(capi.ptr(a, capi.P32), capi.ptr(a, capi.P32), capi.ptr(m, capi.P32), None, None)
        cands = capi.sr_candidates(n, capi.ptr(b.cand_off, capi.P32), capi.ptr(b.cand_pods, capi.P32), None)
        ASK, HOW = capi.ptr(b.ask, capi.P32), capi.ptr(how, capi.PU8)
        o = out()
        bad = capi.SR_ERR_INVALID_ARG
        fake = ctypes.c_void_p(1)  # never dereferenced: no context exists without a GPU
        assert lib.sr_blockers_plan(None, h, sc.ptr, ctypes.byref(cands), ASK, ctypes.byref(o), HOW) == bad
        assert lib.sr_blockers_plan(fake, None, sc.ptr, ctypes.byref(cands), ASK, ctypes.byref(o), HOW) == bad
        assert lib.sr_blockers_plan(fake, h, None, ctypes.byref(cands), ASK, ctypes.byref(o), HOW) == bad
        assert lib.sr_blockers_plan(fake, h, sc.ptr, None, ASK, ctypes.byref(o), HOW) == bad
        assert lib.sr_blockers_plan(fake, h, sc.ptr, ctypes.byref(cands), None, ctypes.byref(o), HOW) == bad
        assert lib.sr_blockers_plan(fake, h, sc.ptr, ctypes.byref(cands), ASK, None, HOW) == bad
        for missing in ("blockers", "first", "node_of_pod"):
            o = out()
            setattr(o, missing, None)
            assert lib.sr_blockers_plan(fake, h, sc.ptr, ctypes.byref(cands), ASK, ctypes.byref(o), HOW) == bad
        o = out()
        for value in (sc.enc.a["req_cpu"].shape[0] + 5, -1):  # a pod index out of range
            pods = b.cand_pods.copy()
            pods[1] = value
            c2 = capi.sr_candidates(n, capi.ptr(b.cand_off, capi.P32), capi.ptr(pods, capi.P32), None)
            assert lib.sr_blockers_plan(fake, h, sc.ptr, ctypes.byref(c2), ASK, ctypes.byref(o), HOW) == bad
        none = capi.sr_candidates(0, None, None, None)
        assert lib.sr_blockers_plan(fake, h, sc.ptr, ctypes.byref(none), None, ctypes.byref(o), None) == capi.SR_OK
        assert lib.sr_snapshot_fork(h) == capi.SR_OK
        assert lib.sr_blockers_plan(fake, h, sc.ptr, ctypes.byref(cands), ASK, ctypes.byref(o), HOW) == capi.SR_ERR_STATE
    finally:
        lib.sr_snapshot_destroy(h)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hand_cases_against_the_reference(case):
    b = B.Built(case)
    ref = oracle_blockers_plan(b.sc, b.sc.oracle_snapshot(), b.cand_off, b.cand_pods, b.ask, b.n_spot)
    assert list(ref["node_of_pod"]) == list(b.node_of_pod)
    assert list(ref["blockers"]) == list(b.blockers) and list(ref["first"]) == list(b.first)
    assert list(ref["fallback"]) == list(b.fallback)


def check_blocker_rows(sc, osnap, cand_off, cand_pods, mapping, counts, n_spot, c):
    """Every blocker of candidate c in its own context, by the oracle forked and filled with the compacted list:
    no node takes it, and fitsRequest's bits add up to the counts row."""
    lo, hi = int(cand_off[c] - cand_off[0]), int(cand_off[c + 1] - cand_off[0])
    pods, row = cand_pods[int(cand_off[c]):int(cand_off[c + 1])], mapping[lo:hi]
    for k in range(hi - lo):
        if row[k] >= 0:
            assert not counts[lo + k].any()
            continue
        cp, cm, at = compacted(pods, row, k)
        fits, bits = C.oracle_in_context(sc, osnap, cp, cm, at, n_spot)
        assert not any(fits), (c, k)
        for bit in (C.PODS, C.CPU, C.MEMORY, C.EPHEMERAL):
            assert counts[lo + k][bit.bit_length() - 1] == sum(1 for m in bits if m & bit), (c, k, bit)
        # a node refuses for at least one reason: the row covers the pool
        assert counts[lo + k].sum() >= n_spot


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hand_cases_through_the_view(case):
    b = B.Built(case)
    v = blockers_view(b.sc, b.cand_off, b.cand_pods, b.ask)
    bare = blockers_view(b.sc, b.cand_off, b.cand_pods, b.ask, counts=False)
    assert list(v["how"]) == list(b.how)
    assert list(v["node_of_pod"]) == list(b.node_of_pod)
    assert list(v["blockers"]) == list(b.blockers) and list(v["first"]) == list(b.first)
    assert list(v["fallback"]) == list(b.fallback)
    for key in ("how", "node_of_pod", "blockers", "first", "fallback"):
        assert np.array_equal(v[key], bare[key]), key
    for i, row in b.pinned.items():
        assert list(v["counts"][i]) == row, i
    osnap = b.sc.oracle_snapshot()
    for c, cd in enumerate(case.cands):
        if cd.blockers >= 0:
            check_blocker_rows(b.sc, osnap, b.cand_off, b.cand_pods, v["node_of_pod"], v["counts"], b.n_spot, c)
        else:
            assert not v["counts"][int(b.cand_off[c]):int(b.cand_off[c + 1])].any()


def test_cases_cover_the_contract():
    cands = [cd for c in CASES for cd in c.cands]
    assert {cd.how for cd in cands} == {B.NONE, B.BATCHED, B.SINGLE}
    assert any(cd.first == 0 and cd.blockers == 1 for cd in cands)
    assert any(0 < cd.first < len(cd.pods) - 1 for cd in cands)
    assert any(cd.first == len(cd.pods) - 1 and cd.first > 0 for cd in cands)
    assert any(cd.blockers == len(cd.pods) >= 3 for cd in cands)
    assert any(cd.blockers == 0 and cd.pods for cd in cands) and any(cd.fallback for cd in cands)
    assert sum(1 for c in CASES if any(cd.how == B.SINGLE for cd in c.cands)) == 5
    two = [cd for cd in cands if cd.blockers >= 2 and cd.node_of_pod[-1] >= 0]
    assert two  # a pod placed behind the second blocker


def test_blockers_check_passes():
    if not os.path.exists(CHECK_BIN):  # host only: builds without a GPU, like the oracle
        subprocess.run(["make", "-C", capi.PKG_ROOT, "bin/blockers_check"], check=True, capture_output=True)
    r = subprocess.run([CHECK_BIN], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert r.stdout.strip().endswith("ok") and "RESULTS DIFFER" not in r.stdout and "LAYOUT WRONG" not in r.stdout


def capacity_input(extra):
    """One node that takes everything; candidates of capacity and capacity + `extra` 1m pods, each with a
    blocker in the middle."""
    cap = capi.SR_BLOCKERS_BATCH_PODS
    nodes = C.pool(3, cpu=1000)
    cands = []
    for n in (cap, cap + extra):
        pods = [P("p%d_%d" % (n, k), cpu=1) for k in range(n)]
        pods[n // 2] = P("big%d" % n, cpu=1001)
        cands.append(pods)
    flat = [p for c in cands for p in c]
    sc = Scenario(nodes, [[] for _ in nodes], flat)
    cand_off = np.array([0, len(cands[0]), len(flat)], np.int32)
    cand_pods = np.array([sc.qidx(i) for i in range(len(flat))], np.int32)
    return sc, cand_off, cand_pods


def test_the_rule_at_the_context_capacity():
    sc, cand_off, cand_pods = capacity_input(1)
    ask = np.zeros(2, np.int32)
    v = blockers_view(sc, cand_off, cand_pods, ask)
    assert list(v["how"]) == [B.BATCHED, B.SINGLE]
    ref = oracle_blockers_plan(sc, sc.oracle_snapshot(), cand_off, cand_pods, ask, 3)
    assert np.array_equal(v["node_of_pod"], ref["node_of_pod"]) and list(v["blockers"]) == [1, 1]
    cap = capi.SR_BLOCKERS_BATCH_PODS
    assert list(v["first"]) == [cap // 2, (cap + 1) // 2]
    # the 1001m pod meets cpu on all three nodes and the pod count on node 0, which the 110 pods before it filled
    row = B.why_row({C.CPU: 3, C.PODS: 1})
    assert list(v["counts"][cap // 2]) == row and list(v["counts"][cap + (cap + 1) // 2]) == row


def stops_later(status):
    return [c for c in range(len(status)) if status[c] > 0]


@pytest.mark.parametrize("kind,seed", RUNS, ids=RUN_IDS)
def test_random_inputs_show_the_feature(kind, seed):
    """On the oracle alone (and the rule, which reads the tables alone): what the GPU test relies on."""
    sc, cand_off, cand_pods = random_input(seed, RANDOM[kind][0])
    osnap = sc.oracle_snapshot()
    status = np.ascontiguousarray(oracle_plan(osnap, sc.ptr, cand_off, cand_pods, mode=1)["status"], np.int32)
    ref = oracle_blockers_plan(sc, osnap, cand_off, cand_pods, status, len(sc.spot))
    assert (ref["blockers"] >= 2).any()
    behind = 0
    for c in range(len(status)):
        row = ref["node_of_pod"][int(cand_off[c]):int(cand_off[c + 1])]
        if ref["blockers"][c] > 0:
            assert ref["first"][c] == status[c]
            behind += int((row[int(ref["first"][c]):] >= 0).any())
    assert behind >= 1
    how = blockers_view(sc, cand_off, cand_pods, status)["how"]
    later = stops_later(status)
    assert any(how[c] == B.BATCHED for c in later) and any(how[c] == B.SINGLE for c in later)


@pytest.mark.parametrize("kind,seed", RUNS, ids=RUN_IDS)
def test_random_clusters_through_the_view(kind, seed):
    sc, cand_off, cand_pods = random_input(seed, RANDOM[kind][0])
    osnap = sc.oracle_snapshot()
    plan = oracle_plan(osnap, sc.ptr, cand_off, cand_pods, mode=1)
    status = np.ascontiguousarray(plan["status"], np.int32)
    n_spot = len(sc.spot)
    v = blockers_view(sc, cand_off, cand_pods, status)
    ref = oracle_blockers_plan(sc, osnap, cand_off, cand_pods, status, n_spot)
    for key in ("blockers", "first", "node_of_pod", "fallback"):
        assert np.array_equal(v[key], ref[key]), key
    for c in range(len(status)):
        lo, hi = int(cand_off[c]), int(cand_off[c + 1])
        if status[c] < 0:
            assert v["how"][c] == B.NONE and v["blockers"][c] == -1 and not v["counts"][lo:hi].any()
            continue
        assert v["first"][c] == status[c]
        k = int(status[c])
        assert np.array_equal(v["node_of_pod"][lo:lo + k], plan["node_of_pod"][lo:lo + k])
        check_blocker_rows(sc, osnap, cand_off, cand_pods, v["node_of_pod"], v["counts"], n_spot, c)
    # asked for the candidates the plan drained: no blocker, the plan's mapping
    ok = np.where(status == capi.SR_CAND_OK, 0, -1).astype(np.int32)
    d = blockers_view(sc, cand_off, cand_pods, ok)
    for c in range(len(status)):
        if ok[c] == 0:
            lo, hi = int(cand_off[c]), int(cand_off[c + 1])
            assert d["blockers"][c] == 0 and d["first"][c] == -1
            assert np.array_equal(d["node_of_pod"][lo:hi], plan["node_of_pod"][lo:hi])
