"""sr_explain_pods without a GPU: the interface, the hand-written masks of
tests/explain_cases.py against the oracle's yes / no, the seeds of the random
GPU test, and the encoder's reason tags on synthetic configs (bin/explain_check)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import explain_cases
import explain_ref
from helpers import header_functions
from oracle_lib import load_oracle
from randcluster import rand_scenario
from spotplanner import capi

CASES = explain_cases.cases()
IDS = [c.name for c in CASES]
# (seed, spot nodes) of test_gpu_explain.test_random_clusters
RANDOM = [(102, 12), (105, 17), (104, 25), (103, 33), (102, 40)]
EXPLAIN_CHECK = os.path.join(capi.PKG_ROOT, "bin", "explain_check")


def test_entry_points_exported_and_bound():
    lib = capi.load_planner()
    for name in ("sr_explain_pods", "sr_explain_candidate"):
        assert name in capi.EXPORTED and name in header_functions()
        assert getattr(lib, name).restype is ctypes.c_int32 and getattr(lib, name).argtypes
    assert capi.SR_ABI_VERSION == 11 and lib.sr_abi_version() == 11
    assert capi.SR_WHY_COUNT == 12 == len(capi.WHY_NAMES)
    assert [getattr(capi, "SR_WHY_" + n) for n in capi.WHY_NAMES] == [1 << r for r in range(12)]
    assert ctypes.sizeof(capi.sr_explain_out) == 5 * ctypes.sizeof(ctypes.c_void_p)


def test_null_handles_are_argument_errors():
    lib = capi.load_planner()
    sc = explain_cases.scenario(CASES[0])
    h = sc.product_snapshot()
    try:
        pods = np.array([sc.qidx(0)], np.int32)
        a = np.zeros(12, np.int32)
        out = capi.sr_explain_out(capi.ptr(a, capi.P32), capi.ptr(a, capi.P32), capi.ptr(a, capi.P32), None, None)
        P = capi.ptr(pods, capi.P32)
        bad = capi.SR_ERR_INVALID_ARG
        # no context exists without a GPU: every call below must be refused before the context is looked at
        assert lib.sr_explain_pods(None, h, sc.ptr, P, 1, ctypes.byref(out)) == bad
        assert lib.sr_explain_candidate(None, h, sc.ptr, P, 1, P, 0, ctypes.byref(out)) == bad
        fake = ctypes.c_void_p(1)  # never dereferenced: the other arguments are checked first
        assert lib.sr_explain_pods(fake, None, sc.ptr, P, 1, ctypes.byref(out)) == bad
        assert lib.sr_explain_pods(fake, h, None, P, 1, ctypes.byref(out)) == bad
        assert lib.sr_explain_pods(fake, h, sc.ptr, P, -1, ctypes.byref(out)) == bad
        assert lib.sr_explain_pods(fake, h, sc.ptr, P, 1, None) == bad
        assert lib.sr_explain_pods(fake, h, sc.ptr, None, 1, ctypes.byref(out)) == bad
        for missing in ("feasible", "first", "counts"):
            o = capi.sr_explain_out(capi.ptr(a, capi.P32), capi.ptr(a, capi.P32), capi.ptr(a, capi.P32), None, None)
            setattr(o, missing, None)
            assert lib.sr_explain_pods(fake, h, sc.ptr, P, 1, ctypes.byref(o)) == bad, missing
            assert lib.sr_explain_candidate(fake, h, sc.ptr, P, 1, P, 0, ctypes.byref(o)) == bad, missing
        assert lib.sr_explain_candidate(fake, None, sc.ptr, P, 1, P, 0, ctypes.byref(out)) == bad
        assert lib.sr_explain_candidate(fake, h, sc.ptr, P, 1, None, 0, ctypes.byref(out)) == bad
        for at in (-1, 1):  # at_pod outside [0, n)
            assert lib.sr_explain_candidate(fake, h, sc.ptr, P, 1, P, at, ctypes.byref(out)) == bad
        assert lib.sr_snapshot_fork(h) == capi.SR_OK
        assert lib.sr_explain_candidate(fake, h, sc.ptr, P, 1, P, 0, ctypes.byref(out)) == capi.SR_ERR_STATE
    finally:
        lib.sr_snapshot_destroy(h)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_masks_agree_with_the_oracle_on_feasibility(case):
    sc = explain_cases.scenario(case)
    osnap = sc.oracle_snapshot()
    lib = load_oracle()
    assert lib.oracle_pod_needs_fallback(osnap.h, sc.ptr, sc.qidx(0)) == 0
    assert len(case.masks) == len(case.nodes) <= 8
    got = [lib.oracle_check_predicates(osnap.h, sc.ptr, sc.qidx(0), i) for i in range(len(case.nodes))]
    assert got == [1 if m == 0 else 0 for m in case.masks], case.name
    assert all(0 <= m < 1 << capi.SR_WHY_COUNT for m in case.masks)


def test_cases_cover_every_reason_alone_and_combined():
    from known_answer import cases as known
    names = set(IDS)
    assert {c.name for c in known()} <= names
    alone = {m for c in CASES for m in c.masks if m and m & (m - 1) == 0}
    assert alone == {1 << r for r in range(capi.SR_WHY_COUNT)}, sorted(alone)
    bits = [bin(m).count("1") for c in CASES for m in c.masks]
    assert 2 in bits and 3 in bits
    E = explain_cases
    every = [m for c in CASES for m in c.masks]
    assert E.PODS | E.CPU in every and E.TAINT | E.NODE_AFFINITY | E.PORTS in every
    assert E.UNSCHEDULABLE in every and E.TAINT in every and E.UNSCHEDULABLE | E.TAINT in every
    for name in ("x_zero_request_shortcut", "x_zero_cpu_request_on_overcommitted_node", "x_request_above_every_node",
                 "x_affinity_with_empty_term_list", "x_prefilter_fail"):
        assert name in names


@pytest.mark.parametrize("seed,n_spot", RANDOM)
def test_random_seeds_show_the_twin_groups_on_the_oracle(seed, n_spot):
    """The seeds of the GPU test: without inter-pod terms, the pod count refuses on at most a quarter of
    the nodes, and the oracle alone refuses twins of every group somewhere else."""
    nodes, spot_pods, cands = rand_scenario(seed, n_spot=n_spot, n_cand=6, max_pods=5)
    ref = explain_ref.Reference(nodes, spot_pods, [p for c in cands for p in c])
    assert 12 <= ref.n_spot <= 40 and ref.n >= 8
    assert ref.pods_refusing_share() <= 0.25
    want = 0
    for _, bits in explain_ref.TWIN_GROUPS:
        want |= bits
    assert ref.twin_bits_seen() == want
    assert not ref.fallback.all()
    masks = {ref.resource_mask(i, j) for i in range(ref.n) for j in range(ref.n_spot)}
    assert any(m & explain_ref.CPU for m in masks) and any(m & explain_ref.MEMORY for m in masks)


# what each synthetic config is built to show (csrc/synth/synth.cpp): C1 / C2 plain pods against cpu and memory;
# C3 selectors, required affinity, tolerations against tainted and cordoned pools; C5 host ports; the realistic
# variant GPU requests (SCALAR) and zonal CSI volumes (VOLUMES); the affinity variant hostname anti-affinity
# (INTER_POD) and zone spread constraints (SPREAD)
SYNTH = [
    (1, {}, {"CPU", "MEMORY"}),
    (3, {}, {"UNSCHEDULABLE", "TAINT", "NODE_AFFINITY", "CPU", "MEMORY"}),
    (5, {}, {"PORTS", "CPU", "MEMORY"}),
    (3, {"SR_SYNTH_REALISTIC": "1"}, {"TAINT", "NODE_AFFINITY", "CPU", "MEMORY", "SCALAR", "VOLUMES"}),
    (3, {"SR_SYNTH_AFFINITY": "1"}, {"TAINT", "NODE_AFFINITY", "CPU", "MEMORY", "INTER_POD", "SPREAD"}),
]


@pytest.mark.parametrize("config,env,want", SYNTH, ids=["c1", "c3", "c5", "c3-realistic", "c3-affinity"])
def test_explain_check_on_synthetic_configs(config, env, want):
    assert os.path.exists(EXPLAIN_CHECK), "run __graft_entry__.build()"
    r = subprocess.run([EXPLAIN_CHECK, str(config), "20", "40"], env=dict(os.environ, **env), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    seen = {line.split()[1] for line in r.stdout.splitlines() if line.startswith("reason ")}
    assert want <= seen, (sorted(want - seen), r.stdout)
    assert r.stdout.rstrip().endswith("ok")
