"""sr_evacuate_plan without a GPU: the interface, the hand cases of tests/evacuate_cases.py against the oracle on
a really reduced snapshot (tests/evacuate_ref.py), and everything but the kernel through the host view
(sr_evacuate_plan_view of lib/libsrexplainview.so: the rule, the staging of a pass and evacuate_scenario, the
statement the kernel follows) and bin/evacuate_check.  The random inputs of test_gpu_evacuate.py are fixed here,
with the conditions that test relies on asserted on the oracle alone."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import evacuate_cases as E
import explain_plan_cases as C
from evacuate_ref import (compacted, first_fit_standing, masked_blockers, n_minus_one, oracle_evacuate,
                          oracle_evacuate_plan, pools, reduced_in_context, reduced_oracle, scenarios)
from helpers import header_functions
from spotplanner import capi
from test_explain_plan_reference import RANDOM, load_view, random_input

CASES = E.cases()
IDS = [c.name for c in CASES]
# Two seeds per kind of test_explain_plan_reference.random_input: the first ones from 0 on which the oracle alone
# finds, among the N-1 and the two-pool scenarios over the cluster's spot nodes, a scenario that strands a pod, a
# scenario with pods that strands none, and a pod whose first fit on the standing snapshot is a node its scenario
# loses (test_random_inputs_show_the_feature); the inter-pod seeds also hold a scenario the rule refuses
SEEDS = {"plain": [0, 1], "inter_pod": [0, 1]}
RUNS = [(kind, seed) for kind in sorted(SEEDS) for seed in SEEDS[kind]]
RUN_IDS = ["%s-%d" % r for r in RUNS]
CHECK_BIN = os.path.join(capi.PKG_ROOT, "bin", "evacuate_check")


def random_scenarios(kind, seed):
    """(scenario, scen_off, scen_pods, lost_off, lost_pos): every spot node lost alone, then the two pools of the
    even and the odd positions; a scenario moves the pods of its lost nodes."""
    sc, _, _ = random_input(seed, RANDOM[kind][0])[:3]
    n_spot = len(sc.spot)
    return (sc,) + scenarios(sc, n_minus_one(n_spot) + pools(n_spot, 2))


def evacuate_view(sc, scen_off, scen_pods, lost_off, lost_pos, counts=True, status=capi.SR_OK, snapshot_cluster=None):
    """sr_evacuate_plan on the host: dict(stranded, first, node_of_pod, counts, how).  `snapshot_cluster`: the
    cluster the snapshot is built from when it is not the call's."""
    lib = load_view()
    PC, VP = ctypes.POINTER(capi.sr_cluster), ctypes.c_void_p
    lib.sr_evacuate_plan_view.argtypes = [PC, VP, ctypes.POINTER(capi.sr_candidates), capi.P32, capi.P32,
                                          ctypes.POINTER(capi.sr_evacuate_out)]
    lib.sr_evacuate_plan_view.restype = ctypes.c_int32
    n, total = len(scen_off) - 1, int(scen_off[-1] - scen_off[0])
    h = ctypes.c_void_p()
    assert lib.sr_snapshot_create(snapshot_cluster or sc.ptr, capi.ptr(sc.spot, capi.P32), len(sc.spot),
                                  capi.ptr(sc.node_pod_off, capi.P32), capi.ptr(sc.node_pod_idx, capi.P32),
                                  ctypes.byref(h)) == capi.SR_OK
    stranded, first = np.full(max(n, 1), 77, np.int32), np.full(max(n, 1), 77, np.int32)
    mapping = np.full(max(total, 1), 77, np.int32)
    cnt = np.full((max(total, 1), capi.SR_WHY_COUNT), 77, np.int32)
    how = np.full(max(n, 1), 77, np.uint8)
    o = capi.sr_evacuate_out(capi.ptr(stranded, capi.P32), capi.ptr(first, capi.P32), capi.ptr(mapping, capi.P32),
                             capi.ptr(cnt, capi.P32) if counts else None, capi.ptr(how, capi.PU8))
    c = capi.sr_candidates(n, capi.ptr(scen_off, capi.P32), capi.ptr(scen_pods, capi.P32), None)
    try:
        st = lib.sr_evacuate_plan_view(sc.ptr, h, ctypes.byref(c), capi.ptr(lost_off, capi.P32),
                                       capi.ptr(lost_pos, capi.P32), ctypes.byref(o))
    finally:
        lib.sr_snapshot_destroy(h)
    assert st == status, st
    return dict(stranded=stranded[:n], first=first[:n], node_of_pod=mapping[:total], counts=cnt[:total] if counts else None,
                how=how[:n])


def test_entry_point_exported_and_bound():
    lib = capi.load_planner()
    assert "sr_evacuate_plan" in capi.EXPORTED and "sr_evacuate_plan" in header_functions()
    assert lib.sr_evacuate_plan.restype is ctypes.c_int32 and len(lib.sr_evacuate_plan.argtypes) == 7
    assert capi.SR_ABI_VERSION == 11 and lib.sr_abi_version() == 11
    assert [f[0] for f in capi.sr_evacuate_out._fields_] == ["stranded", "first", "node_of_pod", "counts", "how"]
    assert (capi.SR_EVAC_JUDGED, capi.SR_EVAC_FALLBACK, capi.SR_EVAC_NOT_PLAIN) == (E.JUDGED, E.FALLBACK, E.NOT_PLAIN)


def test_arguments_are_refused_before_the_context_is_looked_at():
    lib = capi.load_planner()
    b = E.Built(CASES[0])
    sc = b.sc
    h = sc.product_snapshot()
    try:
        n, total = len(b.scen_off) - 1, len(b.scen_pods)
        a, m = np.zeros(n, np.int32), np.zeros(total * 12, np.int32)

        def out():
            return capi.sr_evacuate_out(capi.ptr(a, capi.P32), capi.ptr(a, capi.P32), capi.ptr(m, capi.P32), None, None)
        scen = capi.sr_candidates(n, capi.ptr(b.scen_off, capi.P32), capi.ptr(b.scen_pods, capi.P32), None)
        LO, LP = capi.ptr(b.lost_off, capi.P32), capi.ptr(b.lost_pos, capi.P32)
        o = out()
        bad = capi.SR_ERR_INVALID_ARG
        fake = ctypes.c_void_p(1)  # never dereferenced: no context exists without a GPU
        call = lib.sr_evacuate_plan
        assert call(None, h, sc.ptr, ctypes.byref(scen), LO, LP, ctypes.byref(o)) == bad
        assert call(fake, None, sc.ptr, ctypes.byref(scen), LO, LP, ctypes.byref(o)) == bad
        assert call(fake, h, None, ctypes.byref(scen), LO, LP, ctypes.byref(o)) == bad
        assert call(fake, h, sc.ptr, None, LO, LP, ctypes.byref(o)) == bad
        assert call(fake, h, sc.ptr, ctypes.byref(scen), None, LP, ctypes.byref(o)) == bad
        assert call(fake, h, sc.ptr, ctypes.byref(scen), LO, None, ctypes.byref(o)) == bad
        assert call(fake, h, sc.ptr, ctypes.byref(scen), LO, LP, None) == bad
        for missing in ("stranded", "first", "node_of_pod"):
            o = out()
            setattr(o, missing, None)
            assert call(fake, h, sc.ptr, ctypes.byref(scen), LO, LP, ctypes.byref(o)) == bad
        o = out()
        for value in (sc.enc.a["req_cpu"].shape[0] + 5, -1):  # a pod index out of range
            pods = b.scen_pods.copy()
            pods[1] = value
            s2 = capi.sr_candidates(n, capi.ptr(b.scen_off, capi.P32), capi.ptr(pods, capi.P32), None)
            assert call(fake, h, sc.ptr, ctypes.byref(s2), LO, LP, ctypes.byref(o)) == bad
        for value in (-1, b.n_spot):  # a lost position outside the list
            pos = b.lost_pos.copy()
            pos[0] = value
            assert call(fake, h, sc.ptr, ctypes.byref(scen), LO, capi.ptr(pos, capi.P32), ctypes.byref(o)) == bad
        s = next(i for i, sn in enumerate(b.case.scens) if len(sn.lost) >= 2)  # a position repeated in a scenario
        pos = b.lost_pos.copy()
        pos[b.lost_off[s] + 1] = pos[b.lost_off[s]]
        assert call(fake, h, sc.ptr, ctypes.byref(scen), LO, capi.ptr(pos, capi.P32), ctypes.byref(o)) == bad
        for off in (b.lost_off, b.scen_off):  # a CSR that decreases
            broken = off.copy()
            broken[1], broken[2] = broken[2] + 1, broken[1]
            if off is b.lost_off:
                assert call(fake, h, sc.ptr, ctypes.byref(scen), capi.ptr(broken, capi.P32), LP, ctypes.byref(o)) == bad
            else:
                s2 = capi.sr_candidates(n, capi.ptr(broken, capi.P32), capi.ptr(b.scen_pods, capi.P32), None)
                assert call(fake, h, sc.ptr, ctypes.byref(s2), LO, LP, ctypes.byref(o)) == bad
        none = capi.sr_candidates(0, None, None, None)
        assert call(fake, h, sc.ptr, ctypes.byref(none), None, None, ctypes.byref(o)) == capi.SR_OK
        assert lib.sr_snapshot_fork(h) == capi.SR_OK
        assert call(fake, h, sc.ptr, ctypes.byref(scen), LO, LP, ctypes.byref(o)) == capi.SR_ERR_STATE
    finally:
        lib.sr_snapshot_destroy(h)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hand_cases_against_the_reference(case):
    """The hand answers are the reduced-snapshot oracle's, for the scenarios outside the rule too; where a case says
    so, merely masking the standing snapshot gives another answer."""
    b = E.Built(case)
    osnap = b.sc.oracle_snapshot()
    for s, sn in enumerate(case.scens):
        pods = b.scen_pods[int(b.scen_off[s]):int(b.scen_off[s + 1])]
        ref = oracle_evacuate(b.sc, pods, sn.lost)
        if sn.how == E.FALLBACK:
            assert ref.fallback == 1
            continue
        assert ref.fallback == 0 and ref.node_of_pod == sn.node_of_pod, (s, ref.node_of_pod)
        masked = masked_blockers(b.sc, osnap, pods, sn.lost)
        if sn.how == E.JUDGED:
            assert masked == sn.node_of_pod, (s, masked)
        assert (masked != sn.node_of_pod) == sn.differs, (s, masked)


def check_stranded_rows(sc, scen_off, scen_pods, lost, mapping, counts, s):
    """Every stranded pod of scenario s in its own context, by the reduced oracle forked and filled with the
    compacted list: no surviving node takes it, and fitsRequest's bits add up to the counts row."""
    osnap, keep = reduced_oracle(sc, lost)
    lo, hi = int(scen_off[s] - scen_off[0]), int(scen_off[s + 1] - scen_off[0])
    pods, row = scen_pods[int(scen_off[s]):int(scen_off[s + 1])], mapping[lo:hi]
    for k in range(hi - lo):
        if row[k] >= 0:
            assert not counts[lo + k].any()
            continue
        cp, cm, at = compacted(pods, row, k)
        fits, bits = reduced_in_context(sc, osnap, keep, cp, cm, at)
        assert not any(fits), (s, k)
        for bit in (C.PODS, C.CPU, C.MEMORY, C.EPHEMERAL):
            assert counts[lo + k][bit.bit_length() - 1] == sum(1 for m in bits if m & bit), (s, k, bit)
        # a surviving node refuses for at least one reason, and no other node is counted
        assert counts[lo + k].sum() >= len(keep) and counts[lo + k].max() <= len(keep)
    osnap.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hand_cases_through_the_view(case):
    b = E.Built(case)
    v = evacuate_view(b.sc, b.scen_off, b.scen_pods, b.lost_off, b.lost_pos)
    bare = evacuate_view(b.sc, b.scen_off, b.scen_pods, b.lost_off, b.lost_pos, counts=False)
    assert list(v["how"]) == list(b.how)
    assert list(v["node_of_pod"]) == list(b.node_of_pod)
    assert list(v["stranded"]) == list(b.stranded) and list(v["first"]) == list(b.first)
    for key in ("how", "node_of_pod", "stranded", "first"):
        assert np.array_equal(v[key], bare[key]), key
    for i, row in b.pinned.items():
        assert list(v["counts"][i]) == row, i
    for s, sn in enumerate(case.scens):
        if sn.how == E.JUDGED:
            check_stranded_rows(b.sc, b.scen_off, b.scen_pods, sn.lost, v["node_of_pod"], v["counts"], s)
        else:  # nothing is reported
            assert not v["counts"][int(b.scen_off[s]):int(b.scen_off[s + 1])].any()


def test_cases_cover_the_contract():
    scens = [sn for c in CASES for sn in c.scens]
    assert {sn.how for sn in scens} == {E.JUDGED, E.FALLBACK, E.NOT_PLAIN}
    assert any(sn.lost == [] and sn.pods for sn in scens) and any(not sn.pods for sn in scens)
    assert any(len(sn.lost) == len(c.nodes) and sn.pods for c in CASES for sn in c.scens)
    assert any(sn.stranded == 0 and sn.pods for sn in scens)
    assert any(0 < sn.first < len(sn.pods) - 1 or (sn.first == 0 and sn.node_of_pod[-1] >= 0) for sn in scens)
    # one case per clause of the rule, and in four of them the standing snapshot really misleads
    assert sum(1 for c in CASES if any(sn.how == E.NOT_PLAIN for sn in c.scens)) == 7
    assert sum(1 for sn in scens if sn.differs) == 4


def test_evacuate_check_passes():
    if not os.path.exists(CHECK_BIN):  # host only: builds without a GPU, like the oracle
        subprocess.run(["make", "-C", capi.PKG_ROOT, "bin/evacuate_check"], check=True, capture_output=True)
    r = subprocess.run([CHECK_BIN], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert r.stdout.strip().endswith("ok") and "RESULTS DIFFER" not in r.stdout and "LAYOUT WRONG" not in r.stdout


def test_the_rule_has_no_pod_limit():
    """300 pods, past SR_BLOCKERS_BATCH_PODS: one scenario, judged, against the reduced oracle."""
    from helpers import Scenario
    from known_answer import P
    n = 300
    assert n > capi.SR_BLOCKERS_BATCH_PODS
    nodes = C.pool(4, cpu=1000)
    pods = [P("p%d" % k, cpu=1) for k in range(n)]
    pods[n // 2] = P("big", cpu=1001)
    sc = Scenario(nodes, [[] for _ in nodes], pods)
    args = scenarios(sc, [[0]], moved=[[sc.qidx(i) for i in range(n)]])
    v = evacuate_view(sc, *args)
    ref = oracle_evacuate_plan(sc, *args)
    assert list(v["how"]) == [E.JUDGED] and list(v["stranded"]) == [1] and list(v["first"]) == [n // 2]
    assert np.array_equal(v["node_of_pod"], ref["node_of_pod"])
    # 110 pods fill node 1, 110 node 2, the rest goes to node 3; the big pod met cpu on all three and the pod count
    # on node 1
    assert list(v["counts"][n // 2]) == E.why_row({C.CPU: 3, C.PODS: 1})
    assert sorted(set(int(j) for j in v["node_of_pod"])) == [-1, 1, 2, 3]


def unknown_scalars_input():
    """Three nodes, a pod on node 0 and one on node 1, and the cluster a snapshot is built from when the caller
    passed no scalar tables while node 0's pod is flagged as carrying scalar requests: its usage is unknown.
    Returns (scenario, that cluster struct, the call's arrays): node 0 lost, node 1 lost, each moving its pod."""
    from helpers import Scenario
    from known_answer import P
    sc = Scenario(C.pool(3), [[P("g", cpu=10)], [P("w", cpu=10)], []], [])
    A = dict(sc.enc.a)
    for key in ("pod_scalar_off", "pod_scalar_name", "pod_scalar_req", "pod_scalar_acc", "node_scalar_off",
                "node_scalar_name", "node_scalar_alloc"):
        A[key] = None
    A["flags"] = sc.enc.a["flags"].copy()
    A["flags"][0] |= capi.SR_POD_FB_SCALAR_RESOURCES
    return sc, capi.make_cluster_struct(A), scenarios(sc, [[0], [1]])


def test_a_pod_of_unknown_scalars_on_the_lost_node_is_not_plain():
    """The clause beside required anti-affinity: with that pod in the snapshot every pod with scalars goes to the
    fallback, without it none does, so the standing snapshot may not speak for the reduced one."""
    sc, bare, args = unknown_scalars_input()
    v = evacuate_view(sc, *args, snapshot_cluster=ctypes.byref(bare))
    assert list(v["how"]) == [E.NOT_PLAIN, E.JUDGED]
    assert list(v["stranded"]) == [-1, 0] and list(v["node_of_pod"]) == [-1, 0]
    # built from the call's own cluster the pod's scalars are known (it has none): both scenarios are judged
    assert list(evacuate_view(sc, *args)["how"]) == [E.JUDGED, E.JUDGED]


def test_negative_accounting_is_not_plain():
    """A pod whose accounted request is negative leaves the arithmetic the deltas rely on."""
    from helpers import Scenario
    from known_answer import P
    sc = Scenario(C.pool(3), [[], [], []], [P("a0", cpu=100), P("a1", cpu=100)])
    args = scenarios(sc, [[0], [0]], moved=[[sc.qidx(0), sc.qidx(1)], [sc.qidx(1)]])
    assert list(evacuate_view(sc, *args)["how"]) == [E.JUDGED, E.JUDGED]
    assert sc.enc.a["acc_cpu"] is not None
    sc.enc.a["acc_cpu"][sc.qidx(0)] = -1  # (the cluster struct points at this array)
    v = evacuate_view(sc, *args)
    assert list(v["how"]) == [E.NOT_PLAIN, E.JUDGED]
    assert list(v["stranded"]) == [-1, 0] and list(v["node_of_pod"]) == [-1, -1, 1]


@pytest.mark.parametrize("kind,seed", RUNS, ids=RUN_IDS)
def test_random_inputs_show_the_feature(kind, seed):
    """On the oracle alone: what the GPU test relies on."""
    sc, scen_off, scen_pods, lost_off, lost_pos = random_scenarios(kind, seed)
    ref = oracle_evacuate_plan(sc, scen_off, scen_pods, lost_off, lost_pos)
    n = len(scen_off) - 1
    sizes = scen_off[1:] - scen_off[:-1]
    judged = ref["fallback"] == 0
    assert ((ref["stranded"] > 0) & judged).any()
    assert ((ref["stranded"] == 0) & judged & (sizes > 0)).any()
    osnap = sc.oracle_snapshot()
    moved_on = 0
    for s in range(n):
        lost = set(int(j) for j in lost_pos[int(lost_off[s]):int(lost_off[s + 1])])
        for p in scen_pods[int(scen_off[s]):int(scen_off[s + 1])]:
            moved_on += first_fit_standing(sc, osnap, p) in lost
    assert moved_on >= 1


@pytest.mark.parametrize("kind,seed", RUNS, ids=RUN_IDS)
def test_random_clusters_through_the_view(kind, seed):
    sc, scen_off, scen_pods, lost_off, lost_pos = random_scenarios(kind, seed)
    v = evacuate_view(sc, scen_off, scen_pods, lost_off, lost_pos)
    ref = oracle_evacuate_plan(sc, scen_off, scen_pods, lost_off, lost_pos)
    n = len(scen_off) - 1
    how = v["how"]
    assert (how == E.JUDGED).any()
    if kind == "inter_pod":
        assert (how == E.NOT_PLAIN).any()
    for s in range(n):
        lo, hi = int(scen_off[s]), int(scen_off[s + 1])
        if how[s] == E.JUDGED:
            assert ref["fallback"][s] == 0
            assert v["stranded"][s] == ref["stranded"][s] and v["first"][s] == ref["first"][s], s
            assert np.array_equal(v["node_of_pod"][lo:hi], ref["node_of_pod"][lo:hi]), s
            lost = lost_pos[int(lost_off[s]):int(lost_off[s + 1])]
            if v["stranded"][s] > 0:
                check_stranded_rows(sc, scen_off, scen_pods, lost, v["node_of_pod"], v["counts"], s)
        else:
            assert how[s] in (E.NOT_PLAIN, E.FALLBACK)
            if how[s] == E.FALLBACK:
                assert ref["fallback"][s] == 1
            assert v["stranded"][s] == -1 and v["first"][s] == -1
            assert (v["node_of_pod"][lo:hi] == -1).all() and not v["counts"][lo:hi].any()
