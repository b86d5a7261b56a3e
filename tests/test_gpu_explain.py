"""sr_explain_pods / sr_explain_candidate on the GPU: the hand-written masks of
tests/explain_cases.py, random clusters against the oracle (tests/explain_ref.py),
the row-word and block edges, plans of sr_plan explained pod by pod, a K0-less
tick's stale node section, fallback pods, and planning around an explain call."""
import ctypes
import dataclasses

import numpy as np
import pytest

import explain_cases
import explain_ref
from helpers import Scenario
from known_answer import N, P, used
from oracle_lib import load_oracle
from randcluster import rand_scenario
from spotplanner import capi
from spotplanner.model import Container, Pod, Taint
from spotplanner.rescheduler import PlannerError, explain_arrays, explain_candidate_arrays, plan_arrays
from test_explain_reference import RANDOM
from test_gpu_k2_dispatch import make_checker

pytestmark = pytest.mark.gpu

CASES = explain_cases.cases()
E = explain_cases


def _check_sums(res, i, masks):
    """counts / feasible / first of pod i follow from its masks."""
    masks = np.asarray(masks)
    assert [int(x) for x in res.node_mask[i]] == [int(m) for m in masks]
    for r in range(capi.SR_WHY_COUNT):
        assert res.counts[i][r] == int(np.sum((masks >> r) & 1)), capi.WHY_NAMES[r]
    assert res.feasible[i] == int(np.sum(masks == 0))
    zero = np.flatnonzero(masks == 0)
    assert res.first[i] == (int(zero[0]) if len(zero) else -1)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_hand_written_masks(checker, case):
    sc = explain_cases.scenario(case)
    lib = capi.load_planner()
    h = sc.product_snapshot()
    try:
        pods = np.array([sc.qidx(0)], np.int32)
        res = explain_arrays(checker, h, sc.ptr, pods)
        assert res.fallback[0] == 0
        _check_sums(res, 0, case.masks)
        assert res.reasons(0) == {capi.WHY_NAMES[r]: sum(m >> r & 1 for m in case.masks)
                                  for r in range(capi.SR_WHY_COUNT) if any(m >> r & 1 for m in case.masks)}
        bare = explain_arrays(checker, h, sc.ptr, pods, node_mask=False)  # the same without the per-node masks
        assert bare.node_mask is None
        assert np.array_equal(bare.counts, res.counts) and bare.feasible[0] == res.feasible[0]
        assert bare.first[0] == res.first[0]
        out = np.full(1, -7, np.int32)  # first is sr_find_spot_nodes' answer
        assert lib.sr_find_spot_nodes(checker.handle, h, sc.ptr, capi.ptr(pods, capi.P32), 1, capi.ptr(out, capi.P32),
                                      None) == capi.SR_OK
        assert out[0] == res.first[0]
    finally:
        lib.sr_snapshot_destroy(h)


@pytest.mark.parametrize("seed,n_spot", RANDOM)
def test_random_clusters(checker, seed, n_spot):
    """Every candidate pod of a random cluster in one call: feasibility, fitsRequest's bits and the
    twins' groups against the oracle; no inter-pod, spread or volume bit on inputs without such terms."""
    nodes, spot_pods, cands = rand_scenario(seed, n_spot=n_spot, n_cand=6, max_pods=5)
    ref = explain_ref.Reference(nodes, spot_pods, [p for c in cands for p in c])
    lib = capi.load_planner()
    h = ref.sc.product_snapshot()
    try:
        res = explain_arrays(checker, h, ref.sc.ptr, ref.pod_indices())
    finally:
        lib.sr_snapshot_destroy(h)
    ref.check(res)
    assert not (res.node_mask & (capi.SR_WHY_INTER_POD | capi.SR_WHY_SPREAD | capi.SR_WHY_VOLUMES)).any()


@pytest.mark.parametrize("seed,kw", [(7, dict(anti=0.4)), (8, dict(anti=0.3, aff=0.3)),
                                     (9, dict(anti=0.4, aff=0.2, shared_keys=True))],
                         ids=["anti", "anti_aff", "shared_keys"])
def test_inter_pod_inputs_feasibility(checker, seed, kw):
    """Feasibility against the oracle, and INTER_POD apart from the rest: a twin of the pod without
    terms, labels or a namespace any term selects in passes InterPodAffinity everywhere, so the oracle's
    answer for the twin is "no bit but INTER_POD"."""
    nodes, spot_pods, cands = rand_scenario(seed, n_spot=14, n_cand=6, max_pods=5, valid_selectors=True, **kw)
    pods = [p for c in cands for p in c]
    twins = [dataclasses.replace(p, name=p.name + "-t", namespace="nobody", labels={}, pod_affinity=None,
                                 pod_anti_affinity=None) for p in pods]
    n = len(pods)
    sc = Scenario(nodes, spot_pods, pods + twins)
    lib, ora = capi.load_planner(), load_oracle()
    osnap = sc.oracle_snapshot()
    h = sc.product_snapshot()
    try:
        idx = np.array([sc.qidx(i) for i in range(n)], np.int32)
        res = explain_arrays(checker, h, sc.ptr, idx)
        fb = np.zeros(n, np.uint8)  # the same pods are outside the encoded set for sr_find_spot_nodes
        pos = np.zeros(n, np.int32)
        assert lib.sr_find_spot_nodes(checker.handle, h, sc.ptr, capi.ptr(idx, capi.P32), n, capi.ptr(pos, capi.P32),
                                      capi.ptr(fb, capi.PU8)) == capi.SR_OK
    finally:
        lib.sr_snapshot_destroy(h)
    assert list(res.fallback) == list(fb)
    judged = inter = 0
    for i in range(n):
        if ora.oracle_pod_needs_fallback(osnap.h, sc.ptr, sc.qidx(i)):
            assert res.fallback[i] == 1
        if res.fallback[i]:
            continue
        judged += 1
        assert res.first[i] == pos[i]
        for j in range(len(nodes)):
            m = int(res.node_mask[i][j])
            assert (m == 0) == (ora.oracle_check_predicates(osnap.h, sc.ptr, sc.qidx(i), j) == 1), (pods[i].name, j)
            twin_fits = ora.oracle_check_predicates(osnap.h, sc.ptr, sc.qidx(n + i), j) == 1
            assert (m & ~capi.SR_WHY_INTER_POD == 0) == twin_fits, (pods[i].name, j, hex(m))
            inter += bool(m & capi.SR_WHY_INTER_POD)
        _check_sums(res, i, res.node_mask[i])
    assert judged >= 5 and inter > 0, (judged, inter)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129, 256, 257])
def test_row_word_and_block_edges(checker, n):
    """A refusing node at the last position of pools ending at, before and after a 64-bit row word and
    a 256-node block: no padding node is counted."""
    k = Taint("k", "v", "NoSchedule")
    nodes = [N("n%d" % i, cpu=1000) for i in range(n - 1)] + [N("last", cpu=1000, taints=[k])]
    base = [[] for _ in range(n - 1)] + [[used(cpu=950)]]
    sc = Scenario(nodes, base, [P(cpu=100), P(cpu=0)])
    lib = capi.load_planner()
    h = sc.product_snapshot()
    try:
        res = explain_arrays(checker, h, sc.ptr, np.array([sc.qidx(0), sc.qidx(1)], np.int32))
    finally:
        lib.sr_snapshot_destroy(h)
    assert res.node_mask.shape == (2, n)
    _check_sums(res, 0, [0] * (n - 1) + [E.TAINT | E.CPU])
    _check_sums(res, 1, [0] * (n - 1) + [E.TAINT])
    for i in range(2):
        assert res.feasible[i] + int(np.sum(res.node_mask[i] != 0)) == n
        assert res.feasible[i] == n - 1 and res.counts[i].sum() == (2 if i == 0 else 1)


def _node_states(lib, h, n):
    out = []
    for j in range(n):
        req = np.zeros(3, np.int64)
        k = ctypes.c_int32()
        assert lib.sr_snapshot_node_state(h, j, capi.ptr(req, capi.P64), ctypes.byref(k)) == capi.SR_OK
        out.append((tuple(int(x) for x in req), int(k.value)))
    return out


@pytest.mark.parametrize("seed", [22, 24])
def test_explain_candidate_against_plans(checker, seed):
    nodes, spot_pods, cands = rand_scenario(seed, n_spot=12, n_cand=8, max_pods=6)
    flat = [p for c in cands for p in c]
    sc = Scenario(nodes, spot_pods, flat)
    cand_off = np.zeros(len(cands) + 1, np.int32)
    cand_off[1:] = np.cumsum([len(c) for c in cands])
    cand_pods = np.array([sc.qidx(i) for i in range(len(flat))], np.int32)
    lib, ora = capi.load_planner(), load_oracle()
    osnap = sc.oracle_snapshot()
    h = sc.product_snapshot()
    try:
        plan = plan_arrays(checker, h, sc.ptr, cand_off, cand_pods)
        before = _node_states(lib, h, len(nodes))
        failing = placed = 0
        for c in range(len(cands)):
            st = int(plan.status[c])
            if st == capi.SR_CAND_FALLBACK or st == capi.SR_CAND_EMPTY:
                continue
            pods = cand_pods[cand_off[c]:cand_off[c + 1]]
            mapping = plan.node_of_pod[cand_off[c]:cand_off[c + 1]]
            last = st if st >= 0 else len(pods) - 1
            for k in range(last + 1):
                res = explain_candidate_arrays(checker, h, sc.ptr, pods, mapping, k)
                assert res.fallback[0] == 0
                if k == st:  # the failing pod fits nowhere after the earlier pods were added
                    assert res.feasible[0] == 0 and res.first[0] == -1 and (res.node_mask[0] != 0).all()
                    failing += 1
                else:
                    assert res.first[0] == mapping[k], (c, k)
                    placed += 1
                # the oracle forked and filled the same way
                assert ora.oracle_snapshot_fork(osnap.h) == 0
                for q in range(k):
                    ora.oracle_snapshot_add_pod(osnap.h, sc.ptr, int(pods[q]), int(mapping[q]))
                fits = [ora.oracle_check_predicates(osnap.h, sc.ptr, int(pods[k]), j) for j in range(len(nodes))]
                ora.oracle_snapshot_revert(osnap.h)
                assert [int(m == 0) for m in res.node_mask[0]] == fits, (c, k)
                assert _node_states(lib, h, len(nodes)) == before
        assert failing >= 1 and placed >= 5, (failing, placed)
        # argument errors leave the snapshot alone
        pods = cand_pods[:2]
        for mapping, at in (([-1, 0], 1), ([len(nodes), 0], 1), ([0, 0], 2), ([0, 0], -1)):
            with pytest.raises(PlannerError) as e:
                explain_candidate_arrays(checker, h, sc.ptr, pods, np.array(mapping, np.int32), at)
            assert e.value.status == capi.SR_ERR_INVALID_ARG
            assert _node_states(lib, h, len(nodes)) == before
        assert lib.sr_snapshot_fork(h) == capi.SR_OK  # (still unforked after every call above)
        with pytest.raises(PlannerError) as e:
            explain_candidate_arrays(checker, h, sc.ptr, pods, np.array([0, 0], np.int32), 0)
        assert e.value.status == capi.SR_ERR_STATE
    finally:
        lib.sr_snapshot_destroy(h)


def _steady_scenario(scale=1, extra=()):
    """Eight 1000m nodes, the last four closed by a 950m base pod; three candidates of 600m pods; a
    950m filler.  Filling an open node leaves it the 50m the closed nodes have: no free value appears or
    goes, so no threshold moves and the tick after it needs no K0.
    scale: that many times the nodes and the candidates, the last candidate of every three one pod longer than
    the open nodes are many; extra: further query pods behind the filler (sc.qidx from the filler's index + 1)."""
    nodes = [N("n%d" % i, cpu=1000) for i in range(8 * scale)]
    base = [[] for _ in range(4 * scale)] + [[used(cpu=950, name="b%d" % i)] for i in range(4 * scale)]
    cands = []
    for g in range(scale):
        cands += [[P("c%d-%d" % (3 * g + j, k), cpu=600) for k in range(n)] for j, n in enumerate((1, 2, 4 * scale + 1))]
    flat = [p for c in cands for p in c]
    query = flat + [Pod("filler", containers=[Container(cpu_milli=950)])] + list(extra)
    n_base = sum(len(b) for b in base)
    sc = Scenario(nodes, base, query, stamps=[1000 + i for i in range(n_base + len(query))])
    cand_off = np.zeros(len(cands) + 1, np.int32)
    cand_off[1:] = np.cumsum([len(c) for c in cands])
    cand_pods = np.array([sc.qidx(i) for i in range(len(flat))], np.int32)
    return sc, cand_off, cand_pods, sc.qidx(len(flat))


def test_explain_after_a_k0_less_tick():
    """After a K0-less tick the resident node section is stale; an explain call sees the current values."""
    sc, cand_off, cand_pods, filler = _steady_scenario()
    lib = capi.load_planner()
    ck = make_checker()
    h = sc.product_snapshot()
    try:
        probe = cand_pods[:1]
        for _ in range(2):
            plan_arrays(ck, h, sc.ptr, cand_off, cand_pods)
        res = explain_arrays(ck, h, sc.ptr, probe)
        assert res.first[0] == 0 and res.node_mask[0][0] == 0
        assert lib.sr_snapshot_add_pod(h, sc.ptr, filler, 0) == capi.SR_OK
        k0 = []
        for _ in range(2):
            p = plan_arrays(ck, h, sc.ptr, cand_off, cand_pods)
            k0.append(int(ck.timing().k0_columns))
        print("k0_columns after the fill:", k0)
        assert k0[-1] == -2, k0
        assert p.node_of_pod[0] == 1
        res = explain_arrays(ck, h, sc.ptr, probe)
        assert res.node_mask[0][0] == capi.SR_WHY_CPU and res.first[0] == 1
        _check_sums(res, 0, [E.CPU, 0, 0, 0, E.CPU, E.CPU, E.CPU, E.CPU])
    finally:
        lib.sr_snapshot_destroy(h)
        ck.close()


def test_fallback_pod_among_others(checker):
    nodes = [N("a", cpu=1000), N("b", cpu=1000, taints=[Taint("k", "v", "NoSchedule")]), N("c", cpu=1000)]
    base = [[used(cpu=950)], [], []]
    sc = Scenario(nodes, base, [P("p0", cpu=100), Pod("fb", containers=[Container(cpu_milli=100)], has_pvc=True),
                                P("p2", cpu=0)])
    lib = capi.load_planner()
    h = sc.product_snapshot()
    try:
        res = explain_arrays(checker, h, sc.ptr, np.array([sc.qidx(0), sc.qidx(1), sc.qidx(2)], np.int32))
        alone = explain_arrays(checker, h, sc.ptr, np.array([sc.qidx(0), sc.qidx(2)], np.int32))
    finally:
        lib.sr_snapshot_destroy(h)
    assert list(res.fallback) == [0, 1, 0]
    assert res.feasible[1] == -1 and res.first[1] == -1 and not res.counts[1].any() and not res.node_mask[1].any()
    _check_sums(res, 0, [E.CPU, E.TAINT, 0])
    _check_sums(res, 2, [0, E.TAINT, 0])
    for a, b in ((0, 0), (2, 1)):
        assert np.array_equal(res.node_mask[a], alone.node_mask[b]) and np.array_equal(res.counts[a], alone.counts[b])


def test_plans_around_an_explain_call_are_identical():
    """The third plan of one input on a fresh context, with and without an explain call before it:
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
                res = explain_arrays(ck, h, sc.ptr, cand_pods)
                assert res.first[0] == first.node_of_pod[0] == 0  # (a candidate's first pod meets the base state)
            p = plan_arrays(ck, h, sc.ptr, cand_off, cand_pods)
            t = ck.timing()
            seen.append((list(p.status), list(p.node_of_pod), p.winner, list(p.winner_map), int(t.bytes_uploaded),
                         int(t.enc_reused), int(t.k0_columns)))
            assert list(first.status) == list(p.status) and list(first.node_of_pod) == list(p.node_of_pod)
        finally:
            lib.sr_snapshot_destroy(h)
            ck.close()
    print("third plan without / with an explain call before it:", seen)
    assert seen[0] == seen[1]
    assert seen[0][5] == 1  # a steady prepare: the candidate side was reused
