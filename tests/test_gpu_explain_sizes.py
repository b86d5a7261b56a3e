"""sr_explain_pods / sr_explain_candidate beyond one block, bit-exact against
the formulas and hand-written masks of explain_sizes.py (proved on the oracle
by test_explain_sizes_reference.py): every reason at every row word, wave and
block position of pools of 320, 1,100 and 4,300 nodes; the first feasible node
in a late wave and block, and the earlier of two blocks; 300 pods of 300
classes in one call, in another order than the cluster's, with fallback pods in
between; 65,537 entries across the gridDim.y split; the explain buffers reused
on one context across pools of different sizes; and candidates whose earlier
pods decide the later pod's mask.  No result is compared with another call of
the code under test."""
import contextlib
import time

import numpy as np
import pytest

import explain_sizes as X
from spotplanner import capi
from spotplanner.rescheduler import explain_arrays, explain_candidate_arrays
from test_gpu_explain import _node_states
from test_gpu_k2_dispatch import make_checker

pytestmark = pytest.mark.gpu


def check_rows(res, want, fallback=None):
    """node_mask equals `want` ([pods][nodes]) in one comparison; counts, feasible and first follow from it;
    a fallback row reads -1 / -1 and zeros."""
    want = np.asarray(want, np.uint16)
    fallback = np.zeros(len(want), bool) if fallback is None else np.asarray(fallback, bool)
    assert np.array_equal(res.fallback, fallback.astype(np.uint8))
    if res.node_mask is not None:
        assert res.node_mask.shape == want.shape
        assert np.array_equal(res.node_mask, want), np.argwhere(res.node_mask != want)[:8]
    counts = np.stack([((want >> r) & 1).sum(1) for r in range(capi.SR_WHY_COUNT)], 1)
    assert np.array_equal(res.counts, counts), np.argwhere(res.counts != counts)[:8]
    ok = want == 0
    feasible = np.where(fallback, -1, ok.sum(1))
    first = np.where(fallback | ~ok.any(1), -1, ok.argmax(1))
    assert np.array_equal(res.feasible, feasible), np.flatnonzero(res.feasible != feasible)[:8]
    assert np.array_equal(res.first, first), np.flatnonzero(res.first != first)[:8]


@contextlib.contextmanager
def snapshot(sc):
    h = sc.product_snapshot()
    try:
        yield h
    finally:
        capi.load_planner().sr_snapshot_destroy(h)


def explain_pool(ck, pool, pods, want, fallback=None, masks=(True, False), h=None):
    """One call with the per-node masks and one without, each against `want`; returns the last result."""
    pods = np.asarray(pods, np.int32)
    with contextlib.ExitStack() as stack:
        h = h or stack.enter_context(snapshot(pool.sc))
        for on in masks:
            res = explain_arrays(ck, h, pool.sc.ptr, pods, node_mask=on)
            assert (res.node_mask is not None) == on
            check_rows(res, want, fallback)
    return res


@pytest.mark.parametrize("n", X.SIZES)
def test_formula_pools(checker, n):
    pool = X.get_pool(n)
    want = X.formula_masks(n)[None, :]
    assert (want[0, 64:] != 0).any() and want[0, 0] != 0
    explain_pool(checker, pool, [pool.full], want)


@pytest.mark.parametrize("n", [1100, 4300])
def test_first_feasible_in_a_late_wave_and_block(checker, n):
    """All eight sets in one call: first is the maximum of n_pad - position over the waves of a block and over
    the blocks; sr_find_spot_nodes answers the same."""
    pool = X.get_pool(n)
    lib = capi.load_planner()
    want = np.array([[X.first_mask(n, s, j) for j in range(n)] for s in range(len(X.FIRST_SETS))], np.uint16)
    pods = np.array(pool.firsts, np.int32)
    hand = X.first_want(n)
    with snapshot(pool.sc) as h:
        res = explain_pool(checker, pool, pods, want, masks=(False, True), h=h)
        assert [int(x) for x in res.first] == [f for f, _ in hand]
        assert [int(x) for x in res.feasible] == [k for _, k in hand]
        pos = np.full(len(pods), -7, np.int32)
        assert lib.sr_find_spot_nodes(checker.handle, h, pool.sc.ptr, capi.ptr(pods, capi.P32), len(pods),
                                      capi.ptr(pos, capi.P32), None) == capi.SR_OK
        assert [int(x) for x in pos] == [f for f, _ in hand]


def test_many_pods_many_classes(checker):
    """300 entries in the caller's order: a program per class, results scattered back from the encoded order,
    fallback rows empty and their neighbours as the formulas say."""
    pool = X.get_pool(X.MANY_N, many=True)
    pods = [pool.many[i] for i in X.MANY_ORDER]
    fallback = [X.many_fallback(i) for i in X.MANY_ORDER]
    want = X.many_masks()
    assert want.shape == (300, 1100) and 40 <= sum(fallback) <= 45
    assert not want[np.array(fallback)].any() and len({row.tobytes() for row in want}) > 250
    res = explain_pool(checker, pool, pods, want, fallback)
    for k in np.flatnonzero(fallback):
        assert res.feasible[k] == res.first[k] == -1 and not res.counts[k].any()


def test_entries_across_the_grid_split(checker):
    """65,537 entries cycling through three pods: launch_explain's second launch starts at entry 65,535."""
    sc = X.split_pool()
    n = X.SPLIT_ENTRIES
    pods = np.array([sc.qidx(k % 3) for k in range(n)], np.int32)
    want = np.array(X.SPLIT_MASKS, np.uint16)[np.arange(n) % 3]
    with snapshot(sc) as h:
        t0 = time.perf_counter()
        res = explain_arrays(checker, h, sc.ptr, pods)
        print("sr_explain_pods of %d entries: %.3f s" % (n, time.perf_counter() - t0))
        bare = explain_arrays(checker, h, sc.ptr, pods, node_mask=False)
    check_rows(res, want)
    check_rows(bare, want)
    assert [list(r) for r in res.node_mask[65534:]] == [X.SPLIT_MASKS[65534 % 3], X.SPLIT_MASKS[0], X.SPLIT_MASKS[1]]
    assert [int(x) for x in res.first[65534:]] == [1, 2, 0]


def test_buffers_reused_across_sizes():
    """One fresh context: the 4,300 pool, a 65-node pool, the 4,300 pool again without and with masks, the 320
    pool.  x_in / x_out only grow and the explain encoder keeps a view of the pool: every result is still its own
    pool's formula."""
    ck = make_checker()
    try:
        big, small = X.get_pool(4300), X.get_pool(320)
        wbig, wsmall = X.formula_masks(4300)[None, :], X.formula_masks(320)[None, :]
        explain_pool(ck, big, [big.full], wbig, masks=(True,))
        sc, m100, m0 = X.edge_pool(65)
        with snapshot(sc) as h:
            check_rows(explain_arrays(ck, h, sc.ptr, np.array([sc.qidx(0), sc.qidx(1)], np.int32)), [m100, m0])
        explain_pool(ck, big, [big.full], wbig, masks=(False, True))
        explain_pool(ck, small, [small.full], wsmall, masks=(True, False))
    finally:
        ck.close()


CAND = X.cand_cases()


@pytest.mark.parametrize("case", CAND, ids=[c.name for c in CAND])
def test_earlier_pod_of_the_candidate_decides(checker, case):
    sc = X.cand_scenario(case)
    lib = capi.load_planner()
    n, k = len(case.nodes), len(case.pods) - 1
    pods = np.array([sc.qidx(q) for q in range(k + 1)], np.int32)
    mapping = np.array(case.mapping + [-1], np.int32)
    h = sc.product_snapshot()
    try:
        before = _node_states(lib, h, n)
        res = explain_candidate_arrays(checker, h, sc.ptr, pods, mapping, k)
        check_rows(res, [case.with_])
        assert _node_states(lib, h, n) == before
        bare = explain_candidate_arrays(checker, h, sc.ptr, pods, mapping, k, node_mask=False)
        check_rows(bare, [case.with_])
        alone = explain_arrays(checker, h, sc.ptr, pods[k:])  # without the earlier pods
        check_rows(alone, [case.without])
        assert _node_states(lib, h, n) == before
        if k == 2:  # the middle pod sees the first one only
            mid = explain_candidate_arrays(checker, h, sc.ptr, pods, mapping, 1)
            assert mid.fallback[0] == 0 and mid.node_mask[0][case.mapping[1]] == 0
    finally:
        lib.sr_snapshot_destroy(h)
