"""sr_explain_plan beyond one block, bit-exact against the rule-derived masks
of explain_plan_sizes.py (proved on the host view and the oracle by
test_explain_plan_sizes_reference.py): contexts on every row word of pools of
320, 1,100 and 4,300 nodes; the first feasible node decided by the context in a
late wave and block; 300 classes in the caller's order with a context of its
own each and PVC pods in between; 65,537 candidates across the gridDim.y split;
the explain buffers shared with sr_explain_pods across sizes on one context;
and the limits of the plain-context rule.  Every call runs with the per-node
masks and without; the per-candidate loop (sr_explain_candidate) is asked
beside it where the module says so (Input.loop)."""
import time

import numpy as np
import pytest

import explain_plan_cases as C
import explain_plan_sizes as S
import explain_sizes as X
from spotplanner import capi
from spotplanner.rescheduler import PlannerError, explain_arrays, explain_candidate_arrays, explain_plan_arrays
from test_gpu_explain import _check_sums, _node_states
from test_gpu_explain_plan import _same
from test_gpu_explain_sizes import check_rows, snapshot
from test_gpu_k2_dispatch import make_checker

pytestmark = pytest.mark.gpu


def check_plan(res, inp):
    """how, fallback, the masks in one comparison, and counts / feasible / first as they follow from them."""
    assert [int(x) for x in res.how] == inp.how
    assert [int(x) for x in res.fallback] == inp.fallback
    if res.node_mask is not None:
        assert res.node_mask.shape == inp.want.shape
        assert np.array_equal(res.node_mask, inp.want), np.argwhere(res.node_mask != inp.want)[:8]
    counts, feasible, first = inp.sums()
    assert np.array_equal(res.counts, counts), np.argwhere(res.counts != counts)[:8]
    assert np.array_equal(res.feasible, feasible), np.flatnonzero(res.feasible != feasible)[:8]
    assert np.array_equal(res.first, first), np.flatnonzero(res.first != first)[:8]
    for c, (f, k) in inp.hand.items():
        assert (int(res.first[c]), int(res.feasible[c])) == (f, k), inp.names[c]


def call(ck, h, inp, node_mask=True):
    return explain_plan_arrays(ck, h, inp.sc.ptr, inp.cand_off, inp.cand_pods, inp.at_pod, inp.node_of_pod,
                               node_mask=node_mask)


def explain_input(ck, inp, masks=(False, True), loop=True):
    """One call without the per-node masks and one with them, each against the input's expectation; the
    candidates of inp.loop field for field against sr_explain_candidate; the snapshot as it was."""
    lib = capi.load_planner()
    with snapshot(inp.sc) as h:
        before = _node_states(lib, h, inp.n_spot) if inp.n_spot <= 320 else None
        for on in masks:
            res = call(ck, h, inp, on)
            assert (res.node_mask is not None) == on
            check_plan(res, inp)
        for c in inp.loop if loop and masks[-1] else ():
            lo, hi = int(inp.cand_off[c]), int(inp.cand_off[c + 1])
            _same(res, c, explain_candidate_arrays(ck, h, inp.sc.ptr, inp.cand_pods[lo:hi], inp.node_of_pod[lo:hi],
                                                   int(inp.at_pod[c])))
        if before is not None:
            assert _node_states(lib, h, inp.n_spot) == before
    return res


@pytest.mark.parametrize("n", S.SIZES)
def test_formula_pools_in_context(checker, n):
    inp = S.formula_input(n)
    assert inp.loop == list(range(inp.n)) and (inp.want[:, 64:] != S.stop_static(n)[64:]).any()
    explain_input(checker, inp)


@pytest.mark.parametrize("n", S.RUN_SIZES)
def test_first_feasible_decided_by_the_context(checker, n):
    """All runs in one call: first is the maximum of n_pad - position over the waves of a block and, by atomicMax,
    over the blocks; the lists share their early words."""
    inp = S.runs_input(n)
    res = explain_input(checker, inp, masks=(False, True))
    assert [int(x) for x in res.first] == S.run_lengths(n)[:-1] + [-1, S.HOLE]
    assert [int(x) for x in res.feasible] == [n - k for k in S.run_lengths(n)] + [n - 255]


def test_many_classes_a_context_each(checker):
    """300 candidates in the caller's order, every list on another node: the lists follow the encoder's
    active-pod order to their own stop pods; the PVC pods are asked again alone and stay outside the set."""
    inp = S.many_input()
    assert inp.how.count(C.SINGLE) == sum(inp.fallback) == 42 and inp.how.count(C.BATCHED) == 258
    res = explain_input(checker, inp)
    for k in np.flatnonzero(inp.fallback):
        assert res.feasible[k] == res.first[k] == -1 and not res.counts[k].any() and not res.node_mask[k].any()


def test_candidates_across_the_grid_split(checker):
    """65,537 queries: launch_explain_plan's second launch starts at query 65,535.  The candidates that are not
    asked take no query, so the 76,460 candidates put queries 65,534 / 65,535 / 65,536 at candidates 76,456 /
    76,457 / 76,459."""
    inp = S.split_input()
    with snapshot(inp.sc) as h:
        t0 = time.perf_counter()
        res = call(checker, h, inp)
        t1 = time.perf_counter()
        bare = call(checker, h, inp, node_mask=False)
        print("sr_explain_plan of %d candidates, %d asked: %.3f s with the masks (the buffers grow), %.3f s without"
              % (inp.n, int((inp.at_pod >= 0).sum()), t1 - t0, time.perf_counter() - t1))
    check_plan(res, inp)
    check_plan(bare, inp)
    last = [76456, 76457, 76459]
    assert [list(res.node_mask[k]) for k in last] == [[S.CPU, S.CPU, 0], [S.CPU, S.TAINT, S.CPU], [S.CPU, 0, S.CPU]]
    assert [int(res.first[k]) for k in last] == [2, -1, 1] == [int(bare.first[k]) for k in last]
    assert [int(bare.feasible[k]) for k in last] == [1, 0, 1]
    assert res.how[76458] == C.NONE and res.feasible[76458] == -1 and not res.node_mask[76458].any()


def test_buffers_across_sizes_and_entry_points():
    """One fresh context: x_in grows by the lists, their offsets and the slack behind `pods`, x_in / x_out only
    grow and sr_explain_pods shares them; every result is still its own input's expectation."""
    ck = make_checker()
    try:
        big, small = S.formula_input(4300), S.formula_input(320)
        explain_input(ck, big, masks=(True,), loop=False)
        sc, m100, m0 = X.edge_pool(65)
        with snapshot(sc) as h:
            check_rows(explain_arrays(ck, h, sc.ptr, np.array([sc.qidx(0), sc.qidx(1)], np.int32)), [m100, m0])
        explain_input(ck, S.runs_input(1100), masks=(False,), loop=False)
        explain_input(ck, small, masks=(True,), loop=False)
        pool = X.get_pool(4300)
        with snapshot(pool.sc) as h:
            check_rows(explain_arrays(ck, h, pool.sc.ptr, np.array([pool.full], np.int32)),
                       X.formula_masks(4300)[None, :])
        explain_input(ck, big, masks=(True, False), loop=False)
    finally:
        ck.close()


LIMITS = S.limit_cases()


@pytest.mark.parametrize("case", LIMITS, ids=[c.name for c in LIMITS])
def test_rule_limits(checker, case):
    b = C.Built(case)
    lib = capi.load_planner()
    with snapshot(b.sc) as h:
        before = _node_states(lib, h, b.n_spot)
        args = (checker, h, b.sc.ptr, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
        if case.name in S.REFUSED:
            # the filled snapshot holds a quantity the encoder does not take: the status of the per-candidate call
            assert len(case.cands) == 1 and case.cands[0].how == C.SINGLE
            with pytest.raises(PlannerError) as one:
                explain_candidate_arrays(checker, h, b.sc.ptr, b.cand_pods, b.node_of_pod, case.cands[0].at_pod)
            assert _node_states(lib, h, b.n_spot) == before
            for on in (True, False):
                with pytest.raises(PlannerError) as e:
                    explain_plan_arrays(*args, node_mask=on)
                assert e.value.status == one.value.status == capi.SR_ERR_CAPACITY
                assert _node_states(lib, h, b.n_spot) == before
            # the context and the snapshot serve the next call: the stop pod alone fits everywhere
            at = np.zeros(1, np.int32)
            alone = explain_plan_arrays(checker, h, b.sc.ptr, np.array([0, 1], np.int32), b.cand_pods[-1:], at, None)
            assert list(alone.how) == [C.BATCHED] and alone.feasible[0] == b.n_spot and alone.first[0] == 0
            return
        res = explain_plan_arrays(*args)
        bare = explain_plan_arrays(*args, node_mask=False)
        assert _node_states(lib, h, b.n_spot) == before
        assert [int(x) for x in res.how] == [cd.how for cd in case.cands] and not res.fallback.any()
        assert bare.node_mask is None and np.array_equal(bare.how, res.how)
        assert np.array_equal(bare.counts, res.counts) and np.array_equal(bare.feasible, res.feasible)
        assert np.array_equal(bare.first, res.first) and np.array_equal(bare.fallback, res.fallback)
        for c, cd in enumerate(case.cands):
            _check_sums(res, c, case.expected(c))
            assert res.first[c] == cd.first
            lo, hi = int(b.cand_off[c]), int(b.cand_off[c + 1])
            _same(res, c, explain_candidate_arrays(checker, h, b.sc.ptr, b.cand_pods[lo:hi], b.node_of_pod[lo:hi],
                                                   cd.at_pod))
