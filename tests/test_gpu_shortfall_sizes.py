"""sr_shortfall_pods / sr_shortfall_plan at the sizes where their reductions can go wrong, against the formulas
and hand-stated reductions of tests/shortfall_sizes.py (proved on the oracle by test_shortfall_reference.py): the
minimum in every wave and block position of pools of 65, 257 and 320 nodes, ties across waves and blocks, pads,
shortfalls that differ only above bit 31, every dimension alone and together, contexts on a residue, the pod
shortfall that saturates, and 65,537 queries across the gridDim.y split.  No result is compared with another
call of the code under test."""
import time

import numpy as np
import pytest

import explain_plan_cases as C
import shortfall_ref as R
import shortfall_sizes as S
from spotplanner.rescheduler import shortfall_arrays, shortfall_plan_arrays
from test_gpu_k2_dispatch import make_checker
from test_gpu_shortfall import snapshot

pytestmark = pytest.mark.gpu

CASES = S.cases()


def check_case(case, why, short, cands, rows):
    """Rows `rows` of a result are candidates `cands` of the case: masks, every node's shortfalls, the reductions
    that follow from them and the ones stated by hand."""
    for i, c in zip(rows, cands):
        masks, want = case.plan.expected(c), case.expected_shorts(c)
        assert why.fallback[i] == 0
        assert [int(m) for m in why.node_mask[i]] == masks, (case.name, c)
        if short.node_short is not None:
            got = short.node_short[i]
            assert np.array_equal(got, np.array(want, np.int64)), (case.name, c, np.argwhere(got != np.array(want))[:4])
        red = R.reduce_row(masks, want)
        pin = case.pin[c]
        if pin:
            assert red == (pin["near"], pin["only_nodes"], pin["only_min"], pin["only_at"])
        R.check_reduced(short, i, red, (case.name, c))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_size_cases(checker, case):
    """Through sr_shortfall_plan (k_shortfall_plan), with and without node_short; the candidates asked at their
    first pod through sr_shortfall_pods (k_shortfall) too."""
    b = C.Built(case.plan)
    every = list(range(len(case.plan.cands)))
    first = [c for c in every if case.plan.cands[c].at_pod == 0]
    with snapshot(b.sc) as h:
        for on in (True, False):
            why, short = shortfall_plan_arrays(checker, h, b.sc.ptr, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod,
                                               node_short=on)
            assert (short.node_short is not None) == on
            assert [int(x) for x in why.how] == [cd.how for cd in case.plan.cands]
            check_case(case, why, short, every, every)
            if first:
                pods = np.array([b.cand_pods[b.cand_off[c]] for c in first], np.int32)
                why, short = shortfall_arrays(checker, h, b.sc.ptr, pods, node_short=on)
                check_case(case, why, short, first, range(len(first)))


def test_queries_across_the_grid_split(checker):
    """65,537 queries with a context each: the second launch starts at query 65,535 and writes its own partials."""
    sc, cand_off, cand_pods, at_pod, node_of_pod = S.split_input()
    n = S.SPLIT_QUERIES
    with snapshot(sc) as h:
        t0 = time.perf_counter()
        why, short = shortfall_plan_arrays(checker, h, sc.ptr, cand_off, cand_pods, at_pod, node_of_pod,
                                           node_short=False)
        print("sr_shortfall_plan of %d queries: %.3f s" % (n, time.perf_counter() - t0))
        last, tail = shortfall_plan_arrays(checker, h, sc.ptr, cand_off[n - 3:].copy(), cand_pods, at_pod[n - 3:].copy(),
                                           node_of_pod[int(cand_off[n - 3]):].copy())
    c = np.arange(n)
    assert (why.how == C.BATCHED).all() and not why.fallback.any()
    want_mask = np.zeros((n, S.SPLIT_NODES), np.uint16)
    want_mask[c, c % S.SPLIT_NODES] = C.CPU
    assert np.array_equal(why.node_mask, want_mask)
    sf = np.array([S.split_short(int(k)) for k in range(3)], np.int64)[c % 3]
    zero = np.zeros(n, np.int64)
    assert np.array_equal(short.near, np.ones(n, np.int32))
    assert np.array_equal(short.only_nodes, np.stack([np.ones(n, np.int32)] + [zero.astype(np.int32)] * 3, 1))
    assert np.array_equal(short.only_min, np.stack([sf, zero, zero, zero], 1))
    minus = np.full(n, -1, np.int32)
    assert np.array_equal(short.only_at, np.stack([(c % S.SPLIT_NODES).astype(np.int32), minus, minus, minus], 1))
    # queries 65,534 .. 65,536 by hand: nodes 14, 15, 16; 50, 1 and 2 short
    assert [int(x) for x in short.only_at[n - 3:, 0]] == [14, 15, 16]
    assert [int(x) for x in short.only_min[n - 3:, 0]] == [50, 1, 2]
    for i in range(3):
        want = np.zeros((S.SPLIT_NODES, 4), np.int64)
        want[14 + i, 0] = [50, 1, 2][i]
        assert np.array_equal(tail.node_short[i], want)
        assert tail.only_at[i][0] == 14 + i and tail.near[i] == 1


def test_buffers_across_sizes_and_entry_points():
    """One fresh context: a 320-node case, the 4-node hand tick, a 65-node case with node_short, the 320-node case
    again: the buffers only grow, and every result is still its own input's."""
    by = {c.name: c for c in CASES}
    ck = make_checker()
    try:
        for name in ("tie_two_blocks", None, "dimensions", "min_65_at_last", "tie_two_blocks"):
            if name is None:
                b = S.hand_tick()
                with snapshot(b.sc) as h:
                    _, short = shortfall_plan_arrays(ck, h, b.sc.ptr, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
                assert short.near[0] == 4 and list(short.only_min[0]) == [200, 0, 0, 0]
                continue
            case = by[name]
            b = C.Built(case.plan)
            every = list(range(len(case.plan.cands)))
            with snapshot(b.sc) as h:
                why, short = shortfall_plan_arrays(ck, h, b.sc.ptr, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
            check_case(case, why, short, every, every)
    finally:
        ck.close()
