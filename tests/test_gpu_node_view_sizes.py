"""sr_node_view_pods / sr_node_view_plan at the smallest shapes at which the kernels can go wrong: the formula
pools of tests/explain_sizes.py (every reason alone on a node past word 0) cut to 1, 63, 64, 65, 256, 257 and 320
nodes -- the word boundary, the four-word block boundary, a ragged last word whose pad lanes must stay out --
with 1, 2, 7 and 8 queries and SR_NODE_VIEW_CHUNK = 1, 3 and 8 (a single chunk, a ragged last chunk, exactly full
chunks) and without it.  Every result equals node_view_ref.fold of the sibling call's per-query arrays."""
from functools import lru_cache

import numpy as np
import pytest

import explain_plan_cases as C
import explain_plan_sizes as XP
import explain_sizes as X
import node_view_ref as V
from known_answer import P
from spotplanner import capi
from spotplanner.rescheduler import (node_view_arrays, node_view_plan_arrays, shortfall_arrays, shortfall_plan_arrays)
from test_gpu_shortfall import snapshot

pytestmark = pytest.mark.gpu

POOLS = (1, 63, 64, 65, 256, 257, 320)
QUERIES = (1, 2, 7, 8)
CHUNKS = (None, 1, 3, 8)
CPU_R, TAINT_R = capi.WHY_NAMES.index("CPU"), capi.WHY_NAMES.index("TAINT")


def set_chunk(monkeypatch, per):
    if per is None:
        monkeypatch.delenv("SR_NODE_VIEW_CHUNK", raising=False)
    else:
        monkeypatch.setenv("SR_NODE_VIEW_CHUNK", str(per))


@pytest.mark.parametrize("n", POOLS)
def test_pools_queries_and_chunks(checker, monkeypatch, n):
    """The full pod and its variants (each leaves one filter group out, so the queries' masks differ node by
    node) against the pool as it is."""
    pool = X.get_pool(n)
    every = np.array([pool.full] + list(pool.variants.values()), np.int32)
    with snapshot(pool.sc) as h:
        for k in QUERIES:
            pods = every[:k]
            set_chunk(monkeypatch, None)
            why, short = shortfall_arrays(checker, h, pool.sc.ptr, pods)
            assert not why.fallback.any()
            if n in X.SIZES:  # (the formula is proved for these pools: test_explain_sizes_reference.py)
                assert np.array_equal(why.node_mask[0], X.formula_masks(n))
            want = V.fold_pods(why, short, n)
            assert want["judged"] == k
            for per in CHUNKS:
                set_chunk(monkeypatch, per)
                V.same(V.as_dict(node_view_arrays(checker, h, pool.sc.ptr, pods)), want, (n, k, per))
            # the same queries as candidates of one pod each, asked at it: the plan entry point's batched pass
            off = np.arange(k + 1, dtype=np.int32)
            for per in (None, 3):
                set_chunk(monkeypatch, per)
                res = node_view_plan_arrays(checker, h, pool.sc.ptr, off, pods, np.zeros(k, np.int32), None)
                V.same(V.as_dict(res), want, (n, k, per, "plan"))
                assert (res.how == C.BATCHED).all()
    # every reason stands alone somewhere in the 320 pool, past word 0: with the full pod alone its sole count is 1
    if n == 320:
        with snapshot(pool.sc) as h:
            set_chunk(monkeypatch, None)
            res = node_view_arrays(checker, h, pool.sc.ptr, every[:1])
        for r, bit in enumerate(X.BITS):
            alone = [j for j in range(64, n) if X.formula_mask(j) == bit]
            assert alone and all(res.sole[j][r] == 1 for j in alone), capi.WHY_NAMES[r]


@lru_cache(maxsize=None)
def context_pool():
    """The 320 pool with XP.stop_pod (batched after plain earlier pods), a 3501m pod that leaves a 4000m node 499m
    for the stop pod's 500m, and a one-milli pod."""
    return X.build(320, extra=[XP.stop_pod(), P("ctx-cpu", cpu=X.NODE_CPU - X.REQ_CPU + 1), P("ctx-tiny", cpu=1)])


def test_contexts_on_the_word_and_block_edges(checker, monkeypatch):
    """Seven candidates whose earlier pods sit on nodes 63, 64 and 256 (the last lane of word 0, the first of
    word 1, the first of block 1) and 319: the touched nodes turn cpu-short for exactly those candidates."""
    pool = context_pool()
    stop, big, tiny = pool.extra
    lists = [([big], [63]), ([big, big], [64, 256]), ([], []), ([big, big, big], [63, 64, 256]), ([tiny], [256]),
             ([big], [319]), ([tiny, big], [64, 64])]
    cand_pods = np.array([p for earlier, _ in lists for p in earlier + [stop]], np.int32)
    cand_off = np.zeros(len(lists) + 1, np.int32)
    cand_off[1:] = np.cumsum([len(e) + 1 for e, _ in lists])
    at_pod = np.array([len(e) for e, _ in lists], np.int32)
    mapping = np.array([x for _, at in lists for x in at + [-1]], np.int32)
    for j in (63, 64, 256, 319):  # the formula leaves these nodes their cpu, so the context alone decides the bit
        assert not X.refuses(j, X.CPU) and XP.base_cpu(j) == 0
    with snapshot(pool.sc) as h:
        set_chunk(monkeypatch, None)
        why, short = shortfall_plan_arrays(checker, h, pool.sc.ptr, cand_off, cand_pods, at_pod, mapping)
        assert (why.how == C.BATCHED).all() and not why.fallback.any()
        want = V.fold_plan(why, short, at_pod, 320)
        for per in CHUNKS:
            set_chunk(monkeypatch, per)
            res = node_view_plan_arrays(checker, h, pool.sc.ptr, cand_off, cand_pods, at_pod, mapping)
            V.same(V.as_dict(res), want, per)
            assert np.array_equal(res.how, why.how)
    assert want["judged"] == 7
    # by hand: candidates 0 and 3 are 1m short on node 63, 1, 3 and 6 on node 64 (6: 3502m taken, 2m short), 1 and 3
    # on node 256 (4 put one milli there: nothing), 5 on node 319
    assert [want["refuses"][j][CPU_R] for j in (63, 64, 256, 319)] == [2, 3, 2, 1]
    static = XP.stop_static(320)
    for j, (m, slot) in {64: (1, 1), 256: (1, 1)}.items():
        if static[j] == 0:
            assert want["sole_min"][j][0] == m and want["sole_at"][j][0] == slot
