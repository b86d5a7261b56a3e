"""What test_gpu_explain_plan_sizes.py rests on, proved without a GPU: every
input of explain_plan_sizes.py through the host view (lib/libsrexplainview.so:
which way each candidate goes, its context list as the kernel reads it, and the
masks explain_node_ctx gives on every node) and through the oracle forked and
filled the same way (its yes / no and fitsRequest's four bits); the hand values
around the grid split and of the runs; and the preconditions that make the
inputs decisive (test_inputs_cover_the_edges)."""
import ctypes

import numpy as np
import pytest

import explain_plan_cases as C
import explain_plan_sizes as S
import explain_sizes as X
from oracle_lib import load_oracle
from spotplanner import capi
from test_explain_plan_reference import load_view, view

LIMITS = S.limit_cases()


def prove(inp, oracle=None):
    """The view on every candidate; the oracle on the candidates `oracle` (default: every evaluated one)."""
    v = view(inp.sc, inp.cand_off, inp.cand_pods, inp.at_pod, inp.node_of_pod)
    assert [int(x) for x in v["how"]] == inp.how
    assert [int(s >= 1) for s in v["slack"]] == [int(x) for x in v["atom0"]]
    for c in range(inp.n):
        if inp.how[c] == C.BATCHED:
            assert v["ctx"][c] == inp.ctx[c], (inp.names[c], v["ctx"][c][:4])
        else:  # (a pod the batched encode hands back keeps the list plan_queries made for it)
            assert inp.ctx[c] is None and (v["ctx"][c] == [] or inp.fallback[c])
    assert np.array_equal(v["masks"], inp.want), np.argwhere(v["masks"] != inp.want)[:8]
    osnap = inp.sc.oracle_snapshot()
    for c in (range(inp.n) if oracle is None else oracle):
        if not inp.evaluated(c):
            continue
        lo, hi = int(inp.cand_off[c]), int(inp.cand_off[c + 1])
        fits, bits = C.oracle_in_context(inp.sc, osnap, inp.cand_pods[lo:hi], inp.node_of_pod[lo:hi],
                                         int(inp.at_pod[c]), inp.n_spot)
        assert fits == [int(m == 0) for m in inp.want[c]], inp.names[c]
        assert bits == [int(m) & S.RESOURCE_BITS for m in inp.want[c]], inp.names[c]
    return v


def check_hand(inp):
    _, feasible, first = inp.sums()
    for c, (f, k) in inp.hand.items():
        assert (int(first[c]), int(feasible[c])) == (f, k), inp.names[c]


@pytest.mark.parametrize("n", S.SIZES)
def test_formula_pools_in_context(n):
    inp = S.formula_input(n)
    prove(inp)
    static = S.stop_static(n)
    rows = dict(zip(S.FORMULA_NAMES, inp.want))
    # the rule engine off the touched nodes is the formula: the stop pod alone
    assert np.array_equal(rows["empty"], static) and inp.ctx[S.FORMULA_NAMES.index("empty")] == []
    assert np.array_equal(static, X.formula_masks(n, affinity=False) & ~np.uint16(S.INTER_POD | S.SPREAD)
                          | (X.formula_masks(n) & S.NODE_AFFINITY))
    # one milli short: a CPU bit on every touched node, new wherever the node had room for the request; exactly
    # the request left: no new bit anywhere
    short = S.class_nodes(n, "cpu_one_short")
    assert all(rows["cpu_one_short"][j] == static[j] | S.CPU for j in short)
    assert sum(not static[j] & S.CPU for j in short) == sum(not X.refuses(j, S.CPU) for j in short) >= 6
    assert np.array_equal(rows["cpu_exact"], static)
    assert sum(c[2][0] > 0 for c in inp.ctx[S.FORMULA_NAMES.index("cpu_exact")]) >= 6
    for name, bits in (("memory", S.MEMORY), ("ephemeral", S.EPHEMERAL), ("all_three", S.CPU | S.MEMORY | S.EPHEMERAL)):
        touched = S.class_nodes(n, name)
        assert all(rows[name][j] == static[j] | bits for j in touched), name
        assert np.array_equal(np.flatnonzero(rows[name] != static),
                              [j for j in touched if static[j] & bits != bits]), name
        assert any(static[j] for j in touched) and any(static[j] == 0 for j in touched), name
    full, room = S.count_nodes(n)
    assert list(np.flatnonzero(rows["pod_count"] != static)) == [full] and rows["pod_count"][full] == S.PODS
    assert inp.ctx[S.FORMULA_NAMES.index("pod_count")] == [(room, 109, (109, 0, 0)), (full, 110, (110, 0, 0))]
    # distinct cluster pods on one candidate's nodes, one repeated pod index on another's
    lo = inp.cand_off
    assert len(set(inp.cand_pods[lo[0]:lo[1]])) == lo[1] - lo[0]
    assert len(set(inp.cand_pods[lo[2]:lo[3] - 1])) == 1 and lo[3] - lo[2] - 1 == len(S.class_nodes(n, "memory")) > 8
    assert len(set(inp.cand_pods[lo[1:] - 1])) == 1       # every candidate stops at the same pod


@pytest.mark.parametrize("n", S.RUN_SIZES)
def test_runs_decide_the_first_feasible_node(n):
    inp = S.runs_input(n)
    prove(inp)
    check_hand(inp)
    W = -(-n // 64)
    assert S.run_lengths(n) == [63, 64, 255, 256, (W - 1) * 64, n - 1, n] and len(inp.hand) == inp.n == 8
    _, feasible, first = inp.sums()
    assert [int(x) for x in first] == [63, 64, 255, 256, (W - 1) * 64, n - 1, -1, S.HOLE]
    assert [int(x) for x in feasible] == [n - 63, n - 64, n - 255, n - 256, n - (W - 1) * 64, 1, 0, n - 255]
    # waves 0, 1, 3 of block 0, block 1, the last block and its last live wave
    assert [f // 256 for f in first[:6]] == [0, 0, 0, 1, (W - 1) // 4, (W - 1) // 4]
    assert [f // 64 % 4 for f in first[:4]] == [0, 1, 3, 0] and (W - 1) % 4 in (1, 3)
    # the lists share their early words and end in different ones
    assert {x[-1][0] // 64 for x in inp.ctx} == {0, 3, W - 2, W - 1} and all(x[:63] == inp.ctx[0] for x in inp.ctx)
    assert len({tuple(x) for x in inp.ctx}) == 8


def test_many_classes_a_context_each():
    inp = S.many_input()
    pool_nodes = [X.many_node(i) for i in X.MANY_ORDER]
    # only the view for all 300; the oracle for the pods whose answer the context decides and every seventh other
    decided = [k for k, i in enumerate(X.MANY_ORDER)
               if inp.evaluated(k) and inp.want[k][pool_nodes[k]] != X.many_mask(i, pool_nodes[k])]
    prove(inp, oracle=sorted(set(decided) | set(range(0, X.MANY, 7))))
    assert inp.how.count(C.SINGLE) == sum(inp.fallback) == 42 and inp.how.count(C.BATCHED) == 258
    lib = load_oracle()
    osnap = inp.sc.oracle_snapshot()
    for k in range(X.MANY):
        stop = int(inp.cand_pods[inp.cand_off[k] + 1])
        assert lib.oracle_pod_needs_fallback(osnap.h, inp.sc.ptr, stop) == inp.fallback[k]
        assert not inp.want[k].any() if inp.fallback[k] else inp.ctx[k][0][0] == pool_nodes[k]
    assert len(set(pool_nodes)) == X.MANY                      # every list names another node
    assert len({tuple(x[0]) for x in inp.ctx if x}) == 258
    # off its own node a row is the pod's row against the base snapshot; on it, by the pod's requests:
    seen = set()
    for k, i in enumerate(X.MANY_ORDER):
        if inp.fallback[k]:
            continue
        j, over = pool_nodes[k], (S.CPU, S.MEMORY, S.EPHEMERAL)[S.many_over(i)]
        base = np.array([X.many_mask(i, jj) for jj in range(X.MANY_N)], np.uint16)
        assert np.array_equal(np.delete(inp.want[k], j), np.delete(base, j))
        new = int(inp.want[k][j]) & ~int(base[j])
        if X.many_zero(i):
            assert new == 0                                        # a request of all zeros: the pod count alone
        else:
            assert int(inp.want[k][j]) & over                      # whatever it asks in that dimension
            asks = (i % 3 != 1, i % 3 != 0, i % 3 == 2)[S.many_over(i)]
            seen.add(("asks" if asks else "zero dimension", over, bool(new)))
    assert {(a, o) for a, o, new in seen if new} == {(a, o) for a in ("asks", "zero dimension")
                                                    for o in (S.CPU, S.MEMORY, S.EPHEMERAL)}
    assert len(decided) > 200


def test_grid_split_inputs():
    inp = S.split_input()
    asked = inp.at_pod >= 0
    assert inp.n == S.SPLIT_N and asked.sum() == S.SPLIT_QUERIES == 65535 + 2
    query = np.cumsum(asked) - 1                # the query a candidate becomes: the asked ones, in order
    assert [int(query[k]) for k in sorted(S.SPLIT_HAND)] == [65534, 65535, 65536] and asked[sorted(S.SPLIT_HAND)].all()
    kinds = {S.split_kind(k): k for k in range(28)}
    assert len(kinds) == 3 * 5   # the periods are coprime: every stop pod in every context
    v = prove(inp, oracle=sorted(set(kinds.values()) | set(S.SPLIT_HAND)))
    assert not v["fallback"].any()
    check_hand(inp)
    rows = [tuple(int(m) for m in inp.want[k]) for k in sorted(S.SPLIT_HAND)]
    assert rows == [tuple(r) for r, _, _ in (S.SPLIT_HAND[k] for k in sorted(S.SPLIT_HAND))]
    assert sorted(S.SPLIT_HAND) == [76456, 76457, 76459] and len(set(rows)) == 3
    for k in S.SPLIT_HAND:   # a non-empty context that changes the row against the base snapshot
        p, where = S.split_kind(k)
        assert inp.ctx[k] == [(where, 1, (S.SPLIT_EARLIER_CPU, 0, 0))]
        assert list(inp.want[k]) != X.SPLIT_MASKS[p]
    ways = {where for _, where in kinds}
    assert ways == {"none", "skip", 0, 1, 2} and {p for p, _ in kinds} == {0, 1, 2}
    assert [inp.how[k] for k in range(7)] == [C.BATCHED] * 4 + [C.NONE] + [C.BATCHED] * 2
    entries = sum(len(x) for x in inp.ctx if x)
    assert entries == sum(isinstance(S.split_kind(k)[1], int) for k in range(S.SPLIT_N)) > 50000


def test_inputs_cover_the_edges():
    for n in S.SIZES:   # touched nodes in the last live word, in every word, on refused and on open nodes
        inp = S.formula_input(n)
        W = -(-n // 64)
        touched = {e[0] for x in inp.ctx for e in x}
        assert {j // 64 for j in touched} == set(range(W)), n
        last = [j for j in touched if j // 64 == W - 1]
        assert len(last) >= 3 and any(inp.want[c][j] != S.stop_static(n)[j] for c in range(inp.n) for j in last), n
        assert max(e[1] for x in inp.ctx for e in x) == 110     # a merged entry with pods > 64
        assert all(np.gcd(S.CLASS_MOD, m) == 1 for m, _ in X.MOD_RES.values())
        assert len(set(S.CLASS_RES.values())) == len(S.CLASS_RES)
    for n in S.RUN_SIZES:
        assert any(x and x[-1][0] == n - 1 for x in S.runs_input(n).ctx)
    assert {len(c.nodes) for c in LIMITS} == {3, 5}
    assert [c.name for c in LIMITS if any(cd.how == C.SINGLE for cd in c.cands)] == list(S.REFUSED)


def _status_on_the_single_path(b, c):
    """What the encoder answers for candidate c asked the SINGLE way: the earlier pods added to a snapshot of the
    view library, the stop pod asked alone against it."""
    lib = load_view()
    lib.sr_snapshot_add_pod.argtypes = [ctypes.c_void_p, ctypes.POINTER(capi.sr_cluster), ctypes.c_int32,
                                        ctypes.c_int32]
    lib.sr_snapshot_add_pod.restype = ctypes.c_int32
    sc, n = b.sc, b.n_spot
    h = ctypes.c_void_p()
    assert lib.sr_snapshot_create(sc.ptr, capi.ptr(sc.spot, capi.P32), n, capi.ptr(sc.node_pod_off, capi.P32),
                                  capi.ptr(sc.node_pod_idx, capi.P32), ctypes.byref(h)) == capi.SR_OK
    try:
        lo, k = int(b.cand_off[c]), int(b.at_pod[c])
        for q in range(k):
            st = lib.sr_snapshot_add_pod(h, sc.ptr, int(b.cand_pods[lo + q]), int(b.node_of_pod[lo + q]))
            assert st == capi.SR_OK
        off, pods, at = np.array([0, 1], np.int32), b.cand_pods[lo + k:lo + k + 1].copy(), np.zeros(1, np.int32)
        how, fb, coff = np.zeros(1, np.uint8), np.zeros(1, np.uint8), np.zeros(2, np.int32)
        node, cnt, acc = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros((1, 3), np.int64)
        slack, atom0, masks = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros((1, n), np.uint16)
        cands = capi.sr_candidates(1, capi.ptr(off, capi.P32), capi.ptr(pods, capi.P32), None)
        return lib.sr_explain_plan_view(sc.ptr, h, ctypes.byref(cands), capi.ptr(at, capi.P32), None,
                                        capi.ptr(how, capi.PU8), capi.ptr(coff, capi.P32), capi.ptr(node, capi.P32),
                                        capi.ptr(cnt, capi.P32), capi.ptr(acc, capi.P64), 1, capi.ptr(slack, capi.P32),
                                        capi.ptr(atom0, capi.PU8), capi.ptr(masks, capi.PU16), capi.ptr(fb, capi.PU8))
    finally:
        lib.sr_snapshot_destroy(h)


@pytest.mark.parametrize("case", LIMITS, ids=[c.name for c in LIMITS])
def test_rule_limits(case):
    b = C.Built(case)
    v = view(b.sc, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
    osnap = b.sc.oracle_snapshot()
    assert [int(x) for x in v["how"]] == [cd.how for cd in case.cands]
    assert not v["fallback"].any()
    for c, cd in enumerate(case.cands):
        lo, hi = int(b.cand_off[c]), int(b.cand_off[c + 1])
        if cd.how == C.BATCHED:
            assert v["ctx"][c] == cd.ctx, (c, v["ctx"][c])
            assert [int(m) for m in v["masks"][c]] == case.expected(c), c
            zero = np.flatnonzero(v["masks"][c] == 0)
            assert (int(zero[0]) if len(zero) else -1) == cd.first
        else:
            assert v["ctx"][c] == [] and not v["masks"][c].any()
            assert _status_on_the_single_path(b, c) == capi.SR_ERR_CAPACITY   # the encoder refuses the quantity
            if case.name == S.NO_INT64:
                continue
        fits, bits = C.oracle_in_context(b.sc, osnap, b.cand_pods[lo:hi], b.node_of_pod[lo:hi], cd.at_pod, b.n_spot)
        assert fits == [int(m == 0) for m in case.expected(c)], c
        assert bits == [int(m) & S.RESOURCE_BITS for m in case.expected(c)], c
    assert (case.name in S.REFUSED) == any(cd.how == C.SINGLE for cd in case.cands)
