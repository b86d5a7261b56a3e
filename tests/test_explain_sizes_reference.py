"""What test_gpu_explain_sizes.py rests on, proved on the CPU oracle alone: the
formula masks of explain_sizes.py bit by bit (the pod with one group left out
fits exactly where no other bit stands), the preconditions that make the pools
decisive (every reason alone past row word 0 and in the last live word, a node
with three bits, a feasible and a refused node in every word), the hand-written
first feasible nodes, the fallback flags and sampled rows of the 300-pod call,
and the candidates whose earlier pods decide the later pod's mask."""
import numpy as np
import pytest

import explain_sizes as X
from oracle_lib import load_oracle
from spotplanner import capi

ALL = (1 << capi.SR_WHY_COUNT) - 1


def fits_row(pool, osnap, q, nodes=None):
    lib = load_oracle()
    nodes = range(pool.n) if nodes is None else nodes
    return np.array([lib.oracle_check_predicates(osnap.h, pool.sc.ptr, q, j) for j in nodes], np.int32)


def test_bits_and_residues():
    assert X.BITS == tuple(1 << r for r in range(capi.SR_WHY_COUNT))
    assert [getattr(capi, "SR_WHY_" + name) for name in capi.WHY_NAMES] == list(X.BITS)
    mods = [m for m, _ in X.MOD_RES.values()]
    assert all(np.gcd(a, b) == 1 for i, a in enumerate(mods) for b in mods[i + 1:]), mods
    assert all(0 <= r < m for m, r in X.MOD_RES.values())


@pytest.mark.parametrize("n", X.SIZES)
def test_pool_preconditions(n):
    """Blocks of 256 nodes, waves of 64: what each pool puts where."""
    masks = X.formula_masks(n)
    W = -(-n // 64)
    assert (n, W, -(-W // 4), W % 4, n % 64) in ((320, 5, 2, 1, 0), (1100, 18, 5, 2, 12), (4300, 68, 17, 0, 12))
    past0 = masks[64:]
    alone = {int(m) for m in past0 if m and m & (m - 1) == 0}
    assert alone == set(X.BITS), sorted(alone)           # every reason decides alone outside word 0
    last = masks[(W - 1) * 64:]
    assert int(np.bitwise_or.reduce(last)) == ALL          # ... and stands in the last live word
    assert any(bin(int(m)).count("1") == 3 for m in masks) and any(bin(int(m)).count("1") == 2 for m in masks)
    for w in range(W):
        word = masks[w * 64:(w + 1) * 64]
        assert (word == 0).any() and (word != 0).any(), w
    assert masks[0] != 0                                   # the first feasible node is not node 0
    for s, members in enumerate(X.FIRST_SETS):             # no node of a first-feasible set is full
        assert not any(X.refuses(j, X.PODS) for j in members(n)), s
    # every wave position of a block holds a first feasible node in some block but the first
    zero = np.flatnonzero(masks == 0)
    assert {int(j) // 64 % 4 for j in zero if j >= 256} == ({0} if n == 320 else {0, 1, 2, 3})


@pytest.mark.parametrize("n", [320, 1100])
def test_every_bit_by_leaving_it_out(n):
    pool = X.get_pool(n)
    lib = load_oracle()
    osnap = pool.sc.oracle_snapshot()
    masks = X.formula_masks(n)
    for q in [pool.full] + list(pool.variants.values()):
        assert lib.oracle_pod_needs_fallback(osnap.h, pool.sc.ptr, q) == 0
    assert np.array_equal(fits_row(pool, osnap, pool.full), (masks == 0).astype(np.int32))
    for bit, q in pool.variants.items():
        # (without its node affinity the pod's spread pairs cover every node: explain_sizes.formula_mask)
        rest = X.formula_masks(n, affinity=False) if bit == X.NODE_AFFINITY else masks & (ALL & ~bit)
        want = (rest == 0).astype(np.int32)
        got = fits_row(pool, osnap, q)
        assert np.array_equal(got, want), (hex(bit), np.flatnonzero(got != want)[:8])
        assert want.sum() > (masks == 0).sum()             # the variant is admitted somewhere the pod is not
    # PODS is no field of the pod: the pool with room for 110 pods on every node
    roomy = X.get_pool(n, roomy=True)
    rsnap = roomy.sc.oracle_snapshot()
    assert np.array_equal(fits_row(roomy, rsnap, roomy.full), ((masks & (ALL & ~X.PODS)) == 0).astype(np.int32))
    # UNSCHEDULABLE apart from TAINT: each variant tolerates one of the two
    both = [j for j in range(n) if masks[j] == X.UNSCHEDULABLE | X.TAINT]
    assert both
    # a node that fails the affinity and holds a web pod: refused with the affinity (for it alone, by the rule
    # quoted at formula_mask) and without it (now for SPREAD: the node's pair exists and counts the web pod)
    hidden = [j for j in range(n) if X.refuses(j, X.SPREAD) and X.refuses(j, X.NODE_AFFINITY)]
    assert hidden == list(range(489, n, 580)) and all(not masks[j] & X.SPREAD for j in hidden)
    if hidden:
        assert not fits_row(pool, osnap, pool.variants[X.NODE_AFFINITY], hidden).any()
        assert not fits_row(pool, osnap, pool.full, hidden).any()
    for bit in (X.UNSCHEDULABLE, X.TAINT):
        assert not fits_row(pool, osnap, pool.variants[bit], both).any()


def test_widest_pool_feasibility():
    """The full pod on 4,300 nodes.  A call for a pod with a spread constraint walks the whole pool, so the pod
    without its constraint is asked on every node (the filters are a conjunction: where it is refused the full pod
    is), and the full pod on the nodes only SPREAD refuses, on the first and the last two row words and on one node
    of every word."""
    n = 4300
    pool = X.get_pool(n)
    lib = load_oracle()
    osnap = pool.sc.oracle_snapshot()
    masks = X.formula_masks(n)
    for q in (pool.full, pool.variants[X.SPREAD]):
        assert lib.oracle_pod_needs_fallback(osnap.h, pool.sc.ptr, q) == 0
    loose = fits_row(pool, osnap, pool.variants[X.SPREAD])
    assert np.array_equal(loose, ((masks & (ALL & ~X.SPREAD)) == 0).astype(np.int32))
    nodes = sorted(set(np.flatnonzero(masks == X.SPREAD)) | set(range(64)) | set(range(n - 76, n))
                   | set(range(37, n, 64)))
    assert len(nodes) < 300 and sum(masks[j] == X.SPREAD for j in nodes) >= 30
    assert np.array_equal(fits_row(pool, osnap, pool.full, nodes), (masks[nodes] == 0).astype(np.int32))


@pytest.mark.parametrize("n", [1100, 4300])
def test_first_feasible_nodes(n):
    """first / feasible as written, on the oracle: only the nodes of a set and the 64 before each are scanned."""
    pool = X.get_pool(n)
    lib = load_oracle()
    osnap = pool.sc.oracle_snapshot()
    for s, (first, feasible) in enumerate(X.first_want(n)):
        q = pool.firsts[s]
        assert lib.oracle_pod_needs_fallback(osnap.h, pool.sc.ptr, q) == 0
        members = X.FIRST_SETS[s](n)
        scan = sorted({j for m in members for j in range(max(0, m - 64), m + 1)}) or list(range(64))
        fits = fits_row(pool, osnap, q, scan)
        want = np.array([X.first_mask(n, s, j) == 0 for j in scan], np.int32)
        assert np.array_equal(fits, want), X.FIRST_NAMES[s]
        yes = [j for j, f in zip(scan, fits) if f]
        assert (yes[0] if yes else -1) == first and len(yes) == feasible == len(members), X.FIRST_NAMES[s]
        assert all(X.first_mask(n, s, j) & X.NODE_AFFINITY for j in range(n) if j not in members)
    # waves 0 and 3 of blocks 0 and 1, the last live wave, two blocks, two waves of one block and a later block
    assert [f // 256 for f, _ in X.first_want(n)[:4]] == [0, 0, 0, 1]
    assert [f // 64 % 4 for f, _ in X.first_want(n)[:4]] == [0, 1, 3, 0]


def test_many_pods_call():
    pool = X.get_pool(X.MANY_N, many=True)
    lib = load_oracle()
    osnap = pool.sc.oracle_snapshot()
    assert len(pool.many) == X.MANY == 300 and sorted(X.MANY_ORDER) == list(range(X.MANY))
    assert X.MANY_ORDER != sorted(X.MANY_ORDER) and X.MANY_ORDER[0] != 0
    assert len({X.many_node(i) for i in range(X.MANY)}) == X.MANY           # a node, a label value, a class each
    assert len({p.node_selector["own"] for p in pool.sc.query if p.name.startswith("many-")}) == X.MANY >= 100
    fb = [lib.oracle_pod_needs_fallback(osnap.h, pool.sc.ptr, q) for q in pool.many]
    assert fb == [int(X.many_fallback(i)) for i in range(X.MANY)] and 40 <= sum(fb) <= 45
    assert X.OVER == [j for j in range(X.MANY_N) if X.overcommitted(j)]
    # the pods whose own node is over-committed: zero requests (the shortcut admits them) and memory alone (the
    # zero cpu request is refused: allocatable < 0 + requested)
    zero = [i for i in range(X.MANY) if X.many_node(i) in X.OVER and X.many_zero(i) and not X.many_fallback(i)]
    mem = [i for i in range(X.MANY) if X.many_node(i) in X.OVER and i % 3 == 1 and not X.many_zero(i)
           and not X.many_fallback(i)]
    assert len(zero) >= 4 and len(mem) >= 4, (zero, mem)
    assert sum(X.many_mask(i, X.many_node(i)) == 0 for i in zero) >= 2
    assert sum(X.many_mask(i, X.many_node(i)) == X.CPU for i in mem) >= 2
    sample = zero + mem
    sample += [i for i in range(8, X.MANY, 23) if not X.many_fallback(i) and i not in sample][:20 - len(sample)]
    assert len(sample) == 20 and max(sample) > 200
    for i in sample:
        want = np.array([X.many_mask(i, j) == 0 for j in range(X.MANY_N)], np.int32)
        got = fits_row(pool, osnap, pool.many[i])
        assert np.array_equal(got, want), (i, np.flatnonzero(got != want)[:8])
        assert want.sum() <= 1                                                # the selector names one node
    # the full pod's masks on this pool are the formula's as well (an over-committed node refuses it for CPU as before)
    assert np.array_equal(fits_row(pool, osnap, pool.full), (X.formula_masks(X.MANY_N) == 0).astype(np.int32))


def test_edge_and_split_pools():
    lib = load_oracle()
    sc, m100, m0 = X.edge_pool(65)
    osnap = sc.oracle_snapshot()
    for q, masks in ((0, m100), (1, m0)):
        fits = [lib.oracle_check_predicates(osnap.h, sc.ptr, sc.qidx(q), j) for j in range(65)]
        assert fits == [int(m == 0) for m in masks]
    sc = X.split_pool()
    osnap = sc.oracle_snapshot()
    for q, masks in enumerate(X.SPLIT_MASKS):
        assert lib.oracle_pod_needs_fallback(osnap.h, sc.ptr, sc.qidx(q)) == 0
        fits = [lib.oracle_check_predicates(osnap.h, sc.ptr, sc.qidx(q), j) for j in range(3)]
        assert fits == [int(m == 0) for m in masks]
    assert len({tuple(m) for m in X.SPLIT_MASKS}) == 3 and X.SPLIT_ENTRIES == 65535 + 2


CAND = X.cand_cases()


def test_candidate_cases_cover_the_ways():
    names = {c.name for c in CAND}
    assert len(names) == len(CAND) == 10
    decided = 0
    for c in CAND:
        for a, b in zip(c.without, c.with_):
            decided |= a ^ b
    assert decided == X.PORTS | X.INTER_POD | X.SPREAD | X.SCALAR | X.VOLUMES | X.PODS
    assert any(len(c.pods) == 3 for c in CAND) and sum(c.flips_to_yes for c in CAND) == 1
    wide = [c for c in CAND if len(c.nodes) > 8]
    assert len(wide) == 1 and len(wide[0].nodes) == 130
    assert all(j // 64 == 2 for j, (a, b) in enumerate(zip(wide[0].without, wide[0].with_)) if a != b)


@pytest.mark.parametrize("case", CAND, ids=[c.name for c in CAND])
def test_candidate_case_on_the_oracle(case):
    sc = X.cand_scenario(case)
    lib = load_oracle()
    osnap = sc.oracle_snapshot()
    n, k = len(case.nodes), len(case.pods) - 1
    for q in range(k + 1):
        assert lib.oracle_pod_needs_fallback(osnap.h, sc.ptr, sc.qidx(q)) == 0, case.pods[q].name
    without = [lib.oracle_check_predicates(osnap.h, sc.ptr, sc.qidx(k), j) for j in range(n)]
    assert lib.oracle_snapshot_fork(osnap.h) == 0
    for q in range(k):  # each earlier pod fits where the mapping puts it, as a plan's mapping does
        assert lib.oracle_check_predicates(osnap.h, sc.ptr, sc.qidx(q), case.mapping[q]) == 1, (case.name, q)
        lib.oracle_snapshot_add_pod(osnap.h, sc.ptr, sc.qidx(q), case.mapping[q])
    with_ = [lib.oracle_check_predicates(osnap.h, sc.ptr, sc.qidx(k), j) for j in range(n)]
    lib.oracle_snapshot_revert(osnap.h)
    assert without == [int(m == 0) for m in case.without], case.rule
    assert with_ == [int(m == 0) for m in case.with_], case.rule
    deciding = [j for j in range(n) if case.without[j] != case.with_[j]]
    assert deciding
    for j in deciding:
        assert (without[j], with_[j]) == ((0, 1) if case.flips_to_yes else (1, 0)), (case.name, j)
    assert [lib.oracle_check_predicates(osnap.h, sc.ptr, sc.qidx(k), j) for j in range(n)] == without  # reverted
