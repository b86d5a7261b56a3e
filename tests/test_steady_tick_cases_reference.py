"""The preconditions of test_gpu_steady_tick_cases.py, on the CPU oracle alone:
the hand-derived nodes and statuses of steady_tick_cases.py are the oracle's on
every tick; every decisive entry has another node (or none) on the state the
tables were last written from, so a kernel that does not correct the changed
node's bits fails it; the far entries have no head node, the pointer-move
entries find their first far window full; and the matrix of sites and
situations has no empty required cell."""
import functools

import pytest

import steady_tick_cases as S
from oracle_lib import load_oracle, oracle_plan

POOL_NAMES = sorted(S.POOLS)


def oracle_snapshot(pool, tick):
    """A fresh oracle snapshot of the pool with the fillers of `tick`."""
    P = S.get_pool(pool)
    snap = P.sc.oracle_snapshot()
    for pod, pos in P.fillers_of(tick):
        snap.lib.oracle_snapshot_add_pod(snap.h, P.sc.ptr, pod, pos)
    return snap


@functools.lru_cache(maxsize=None)
def oracle_tick(pool, tick, big=True, ext=True):
    """The oracle's plan of the tick (computed once per process; do not modify)."""
    P = S.get_pool(pool)
    _, cand_off, cand_pods = P.candidate_arrays(big, ext)
    return oracle_plan(oracle_snapshot(pool, tick), P.sc.ptr, cand_off, cand_pods, mode=1, threads=8)


def pod_slot(pool, cand, pod, big=True, ext=True):
    """(index into node_of_pod, cluster pod index) of pod `pod` of candidate `cand`."""
    P = S.get_pool(pool)
    names, cand_off, cand_pods = P.candidate_arrays(big, ext)
    k = int(cand_off[names.index(cand)]) + pod
    return k, int(cand_pods[k])


def _node(x):
    return -1 if x is None else x


def _fits(snap, pool, pod, pos):
    return load_oracle().oracle_check_predicates(snap.h, S.get_pool(pool).sc.ptr, pod, pos)


@pytest.mark.parametrize("pool", POOL_NAMES)
def test_script_shape(pool):
    """t2..t10 accumulate to exactly 16 changed nodes, t11 has the 17th, t12 one against the new tables; some
    node changes a second time; no tick touches the two keepers; the last tick has no filler."""
    assert len(S.TICKS[pool]) == S.N_TICKS and S.TICKS[pool][0] == S.TICKS[pool][1] and S.TICKS[pool][-1] == {}
    counts = [len(S.changed_nodes(pool, S.TABLES_OF[t], t)) for t in range(2, 13)]
    assert counts == sorted(counts[:10]) + [1] and counts[8] == 16 and counts[9] == 17 and max(counts[:8]) < 16
    keepers = {S.ROLES[pool][k] for k in S.KEEPERS if k in S.ROLES[pool]}
    assert not keepers & S.changed_nodes(pool, 0, S.N_TICKS - 1)
    a0 = S.ROLES[pool]["A0"]
    assert a0 in S.changed_nodes(pool, 1, 2) and a0 in S.changed_nodes(pool, 4, 5)  # a second time
    for t in range(2, 12):  # each tick changes a few nodes at most
        assert len(S.changed_nodes(pool, t - 1, t)) <= 7, t
    kinds = {f for t in S.TICKS[pool] for fs in t.values() for f in fs}
    assert {"z", "e", "m", "c401"} <= kinds


@pytest.mark.parametrize("pool", POOL_NAMES)
def test_oracle_has_the_hand_written_plan(pool):
    P = S.get_pool(pool)
    names, cand_off, cand_pods = P.candidate_arrays(True)
    lib = load_oracle()
    snap = oracle_snapshot(pool, 0)
    for q in cand_pods:  # no probe pod needs the reference path
        assert lib.oracle_pod_needs_fallback(snap.h, P.sc.ptr, int(q)) == 0
    for tick in range(S.N_TICKS):
        o = oracle_tick(pool, tick)
        for c, name in enumerate(names):
            assert int(o["status"][c]) == S.expected_status(pool, tick, name), (tick, name)
    for e in S.entries(pool):
        k, _ = pod_slot(pool, e.cand, e.pod)
        assert int(oracle_tick(pool, e.tick)["node_of_pod"][k]) == _node(e.now), e


@pytest.mark.parametrize("pool", POOL_NAMES)
def test_entries_are_decisive(pool):
    """On the state the tables were last written from the pod of a decisive entry has another node or none;
    (a): the changed node is that node and takes the pod no more; (b): it is the node the pod has now and did
    not take it then.  A guard's pod has the same node on both states."""
    for e in S.entries(pool):
        k, q = pod_slot(pool, e.cand, e.pod)
        stale_tick = S.TABLES_OF[e.tick]
        stale = int(oracle_tick(pool, stale_tick)["node_of_pod"][k])
        assert stale == _node(e.before), e
        assert e.changed in S.changed_nodes(pool, stale_tick, e.tick), e
        guard = any(s in S.GUARDS for s in e.situation)
        assert (e.before == e.now) == guard, e
        then, now = oracle_snapshot(pool, stale_tick), oracle_snapshot(pool, e.tick)
        if "a" in e.situation:
            assert e.changed == e.before and _fits(then, pool, q, e.changed) == 1 and \
                _fits(now, pool, q, e.changed) == 0, e
        if any(s in ("b", "b_exact", "b_inside") for s in e.situation):
            assert e.changed == e.now and _fits(then, pool, q, e.changed) == 0 and \
                _fits(now, pool, q, e.changed) == 1, e
        if "b_minus1" in e.situation or "e_memonly" in e.situation:
            assert _fits(now, pool, q, e.changed) == 0, e
        if "e_zero" in e.situation:
            assert _fits(now, pool, q, e.changed) == 1 and e.now == e.changed, e
            assert now.node_state(e.changed)[0][0] > 1000, e  # overcommitted in cpu
        if "c" in e.situation:  # the node fits the same request without the selector, now and not then
            twin = pod_slot(pool, "comb_any", 0)[1]
            assert _fits(then, pool, twin, e.changed) == 0 and _fits(now, pool, twin, e.changed) == 1 and \
                _fits(now, pool, q, e.changed) == 0, e


@pytest.mark.parametrize("pool", ["far", "wide"])
def test_far_entries_have_no_head_node(pool):
    """A far-class pod is refused by every node below 512 on its tick (it resolves beyond the head); the
    head-class guard of (c) by every node from 512 on."""
    for e in S.entries(pool):
        if e.site not in S.FAR_SITES:
            continue
        _, q = pod_slot(pool, e.cand, e.pod)
        snap = oracle_snapshot(pool, e.tick)
        rng = range(S.HEAD_NODES, S.POOLS[pool]) if e.cand.endswith("_head") else range(S.HEAD_NODES)
        assert e.cand.endswith(("_far", "_head")), e
        assert all(_fits(snap, pool, q, n) == 0 for n in rng), e


@pytest.mark.parametrize("pool", ["far", "wide"])
def test_pointer_move_entries_find_their_window_full(pool):
    """The first far word with a node for the pod on the tick's base state has none left once the earlier
    pods of its candidate are placed; the next word with a node for it holds the changed node and a second
    one that takes the pod."""
    P = S.get_pool(pool)
    seen = 0
    for e in S.entries(pool):
        if e.site != "far_move":
            continue
        seen += 1
        k, q = pod_slot(pool, e.cand, e.pod)
        base = oracle_snapshot(pool, e.tick)
        far_words = range(S.HEAD_NODES // 64, (S.POOLS[pool] + 63) // 64)

        def nodes_for(snap, w):
            return [n for n in range(64 * w, min(64 * w + 64, S.POOLS[pool])) if _fits(snap, pool, q, n) == 1]

        first = next(w for w in far_words if nodes_for(base, w))
        later = oracle_snapshot(pool, e.tick)
        plan = oracle_tick(pool, e.tick)["node_of_pod"]
        for j in range(e.pod):
            later.lib.oracle_snapshot_add_pod(later.h, P.sc.ptr, pod_slot(pool, e.cand, j)[1], int(plan[k - e.pod + j]))
        assert nodes_for(later, first) == [], e
        then = oracle_snapshot(pool, S.TABLES_OF[e.tick])
        nxt = next(w for w in far_words if w > first and (nodes_for(base, w) or nodes_for(then, w)))
        assert e.changed // 64 == nxt and [n for n in nodes_for(later, nxt) if n != e.changed], e
    assert seen >= 2


def test_matrix_has_no_empty_required_cell():
    """Every site takes (a) and (b); (c) to (g) each at a head site and at a far site; every form of (b);
    the far scan with full S rows (`far`) and with head-only ones (`wide`), in chunk 0 and in chunk 1."""
    cells = set()
    for pool in POOL_NAMES:
        for e in S.entries(pool):
            assert e.tick in S.TABLES_OF and e.site in S.SITES + ("far_window",), e
            assert all(s in S.SITUATIONS for s in e.situation), e
            if e.changed is not None and e.site in ("head_w0", "head_w1_7"):
                assert (e.changed < 64) == (e.site == "head_w0") and e.changed < S.HEAD_NODES, e
            if e.site in S.FAR_SITES:
                assert e.changed >= S.HEAD_NODES and (e.site == "far_scan_c1") == (e.changed >= 4096 and
                                                                                   e.site != "far_window"), e
            if e.cand == "big100":
                assert e.pod >= 64 or "e_memonly" in e.situation, e
            if e.cand == "big200":
                assert e.pod >= 128, e
            sites = {e.site, S.CAND_SITE.get(e.cand, e.site)}
            for site in sites:
                for s in e.situation:
                    cells.add((site, "b" if s.startswith("b") and s != "b_minus1" else s))
                    cells.add((pool, site, s))
                    cells.add(("k0_less" if e.tick in S.K0_LESS else "k0", site,
                               "b" if s.startswith("b") and s != "b_minus1" else s))
            where = "far" if e.site in S.FAR_SITES else "head"
            for s in e.situation:
                cells.add((where, s[0]))
                cells.add((where, s))
    missing = [(site, s) for site in S.SITES for s in ("a", "b") if (site, s) not in cells]
    missing += [(site, s) for site in S.SITES for s in ("a", "b")
                if ("k0_less", site, s) not in cells]  # ... on a tick that launches no K0
    missing += [(where, s) for where in ("head", "far") for s in "cdefg" if (where, s) not in cells]
    missing += [s for s in S.SITUATIONS if not any(c[-1] == s for c in cells)]
    missing += [(pool, site, s) for pool in ("far", "wide") for site in ("far_scan_c0", "far_move")
                for s in ("a", "b_exact") if (pool, site, s) not in cells]
    assert missing == []
    # the memory requests: MiB multiples but for modd's odd byte count
    for kind, req in S.KINDS.items():
        assert (req.get("memory", 0) % S.MiB != 0) == (kind == "modd")
