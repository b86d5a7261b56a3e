"""sr_shortfall_pods / sr_shortfall_plan without a GPU: the interface, and everything but the kernels through
the host view (lib/libsrexplainview.so: sr_shortfall_pods_view, sr_shortfall_plan_view), which evaluates the
statements the kernels follow (explain_node_ctx, shortfall_node).  The hand cases of tests/shortfall_sizes.py and
random clusters, every number against fitsRequest's arithmetic on the oracle's own node state
(tests/shortfall_ref.py).  It also proves on the oracle the floors the GPU tests' random seeds rely on.
test_gpu_shortfall.py and test_gpu_shortfall_sizes.py run the same inputs through the C ABI."""
import ctypes
from functools import lru_cache

import numpy as np
import pytest

import explain_plan_cases as C
import shortfall_ref as R
import shortfall_sizes as S
from helpers import Scenario, header_functions
from oracle_lib import oracle_plan
from randcluster import rand_scenario
from spotplanner import capi
from spotplanner.model import Container, ContainerPort

CASES = S.cases()
# rand_scenario arguments of the random inputs (70 spot nodes, 40 candidates, as the explain tests).  The seeds
# are the first six per kind counted from 0; test_floors_of_the_random_seeds proves what the GPU tests rely on.
RANDOM = {"plain": dict(), "inter_pod": dict(anti=0.3, valid_selectors=True)}
SEEDS = {"plain": [0, 1, 2, 3, 4, 5], "inter_pod": [0, 1, 2, 3, 4, 5]}
RUNS = [(kind, seed) for kind in sorted(SEEDS) for seed in SEEDS[kind]]
RUN_IDS = ["%s-%d" % r for r in RUNS]
NEAR_FLOOR = 5   # non-fallback queries with a near-miss node, per seed


def test_entry_points_exported_and_bound():
    lib = capi.load_planner()
    for name, nargs in (("sr_shortfall_pods", 7), ("sr_shortfall_plan", 9)):
        assert name in capi.EXPORTED and name in header_functions()
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == nargs
    assert capi.SR_ABI_VERSION == 11 and lib.sr_abi_version() == 11
    assert (capi.SR_SHORT_CPU, capi.SR_SHORT_MEMORY, capi.SR_SHORT_EPHEMERAL, capi.SR_SHORT_PODS,
            capi.SR_SHORT_COUNT) == (0, 1, 2, 3, 4)
    assert [f for f, _ in capi.sr_shortfall_out._fields_] == ["near", "only_nodes", "only_min", "only_at", "node_short"]
    assert ctypes.sizeof(capi.sr_shortfall_out) == 5 * ctypes.sizeof(ctypes.c_void_p)
    # no existing struct changed its layout
    assert [f for f, _ in capi.sr_explain_out._fields_] == ["feasible", "first", "counts", "node_mask", "fallback"]


def test_the_struct_keeps_its_arrays_alive():
    import gc
    o = capi.sr_shortfall_out(capi.ptr(np.full(3, 7, np.int32), capi.P32), None, None, None, None)
    o.only_min = capi.ptr(np.full(3, 1 << 40, np.int64), capi.P64)
    gc.collect()
    assert [o.near[i] for i in range(3)] == [7, 7, 7] and o.only_min[2] == 1 << 40


def test_null_arguments_are_refused_before_the_context_is_looked_at():
    lib = capi.load_planner()
    b = S.hand_tick()
    sc = b.sc
    h = sc.product_snapshot()
    try:
        n = len(b.cand_off) - 1
        a32, a64 = np.zeros(64, np.int32), np.zeros(64, np.int64)
        how = np.zeros(n, np.uint8)
        P32, P64 = capi.ptr(a32, capi.P32), capi.ptr(a64, capi.P64)

        def out(**missing):
            o = capi.sr_shortfall_out(P32, P32, P64, P32, None)
            for k in missing:
                setattr(o, k, None)
            return o
        why = capi.sr_explain_out(P32, P32, P32, None, None)
        cands = capi.sr_candidates(n, capi.ptr(b.cand_off, capi.P32), capi.ptr(b.cand_pods, capi.P32), None)
        AT, MAP, HOW = capi.ptr(b.at_pod, capi.P32), capi.ptr(b.node_of_pod, capi.P32), capi.ptr(how, capi.PU8)
        PODS = capi.ptr(b.cand_pods, capi.P32)
        bad, fake = capi.SR_ERR_INVALID_ARG, ctypes.c_void_p(1)  # (never dereferenced: no context without a GPU)
        W, O = ctypes.byref(why), ctypes.byref(out())
        assert lib.sr_shortfall_pods(None, h, sc.ptr, PODS, 1, W, O) == bad
        assert lib.sr_shortfall_pods(fake, None, sc.ptr, PODS, 1, W, O) == bad
        assert lib.sr_shortfall_pods(fake, h, None, PODS, 1, W, O) == bad
        assert lib.sr_shortfall_pods(fake, h, sc.ptr, None, 1, W, O) == bad
        assert lib.sr_shortfall_pods(fake, h, sc.ptr, PODS, -1, W, O) == bad
        assert lib.sr_shortfall_pods(fake, h, sc.ptr, PODS, 1, W, None) == bad
        assert lib.sr_shortfall_plan(None, h, sc.ptr, ctypes.byref(cands), AT, MAP, W, O, HOW) == bad
        assert lib.sr_shortfall_plan(fake, None, sc.ptr, ctypes.byref(cands), AT, MAP, W, O, HOW) == bad
        assert lib.sr_shortfall_plan(fake, h, None, ctypes.byref(cands), AT, MAP, W, O, HOW) == bad
        assert lib.sr_shortfall_plan(fake, h, sc.ptr, None, AT, MAP, W, O, HOW) == bad
        assert lib.sr_shortfall_plan(fake, h, sc.ptr, ctypes.byref(cands), None, MAP, W, O, HOW) == bad
        assert lib.sr_shortfall_plan(fake, h, sc.ptr, ctypes.byref(cands), AT, None, W, O, HOW) == bad
        assert lib.sr_shortfall_plan(fake, h, sc.ptr, ctypes.byref(cands), AT, MAP, W, None, HOW) == bad
        for missing in ("near", "only_nodes", "only_min", "only_at"):
            o = out(**{missing: True})
            assert lib.sr_shortfall_pods(fake, h, sc.ptr, PODS, 1, None, ctypes.byref(o)) == bad
            assert lib.sr_shortfall_plan(fake, h, sc.ptr, ctypes.byref(cands), AT, MAP, None, ctypes.byref(o), HOW) == bad
        for missing in ("feasible", "first", "counts"):  # `why` is optional, but whole when given
            w2 = capi.sr_explain_out(P32, P32, P32, None, None)
            setattr(w2, missing, None)
            assert lib.sr_shortfall_pods(fake, h, sc.ptr, PODS, 1, ctypes.byref(w2), O) == bad
            assert lib.sr_shortfall_plan(fake, h, sc.ptr, ctypes.byref(cands), AT, MAP, ctypes.byref(w2), O, HOW) == bad
        at_pod = b.at_pod.copy()  # at_pod >= the candidate's pods; a position below at_pod out of range
        at_pod[0] = 5
        assert lib.sr_shortfall_plan(fake, h, sc.ptr, ctypes.byref(cands), capi.ptr(at_pod, capi.P32), MAP, None, O,
                                     HOW) == bad
        for pos in (-1, b.n_spot):
            m = b.node_of_pod.copy()
            m[0] = pos
            assert lib.sr_shortfall_plan(fake, h, sc.ptr, ctypes.byref(cands), AT, capi.ptr(m, capi.P32), None, O,
                                         HOW) == bad
        assert lib.sr_snapshot_fork(h) == capi.SR_OK
        assert lib.sr_shortfall_plan(fake, h, sc.ptr, ctypes.byref(cands), AT, MAP, None, O, HOW) == capi.SR_ERR_STATE
    finally:
        lib.sr_snapshot_destroy(h)


def prove_case(case: S.SCase):
    """The view's masks and shortfalls equal the case's, the oracle agrees with every number, the reductions that
    follow equal the ones stated by hand.  Returns the reductions per candidate."""
    b = C.Built(case.plan)
    v = R.view_plan(b.sc, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
    osnap = b.sc.oracle_snapshot()
    assert [int(x) for x in v["how"]] == [cd.how for cd in case.plan.cands] and not v["fallback"].any()
    out = []
    for c, cd in enumerate(case.plan.cands):
        lo = int(b.cand_off[c])
        pods, mapping = b.cand_pods[lo:], b.node_of_pod[lo:]
        assert [int(m) for m in v["masks"][c]] == case.plan.expected(c), (case.name, c)
        want = case.expected_shorts(c)
        assert [[int(x) for x in r] for r in v["shorts"][c]] == want, (case.name, c)
        with R.context(b.sc, osnap, pods, mapping, cd.at_pod):
            red = R.check_query(b.sc, osnap, pods[cd.at_pod], v["masks"][c], v["shorts"][c], b.n_spot, (case.name, c))
        assert red == R.reduce_row(case.plan.expected(c), want)
        pin = case.pin[c]
        if pin:
            assert red == (pin["near"], pin["only_nodes"], pin["only_min"], pin["only_at"]), (case.name, c, red)
        out.append(red)
    # the candidates asked at their first pod: the same pod through sr_shortfall_pods' statement
    first = [c for c, cd in enumerate(case.plan.cands) if cd.at_pod == 0]
    if first:
        vp = R.view_pods(b.sc, np.array([b.cand_pods[b.cand_off[c]] for c in first], np.int32))
        for i, c in enumerate(first):
            assert np.array_equal(vp["masks"][i], v["masks"][c]) and np.array_equal(vp["shorts"][i], v["shorts"][c])
    return out


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_size_cases_through_the_view(case):
    prove_case(case)


def test_cases_cover_the_edges():
    names = {c.name for c in CASES}
    for n in S.POOLS:
        for tag in ("0", "63", "64", "last", "nowhere"):
            assert "min_%d_at_%s" % (n, tag) in names
    assert {"min_257_at_255", "min_257_at_256", "min_320_at_255", "min_320_at_256", "tie_two_waves",
            "tie_two_blocks", "above_bit_31", "two_to_the_61", "dimensions", "contexts", "pods_saturate"} <= names
    by = {c.name: c for c in CASES}
    # a last word of one live node and 63 pads, which holds the minimum
    assert len(by["min_65_at_last"].plan.nodes) == 65 and by["min_65_at_last"].pin[0]["only_at"][2] == 64
    assert by["tie_two_waves"].pin[0]["only_at"][0] == 63 and by["tie_two_blocks"].pin[0]["only_at"][1] == 255
    dims = by["dimensions"]
    masks = set(dims.plan.cands[0].masks.values())
    assert {S.CPU, S.MEMORY, S.EPHEMERAL, S.PODS, S.CPU | S.MEMORY, S.CPU | S.MEMORY | S.EPHEMERAL,
            S.TAINT | S.CPU} <= masks
    sat = by["pods_saturate"]
    assert sat.shorts[0][0][3] == sat.shorts[0][1][3] == (1 << 63) - 1 and sat.shorts[0][2][3] == (1 << 63) - 2
    # every dimension is the one of a unique minimum somewhere past word 0
    assert {d for c in CASES if c.name.startswith("min_") and "nowhere" not in c.name
            for d in range(3) if c.pin[0]["only_at"][d] >= 64} == {0, 1, 2}


def test_hand_tick_through_the_view():
    """five 600m pods, four open 1000m nodes.  Against the snapshot as it is nothing refuses the
    fifth pod; after the candidate's four earlier pods every node is 200m short."""
    b = S.hand_tick()
    stop = b.cand_pods[4:5]
    vp = R.view_pods(b.sc, stop)
    assert not vp["masks"].any() and not vp["shorts"].any()
    assert R.reduce_row(vp["masks"][0], vp["shorts"][0]) == (0, [0] * 4, [0] * 4, [-1] * 4)
    v = R.view_plan(b.sc, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
    osnap = b.sc.oracle_snapshot()
    with R.context(b.sc, osnap, b.cand_pods, b.node_of_pod, 4):
        red = R.check_query(b.sc, osnap, stop[0], v["masks"][0], v["shorts"][0], 4)
    assert red == (4, [4, 0, 0, 0], [200, 0, 0, 0], [0, -1, -1, -1])


def test_the_last_queries_of_the_grid_split():
    """Queries 65,530 .. 65,536 of the split input as a slice (cand_pod_off[0] > 0): node c % 70 is cpu-only,
    1 / 2 / 50 short, and the oracle agrees."""
    sc, cand_off, cand_pods, at_pod, node_of_pod = S.split_input()
    first = S.SPLIT_QUERIES - 7
    off = cand_off[first:].copy()
    v = R.view_plan(sc, off, cand_pods, at_pod[first:].copy(), node_of_pod[int(cand_off[first]):].copy())
    osnap = sc.oracle_snapshot()
    assert (v["how"] == C.BATCHED).all()
    for i, c in enumerate(range(first, S.SPLIT_QUERIES)):
        node, lo = c % S.SPLIT_NODES, int(cand_off[c])
        with R.context(sc, osnap, cand_pods[lo:], node_of_pod[lo:], 1):
            red = R.check_query(sc, osnap, cand_pods[lo + 1], v["masks"][i], v["shorts"][i], S.SPLIT_NODES)
        assert red == (1, [1, 0, 0, 0], [S.split_short(c), 0, 0, 0], [node, -1, -1, -1])
    assert [S.split_short(c) for c in (65534, 65535, 65536)] == [50, 1, 2]


# ---- random clusters
@lru_cache(maxsize=None)
def random_reference(kind, seed):
    """(ShortfallReference of the candidates' pods, cand_off, cand_pods) of one random cluster."""
    nodes, spot_pods, cands = rand_scenario(seed, n_spot=70, n_cand=40, max_pods=12, **RANDOM[kind])
    flat = [p for c in cands for p in c]
    ref = R.ShortfallReference(nodes, spot_pods, flat)
    cand_off = np.zeros(len(cands) + 1, np.int32)
    cand_off[1:] = np.cumsum([len(c) for c in cands])
    return ref, cand_off, ref.pod_indices()


@pytest.mark.parametrize("kind,seed", RUNS, ids=RUN_IDS)
def test_random_clusters_through_the_view(kind, seed):
    ref, cand_off, cand_pods = random_reference(kind, seed)
    v = R.view_pods(ref.sc, cand_pods)
    ref.check(v["masks"], v["shorts"], v["fallback"])
    # the oracle's plan: every batched stuck candidate in the context of its earlier pods
    sc, osnap = ref.sc, ref.osnap
    plan = oracle_plan(osnap, sc.ptr, cand_off, cand_pods, mode=1)
    at_pod = np.ascontiguousarray(plan["status"], np.int32)
    mapping = np.ascontiguousarray(plan["node_of_pod"], np.int32)
    pv = R.view_plan(sc, cand_off, cand_pods, at_pod, mapping)
    judged = 0
    for c in range(len(at_pod)):
        if at_pod[c] < 0 or pv["how"][c] != C.BATCHED or pv["fallback"][c]:
            assert not pv["masks"][c].any() and not pv["shorts"][c].any()
            continue
        lo = int(cand_off[c])
        with R.context(sc, osnap, cand_pods[lo:], mapping[lo:], int(at_pod[c])):
            R.check_query(sc, osnap, cand_pods[lo + at_pod[c]], pv["masks"][c], pv["shorts"][c], ref.n_spot, c)
        judged += 1
    assert judged >= 1


def zero_twin(pod, name):
    """`pod` with every field but its requests: zero cpu / memory / ephemeral, no scalar, the same host ports."""
    import dataclasses
    ports = [ContainerPort(p.host_port, p.container_port, p.protocol, p.host_ip) for p in pod.host_ports()]
    return dataclasses.replace(pod, name=name, containers=[Container(ports=ports)], init_containers=[])


def test_floors_of_the_random_seeds():
    """On the oracle alone: on every seed at least NEAR_FLOOR judged pods have a near-miss node; over all seeds
    cpu-only and memory-only nodes both occur.  A lower bound: where the oracle admits the pod's zero-request twin
    (the pod count and every filter but the three compares pass) and refuses the pod itself, the mask is exactly
    fitsRequest's CPU / MEMORY / EPHEMERAL bits."""
    from oracle_lib import load_oracle
    ora = load_oracle()
    only = [0, 0, 0]
    for kind, seed in RUNS:
        ref, _, _ = random_reference(kind, seed)
        twins = Scenario(ref.nodes, ref.sc.spot_pods, [zero_twin(p, "z-" + p.name) for p in ref.pods])
        tsnap = twins.oracle_snapshot()
        near = 0
        for i in range(ref.n):
            if ref.fallback[i] or ref.lists_scalar[i]:
                continue
            rows = [j for j in range(ref.n_spot) if ref.fits[i][j] == 0 and
                    ora.oracle_check_predicates(tsnap.h, twins.ptr, twins.qidx(i), j) == 1]
            near += int(len(rows) > 0)
            for j in rows:
                res = ref.resource_mask(i, j)
                assert res != 0 and res & R.PODS == 0, (kind, seed, i, j)
                for d in range(3):
                    only[d] += int(res == R.DIM_BITS[d])
        print(kind, seed, "judged pods with a near miss shown by the oracle alone:", near)
        assert near >= NEAR_FLOOR, (kind, seed, near)
    print("only-d nodes over all seeds (cpu, memory, ephemeral):", only)
    assert only[0] > 0 and only[1] > 0
