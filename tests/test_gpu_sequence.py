"""sr_plan_sequence on the GPU against the reference pass on the oracle
(sequence_ref.py): the drains, the stop, every judged candidate's status and
mapping, and the snapshot the pass leaves behind, on the inputs whose
preconditions test_sequence_reference.py asserts on the CPU."""
import ctypes
import os

import numpy as np
import pytest

from oracle_lib import oracle_plan
from sequence_ref import (BUILDERS, DYNAMIC_STOPS, FALLBACK_STOPS, FLIP_ROUND, RECORDED, SKIPPED, VOLFLIP, divergence,
                          from_synth, get_input)
from spotplanner import capi
from spotplanner.planner import PlannerError
from spotplanner.rescheduler import plan_arrays, plan_sequence_arrays
from spotplanner.synth import SynthCluster
from test_gpu_parity import compare_plans

pytestmark = pytest.mark.gpu


def make_checker(**env):
    """A planner of its own, created under `env` (read at sr_create)."""
    from spotplanner.planner import PredicateChecker
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return PredicateChecker(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def node_states(h, n_spot):
    lib = capi.load_planner()
    out = []
    for pos in range(n_spot):
        req = np.zeros(3, np.int64)
        k = ctypes.c_int32()
        assert lib.sr_snapshot_node_state(h, pos, capi.ptr(req, capi.P64), ctypes.byref(k)) == capi.SR_OK
        out.append((tuple(int(x) for x in req), int(k.value)))
    return out


def run_sequence(ck, inp, h, max_drains=None, first_cand=0):
    return plan_sequence_arrays(ck, h, inp.ptr, inp.cand_off, inp.cand_pods, max_drains, first_cand)


def assert_equals_reference(inp, h, got, ref, states):
    assert list(got.drained) == list(ref.drained)
    assert (got.stop, got.stop_cand) == (ref.stop, ref.stop_cand)
    assert np.array_equal(got.status, ref.status), (got.status, ref.status)
    assert np.array_equal(got.node_of_pod, ref.node_of_pod)
    assert node_states(h, len(inp.spot)) == states
    assert got.rounds <= len(got.drained) + 1, (got.rounds, len(got.drained))
    assert 0 <= got.rounds_k0 <= got.rounds and 0 <= got.rounds_reused <= got.rounds


def check_sequence(ck, inp, max_drains=None):
    ref, states = inp.reference(max_drains)
    h = inp.product_snapshot()
    try:
        got = run_sequence(ck, inp, h, max_drains)
        assert_equals_reference(inp, h, got, ref, states)
    finally:
        capi.load_planner().sr_snapshot_destroy(h)
    return got


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_sequence_matches_reference_pass(checker, name):
    check_sequence(checker, get_input(name))


@pytest.mark.parametrize("name", ["plain-4", "features-11", "c5", "vol-11", "spread-22", "realistic-80"])
def test_budgets(checker, name):
    inp = get_input(name)
    lib = capi.load_planner()
    full, _ = inp.reference()
    # budget 1 is sr_plan_first
    got = check_sequence(checker, inp, 1)
    h = inp.product_snapshot()
    try:
        n = len(inp.cand_off) - 1
        c = capi.sr_candidates(n, capi.ptr(inp.cand_off, capi.P32), capi.ptr(inp.cand_pods, capi.P32), None)
        wmap = np.full(int(np.max(np.diff(inp.cand_off))), -1, np.int32)
        o = capi.sr_plan_out()
        o.winner_map = capi.ptr(wmap, capi.P32)
        assert lib.sr_plan_first(checker.handle, h, inp.ptr, ctypes.byref(c), ctypes.byref(o)) == capi.SR_OK
    finally:
        lib.sr_snapshot_destroy(h)
    assert list(got.drained) == [o.winner] and got.stop == capi.SR_SEQ_BUDGET
    off = inp.cand_off - inp.cand_off[0]
    assert np.array_equal(got.node_of_pod[off[o.winner]:off[o.winner + 1]], wmap[:o.winner_npods])
    # budgets 2 and 3: prefixes of the unlimited order, everything after the last drain not judged; the
    # snapshot holds exactly the drained candidates' pods (the reference's states after the same budget)
    for budget in (2, 3):
        got = check_sequence(checker, inp, budget)
        assert list(got.drained) == list(full.drained[:budget]) and got.stop == capi.SR_SEQ_BUDGET
        last = int(got.drained[-1])
        assert np.all(got.status[last + 1:] == SKIPPED) and np.all(got.node_of_pod[off[last + 1]:] == -1)
        assert np.array_equal(got.status[:last + 1], full.status[:last + 1])


@pytest.mark.parametrize("seed", sorted(FALLBACK_STOPS))
def test_fallback_stop_and_resume(checker, seed):
    inp = get_input("fallback-%d" % seed)
    ref, states = inp.reference()
    h = inp.product_snapshot()
    try:
        got = run_sequence(checker, inp, h)
        assert_equals_reference(inp, h, got, ref, states)
        assert (got.stop, got.stop_cand) == (capi.SR_SEQ_FALLBACK, FALLBACK_STOPS[seed])
        # the shim judges stop_cand itself (here: not drainable) and resumes behind it on the same snapshot
        ref2, states2 = inp.reference(None, got.stop_cand + 1, after=(None, 0))
        got2 = run_sequence(checker, inp, h, None, got.stop_cand + 1)
        assert_equals_reference(inp, h, got2, ref2, states2)
        assert np.all(got2.status[:got.stop_cand + 1] == SKIPPED)
    finally:
        capi.load_planner().sr_snapshot_destroy(h)


def record_rounds(record_property, what, got):
    print("%s: rounds %d, with K0 %d, reused %d" % (what, got.rounds, got.rounds_k0, got.rounds_reused))
    record_property("rounds", got.rounds)
    record_property("rounds_k0", got.rounds_k0)
    record_property("rounds_reused", got.rounds_reused)


@pytest.mark.parametrize("start", ["cold", "warm"])
@pytest.mark.parametrize("name", DYNAMIC_STOPS)
def test_dynamic_fallback_stop_and_resume(name, start, record_property):
    """A candidate the base snapshot plans turns into a reference-path candidate against the snapshot the earlier
    drains leave (volflip-*: a spot node now holds its attachable volume; spread-2: the drained pods are on the
    spot nodes its spread constraints read), while the encoder is reusing the candidate side: the classification
    is that round's prepare's, not the first one's.

    "cold" is a new planner: it reuses from its third round, so the flip meets a reusing planner on the
    volflip-* inputs (round 5).  On spread-2 the first drain already turns candidate 5 (FLIP_ROUND: round 2, a
    fallback decided by the snapshot's counts, with which the encoder builds no reuse index), so a cold planner
    runs its 6 rounds with rounds_reused == 0 whatever it does; "warm" plans the same input three times from the
    base snapshot first, so that the sequence's first round is already a reusing one and the flip has to be
    noticed by the reuse itself on every input."""
    inp = get_input(name)
    ref, states = inp.reference()
    stop_cand = RECORDED[name][2]
    ck = make_checker()
    h = inp.product_snapshot()
    try:
        if start == "warm":
            hb = inp.product_snapshot()
            try:
                for _ in range(3):
                    plan_arrays(ck, hb, inp.ptr, inp.cand_off, inp.cand_pods)
            finally:
                capi.load_planner().sr_snapshot_destroy(hb)
            assert ck.timing().enc_reused == 1
        got = run_sequence(ck, inp, h)
        record_rounds(record_property, "%s %s" % (name, start), got)
        assert (got.stop, got.stop_cand) == (capi.SR_SEQ_FALLBACK, stop_cand)
        assert_equals_reference(inp, h, got, ref, states)
        if start == "warm" or FLIP_ROUND[name] >= 4:
            assert got.rounds_reused >= 1  # the flip met a planner that had been reusing
        ref2, states2 = inp.reference(None, stop_cand + 1, after=(None, 0))
        got2 = run_sequence(ck, inp, h, None, stop_cand + 1)
        assert_equals_reference(inp, h, got2, ref2, states2)
        assert np.all(got2.status[:stop_cand + 1] == SKIPPED)
        if name in VOLFLIP:
            assert list(ref2.drained) == [6] and list(got2.drained) == [6]
    finally:
        capi.load_planner().sr_snapshot_destroy(h)
        ck.close()


REALISTIC_FORMS = {
    "default": {},
    "k0_every_round": dict(SR_K0_SKIP=0),
    "k0_whole": dict(SR_K0_INCREMENTAL=0),
    "pod_order": dict(SR_K2_MODE=1),
    "general_kernel": dict(SR_K2_NODE_KERNEL=0),
    "whole_node_section": dict(SR_NODE_PATCH=0),
    "wide_rows": dict(SR_K2_NARROW=0),
    "one_plan_slot": dict(SR_PLAN_SLOTS=1),
}
REALISTIC_BUDGET = 10


@pytest.mark.parametrize("form", sorted(REALISTIC_FORMS))
def test_realistic_forms(form, record_property):
    """The floor under the extension-record instances (k2_node<G, XT>, the x windows) and the other K2 and K0
    forms, on the input most of whose candidates carry extension records (init-container accounting, shared
    scalar names and volume-limit keys; test_realistic_80_has_extension_record_candidates)."""
    ck = make_checker(**REALISTIC_FORMS[form])
    try:
        got = check_sequence(ck, get_input("realistic-80"), REALISTIC_BUDGET)
    finally:
        ck.close()
    record_rounds(record_property, "realistic-80 %s" % form, got)
    assert got.rounds == REALISTIC_BUDGET
    if form == "k0_every_round":
        assert got.rounds_k0 == got.rounds


def test_drained_only_call_then_other_workloads(checker):
    """status == NULL and node_of_pod == NULL: the call returns while the last round's K2 and ledger kernel may
    still run.  The next call on the context, a larger plan on another cluster (buffers move), and a sequence
    after it are the oracle's."""
    inp, c5, vol = get_input("realistic-80"), get_input("c5"), get_input("vol-11")
    ref, states = inp.reference(5)
    o5 = oracle_plan(c5.oracle_snapshot(), c5.ptr, c5.cand_off, c5.cand_pods, mode=1, threads=8)
    lib = capi.load_planner()
    h, h5 = inp.product_snapshot(), c5.product_snapshot()
    try:
        n = len(inp.cand_off) - 1
        c = capi.sr_candidates(n, capi.ptr(inp.cand_off, capi.P32), capi.ptr(inp.cand_pods, capi.P32), None)
        drained = np.full(5, -1, np.int32)
        o = capi.sr_sequence_out()
        o.max_drains = 5
        o.drained = capi.ptr(drained, capi.P32)
        st = lib.sr_plan_sequence(checker.handle, h, inp.ptr, ctypes.byref(c), ctypes.byref(o))
        p = plan_arrays(checker, h5, c5.ptr, c5.cand_off, c5.cand_pods)  # no other call in between
        assert st == capi.SR_OK, checker.last_error()
        assert list(drained[:o.n_drained]) == list(ref.drained)
        assert (o.stop, o.stop_cand) == (ref.stop, ref.stop_cand) == (capi.SR_SEQ_BUDGET, -1)
        assert node_states(h, len(inp.spot)) == states
        compare_plans(o5, p, c5.cand_off)
        assert np.array_equal(p.status, o5["status"]) and np.array_equal(p.node_of_pod, o5["node_of_pod"])
    finally:
        lib.sr_snapshot_destroy(h)
        lib.sr_snapshot_destroy(h5)
    check_sequence(checker, vol)


K0_FORMS = {"default": {}, "k0_every_round": dict(SR_K0_SKIP=0), "k0_whole": dict(SR_K0_INCREMENTAL=0)}


@pytest.mark.parametrize("form", sorted(K0_FORMS))
def test_c5_rounds_with_and_without_k0(form, record_property):
    """The C5 input in full (44 drains): rounds whose tables stand (no K0: the
    commit's nodes ride in the kernel arguments), rounds with the incremental
    K0 and, per environment, K0 in every round / never incremental.  The
    encoder reuses the candidate side from the third identical input."""
    ck = make_checker(**K0_FORMS[form])
    try:
        got = check_sequence(ck, get_input("c5"))
    finally:
        ck.close()
    print("c5 %s: rounds %d, with K0 %d, reused %d" % (form, got.rounds, got.rounds_k0, got.rounds_reused))
    record_property("rounds", got.rounds)
    record_property("rounds_k0", got.rounds_k0)
    record_property("rounds_reused", got.rounds_reused)
    assert got.rounds in (44, 45)
    assert got.rounds_reused >= got.rounds - 3
    if form == "k0_every_round":
        assert got.rounds_k0 == got.rounds
    else:
        assert 1 <= got.rounds_k0 < got.rounds  # rounds with K0 and rounds without


AFFINITY_FORMS = {
    "split_cost": dict(SR_K2_SPLIT_MIN=64, SR_LIST_COST_MIN=0),
    "coop_blocks": dict(SR_LIST_COST_MIN=0, SR_K2_WPB=4, SR_K2_COOP=32),
    "pod_order": dict(SR_K2_MODE=1),
    "general_kernel": dict(SR_K2_NODE_KERNEL=0),
    # the affinity input has domain-path candidates: its list reaches the node-order kernel, and with it the
    # cooperative blocks, only through the split launch
    "coop_split": dict(SR_K2_SPLIT_MIN=64, SR_LIST_COST_MIN=0, SR_K2_WPB=4, SR_K2_COOP=32),
}
DISPATCH_BUDGET = 10


def test_dispatch_budget_has_changed_mappings():
    inp = get_input("c3-affinity")
    ref, _ = inp.reference(DISPATCH_BUDGET)
    assert len(ref.drained) == DISPATCH_BUDGET
    assert divergence(inp, ref)[1] >= 4


@pytest.mark.parametrize("which", sorted(AFFINITY_FORMS))
def test_dispatch_forms(which):
    """The floor in every K2 instance: the split launch with a cost-ordered
    list, cooperative blocks, pod order and the general kernel."""
    ck = make_checker(**AFFINITY_FORMS[which])
    try:
        got = check_sequence(ck, get_input("c3-affinity"), DISPATCH_BUDGET)
        t = ck.timing()
    finally:
        ck.close()
    print("%s: K2 launches %d, by cost %d, cooperative %d" % (which, t.k2_launches, t.k2_list_by_cost, t.k2_coop))
    assert got.rounds == DISPATCH_BUDGET
    if which in ("split_cost", "coop_split"):
        assert t.k2_launches == 2 and t.k2_list_by_cost == 1
    if which == "coop_split":
        assert t.k2_coop > 0


def test_cooperative_blocks_with_far_resolutions():
    """Rows of 10 words (600 spot nodes): the cooperative blocks' helper waves
    scan beyond the 512-node head, beside blocks whose entry is below the floor."""
    inp = from_synth(SynthCluster(3, seed=45, n_on_demand=300, n_spot=600))
    ck = make_checker(SR_LIST_COST_MIN=0, SR_K2_WPB=4, SR_K2_COOP=32)
    try:
        got = check_sequence(ck, inp, DISPATCH_BUDGET)
        t = ck.timing()
    finally:
        ck.close()
    assert got.rounds == len(got.drained) == DISPATCH_BUDGET
    assert t.k2_list_by_cost == 1 and t.k2_coop > 0


def test_floor_does_not_leak(checker):
    """After a sequence, sr_plan and sr_plan_first on a fresh snapshot of the same context equal the oracle in full."""
    inp = get_input("c5")
    check_sequence(checker, inp, 5)
    o = oracle_plan(inp.oracle_snapshot(), inp.ptr, inp.cand_off, inp.cand_pods, mode=1, threads=8)
    o0 = oracle_plan(inp.oracle_snapshot(), inp.ptr, inp.cand_off, inp.cand_pods, mode=0)
    lib = capi.load_planner()
    h = inp.product_snapshot()
    try:
        p = plan_arrays(checker, h, inp.ptr, inp.cand_off, inp.cand_pods)
        compare_plans(o, p, inp.cand_off)
        assert np.array_equal(p.status, o["status"]) and np.array_equal(p.node_of_pod, o["node_of_pod"])
        q = plan_arrays(checker, h, inp.ptr, inp.cand_off, inp.cand_pods, full=False)
        assert (q.first_ok, q.winner) == (p.first_ok, p.winner) and np.array_equal(q.winner_map, p.winner_map)
        n = len(inp.cand_off) - 1
        c = capi.sr_candidates(n, capi.ptr(inp.cand_off, capi.P32), capi.ptr(inp.cand_pods, capi.P32), None)
        status = np.zeros(n, np.int32)
        nodes = np.zeros(int(inp.cand_off[-1]), np.int32)
        wmap = np.full(int(np.max(np.diff(inp.cand_off))), -1, np.int32)
        f = capi.sr_plan_out()
        f.status, f.node_of_pod, f.winner_map = (capi.ptr(status, capi.P32), capi.ptr(nodes, capi.P32),
                                                 capi.ptr(wmap, capi.P32))
        assert lib.sr_plan_first(checker.handle, h, inp.ptr, ctypes.byref(c), ctypes.byref(f)) == capi.SR_OK
        assert f.winner == o0["winner"] and np.array_equal(wmap[:f.winner_npods], o0["winner_map"])
        w = f.winner
        assert np.array_equal(status[:w + 1], o0["status"][:w + 1])
        assert np.array_equal(nodes[:inp.cand_off[w + 1]], o0["node_of_pod"][:inp.cand_off[w + 1]])
    finally:
        lib.sr_snapshot_destroy(h)


def _status_of(ck, inp, h, max_drains=1, first_cand=0, cand_global=None):
    n = len(inp.cand_off) - 1
    c = capi.sr_candidates(n, capi.ptr(inp.cand_off, capi.P32), capi.ptr(inp.cand_pods, capi.P32),
                           capi.ptr(cand_global, capi.P32) if cand_global is not None else None)
    drained = np.full(n, -1, np.int32)
    o = capi.sr_sequence_out()
    o.max_drains, o.first_cand = max_drains, first_cand
    o.drained = capi.ptr(drained, capi.P32)
    st = ck.lib.sr_plan_sequence(ck.handle, h, inp.ptr, ctypes.byref(c), ctypes.byref(o))
    return st, o.n_drained


def test_errors(checker):
    inp = get_input("plain-4")
    lib = capi.load_planner()
    h = inp.product_snapshot()
    try:
        before = node_states(h, len(inp.spot))
        n = len(inp.cand_off) - 1
        assert _status_of(checker, inp, h, max_drains=0) == (capi.SR_ERR_INVALID_ARG, 0)
        assert _status_of(checker, inp, h, first_cand=-1) == (capi.SR_ERR_INVALID_ARG, 0)
        assert _status_of(checker, inp, h, first_cand=n + 1) == (capi.SR_ERR_INVALID_ARG, 0)
        assert _status_of(checker, inp, h, cand_global=np.arange(n, dtype=np.int32)) == (capi.SR_ERR_INVALID_ARG, 0)
        assert lib.sr_snapshot_fork(h) == capi.SR_OK
        assert _status_of(checker, inp, h) == (capi.SR_ERR_STATE, 0)
        assert lib.sr_snapshot_revert(h) == capi.SR_OK
        ck = make_checker()
        try:
            ck.attach_collective(1, 0, lambda words: words)
            assert _status_of(ck, inp, h) == (capi.SR_ERR_STATE, 0)
        finally:
            ck.close()
        assert node_states(h, len(inp.spot)) == before  # no call above touched the snapshot
        assert _status_of(checker, inp, h, first_cand=n) == (capi.SR_OK, 0)  # nothing left to judge
        with pytest.raises(PlannerError):
            plan_sequence_arrays(checker, h, inp.ptr, inp.cand_off, inp.cand_pods, 0)
    finally:
        lib.sr_snapshot_destroy(h)


@pytest.mark.parametrize("seed,kw", [(4, dict(features=False, n_spot=6, n_cand=12, max_pods=6)), (11, {})])
def test_drain_sequence_mirror(checker, seed, kw):
    """rescheduler.drainSequence on Pod / Node objects, in the style of canDrainNode: the plans name the
    reference pass's nodes and the ClusterSnapshot keeps the drained candidates' pods."""
    from randcluster import rand_scenario
    from spotplanner import nodes as N
    from spotplanner.rescheduler import drainSequence
    inp = get_input(("plain-%d" if kw else "features-%d") % seed)
    ref, states = inp.reference(3)
    nodes, spot_pods, cands = rand_scenario(seed, **kw)
    infos = N.NodeInfoArray(N.NodeInfo(n, ps, 0, 0) for n, ps in zip(nodes, spot_pods))
    snapshot = infos.GetClusterSnapshot()
    try:
        r, plans = drainSequence(checker, snapshot, infos, cands, max_drains=3)
        assert [c for c, _ in plans] == list(ref.drained) and r.stop == ref.stop
        assert np.array_equal(r.status, ref.status)
        off = inp.cand_off - inp.cand_off[0]
        for c, names in plans:
            assert names == [nodes[int(k)].name for k in ref.node_of_pod[off[c]:off[c + 1]]]
        assert [snapshot.node_state(n.name) for n in nodes] == states
    finally:
        snapshot.close()


def test_every_candidate_drains_without_a_budget(checker):
    """No budget and room for everything: the pass ends with SR_SEQ_END (not at a budget), one round per drain."""
    inp = from_synth(SynthCluster(1, seed=175, n_on_demand=60, n_spot=200))
    got = check_sequence(checker, inp)
    assert len(got.drained) == len(inp.cand_off) - 1 == 60 and got.stop == capi.SR_SEQ_END
    assert got.rounds == 60
    # the same number of drains as a budget: the pass stops there
    assert check_sequence(checker, inp, 60).stop == capi.SR_SEQ_BUDGET
