"""sr_plan_sequence_pdb on the GPU against the reference pass on the oracle
(sequence_pdb_ref.py): the drains, the stop, every candidate's status and
mapping, what each group still allows and the snapshot the pass leaves, on the
hand-derived cases (pdb_cases.py) and the random inputs whose preconditions
test_sequence_pdb_reference.py asserts on the CPU."""
import ctypes

import numpy as np
import pytest

from oracle_lib import oracle_plan
from pdb_cases import CASES, case_input, case_limits
from sequence_pdb_ref import PDB, RANDOM_INPUTS, groups_for, masking_groups, pdb_reference, reference_sequence_pdb
from sequence_ref import get_input
from spotplanner import capi
from spotplanner.planner import PlannerError
from spotplanner.rescheduler import PdbLimits, plan_arrays, plan_sequence_arrays
from test_gpu_parity import compare_plans
from test_gpu_sequence import assert_equals_reference, make_checker, node_states, record_rounds

pytestmark = pytest.mark.gpu


def run_limited(ck, inp, h, allowed, pod_group, max_drains=None, first_cand=0):
    return plan_sequence_arrays(ck, h, inp.ptr, inp.cand_off, inp.cand_pods, max_drains, first_cand,
                                limits=PdbLimits(allowed, pod_group))


def assert_equals_limited(inp, h, got, ref, states):
    assert_equals_reference(inp, h, got, ref, states)  # drained, stop, stop_cand, status, node_of_pod, node states
    assert np.array_equal(got.remaining, ref.remaining), (got.remaining, ref.remaining)
    off = inp.cand_off - inp.cand_off[0]
    for c in np.nonzero(ref.status == PDB)[0]:  # a refused candidate is never planned
        assert np.all(got.node_of_pod[off[c]:off[c + 1]] == -1)


def check_limited(ck, inp, key, allowed, pod_group, max_drains=None):
    ref, states = pdb_reference(inp, key, allowed, pod_group, max_drains)
    h = inp.product_snapshot()
    try:
        got = run_limited(ck, inp, h, allowed, pod_group, max_drains)
        assert_equals_limited(inp, h, got, ref, states)
    finally:
        capi.load_planner().sr_snapshot_destroy(h)
    return got, ref


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_derived_cases(checker, name):
    case, inp = CASES[name], case_input(name)
    allowed, pod_group = case_limits(name)
    got, _ = check_limited(checker, inp, "case", allowed, pod_group, case.max_drains)
    # ... and the answers written out in pdb_cases.py themselves
    assert list(got.drained) == case.drained and (got.stop, got.stop_cand) == (case.stop, case.stop_cand)
    assert list(got.status) == case.status and list(got.node_of_pod) == case.node_of_pod
    assert list(got.remaining) == case.remaining
    if case.rounds is not None:
        assert got.rounds == case.rounds


def test_resume_equals_one_uninterrupted_pass(checker):
    """(h): max_drains reached with allowances left, then first_cand and allowed = remaining on the same snapshot."""
    inp = case_input("h-budget-one")
    allowed, pod_group = case_limits("h-budget-one")
    whole, states = pdb_reference(case_input("h-uninterrupted"), "case", allowed, pod_group)
    h = inp.product_snapshot()
    try:
        first = run_limited(checker, inp, h, allowed, pod_group, 1)
        assert first.stop == capi.SR_SEQ_BUDGET and list(first.remaining) == CASES["h-budget-one"].remaining
        second = run_limited(checker, inp, h, first.remaining, pod_group, None, int(first.drained[-1]) + 1)
        assert list(first.drained) + list(second.drained) == list(whole.drained)
        assert list(first.status[:1]) + list(second.status[1:]) == list(whole.status)
        assert np.array_equal(np.maximum(first.node_of_pod, second.node_of_pod), whole.node_of_pod)
        assert np.array_equal(second.remaining, whole.remaining)
        assert node_states(h, len(inp.spot)) == states
    finally:
        capi.load_planner().sr_snapshot_destroy(h)


@pytest.mark.parametrize("name", sorted(RANDOM_INPUTS))
def test_random_inputs_match_reference_pass(checker, name):
    inp = get_input(name)
    allowed, pod_group = groups_for(inp, RANDOM_INPUTS[name])
    got, ref = check_limited(checker, inp, "random", allowed, pod_group)
    assert np.any(got.status == PDB) and len(got.drained) >= 1


@pytest.mark.parametrize("name", sorted(RANDOM_INPUTS))
def test_no_limits_is_sr_plan_sequence(checker, name):
    """limits = NULL, n_groups = 0 and allowances that never bind: sr_plan_sequence's outputs, rounds included."""
    inp = get_input(name)
    ref, states = inp.reference()
    lib = capi.load_planner()
    n = len(inp.cand_off) - 1
    n_pods = int(inp.cand_off[-1] - inp.cand_off[0])
    _, pod_group = groups_for(inp, RANDOM_INPUTS[name])
    h = inp.product_snapshot()
    try:
        plain = plan_sequence_arrays(checker, h, inp.ptr, inp.cand_off, inp.cand_pods)
        assert_equals_reference(inp, h, plain, ref, states)
    finally:
        lib.sr_snapshot_destroy(h)

    def raw(limits):
        hh = inp.product_snapshot()
        try:
            c = capi.sr_candidates(n, capi.ptr(inp.cand_off, capi.P32), capi.ptr(inp.cand_pods, capi.P32), None)
            drained, status = np.full(n, -1, np.int32), np.full(n, 99, np.int32)
            nodes = np.full(n_pods, 99, np.int32)
            o = capi.sr_sequence_out()
            o.max_drains = 2 ** 31 - 1
            o.drained, o.status, o.node_of_pod = (capi.ptr(drained, capi.P32), capi.ptr(status, capi.P32),
                                                  capi.ptr(nodes, capi.P32))
            st = lib.sr_plan_sequence_pdb(checker.handle, hh, inp.ptr, ctypes.byref(c), limits, ctypes.byref(o))
            assert st == capi.SR_OK, checker.last_error()
            assert list(drained[:o.n_drained]) == list(plain.drained)
            assert (o.stop, o.stop_cand, o.rounds) == (plain.stop, plain.stop_cand, plain.rounds)
            assert np.array_equal(status, plain.status) and np.array_equal(nodes, plain.node_of_pod)
            assert node_states(hh, len(inp.spot)) == states
        finally:
            lib.sr_snapshot_destroy(hh)

    raw(None)
    raw(ctypes.byref(capi.sr_pdb_limits(0, None, None, None)))
    h = inp.product_snapshot()
    try:
        loose = run_limited(checker, inp, h, np.full(int(pod_group.max()) + 1, 2 ** 30, np.int32), pod_group)
        assert_equals_reference(inp, h, loose, ref, states)
        assert loose.rounds == plain.rounds
        spent = np.bincount(_drained_groups(inp, pod_group, loose.drained), minlength=len(loose.remaining))
        assert np.array_equal(2 ** 30 - loose.remaining, spent)
    finally:
        lib.sr_snapshot_destroy(h)


def _drained_groups(inp, pod_group, drained):
    off = inp.cand_off - inp.cand_off[0]
    g = np.concatenate([pod_group[off[c]:off[c + 1]] for c in drained] + [np.zeros(0, np.int32)])
    return g[g >= 0]


@pytest.mark.parametrize("name", ["b-refused-though-fits", "c5"])
def test_masking(checker, name):
    """A refused, drainable candidate directly below the round's winner: K2's first drainable candidate, the only
    one whose mapping K2 itself sends to the host, is the refused one, so the winner's mapping can only come
    from the ledger step's words (test_sequence_pdb_reference.py::test_masking_inputs holds the premise)."""
    if name == "c5":
        inp = get_input(name)
        c, allowed, pod_group = masking_groups(inp)
    else:
        inp, c = case_input(name), 0
        allowed, pod_group = case_limits(name)
    got, ref = check_limited(checker, inp, "masking", allowed, pod_group, 1)
    w = int(ref.drained[0])
    off = inp.cand_off - inp.cand_off[0]
    assert got.status[c] == PDB and list(got.drained) == [w] and w > c
    assert np.array_equal(got.node_of_pod[off[w]:off[w + 1]], ref.node_of_pod[off[w]:off[w + 1]])
    assert got.rounds == 1
    check_limited(checker, inp, "masking", allowed, pod_group)  # and the whole pass behind it


PDB_FORMS = {"default": {}, "pod_order": dict(SR_K2_MODE=1), "one_plan_slot": dict(SR_PLAN_SLOTS=1),
             "k0_every_round": dict(SR_K0_SKIP=0)}


@pytest.mark.parametrize("budget", [1, 2, None])
@pytest.mark.parametrize("form", sorted(PDB_FORMS))
def test_realistic_budgets_and_forms(form, budget, record_property):
    inp = get_input("realistic-80")
    allowed, pod_group = groups_for(inp, RANDOM_INPUTS["realistic-80"])
    ck = make_checker(**PDB_FORMS[form])
    try:
        got, ref = check_limited(ck, inp, "random", allowed, pod_group, budget)
    finally:
        ck.close()
    record_rounds(record_property, "realistic-80 pdb %s budget %s" % (form, budget), got)
    if budget is not None:
        assert len(got.drained) == budget and got.stop == capi.SR_SEQ_BUDGET
    if form == "k0_every_round":
        assert got.rounds_k0 == got.rounds


def test_no_state_leaks(checker):
    """A limited call, then on the same context a plain sr_plan_sequence of the same input and an sr_plan of
    another one: both are the oracle's (the floor, the allowances and the result words stay with their call)."""
    inp, other = get_input("vol-11"), get_input("c5")
    allowed, pod_group = groups_for(inp, RANDOM_INPUTS["vol-11"])
    check_limited(checker, inp, "random", allowed, pod_group)
    ref, states = inp.reference()
    lib = capi.load_planner()
    h, ho = inp.product_snapshot(), other.product_snapshot()
    try:
        got = plan_sequence_arrays(checker, h, inp.ptr, inp.cand_off, inp.cand_pods)
        assert_equals_reference(inp, h, got, ref, states)
        assert not np.any(got.status == PDB) and got.remaining is None
        o = oracle_plan(other.oracle_snapshot(), other.ptr, other.cand_off, other.cand_pods, mode=1, threads=8)
        p = plan_arrays(checker, ho, other.ptr, other.cand_off, other.cand_pods)
        compare_plans(o, p, other.cand_off)
        assert np.array_equal(p.status, o["status"]) and np.array_equal(p.node_of_pod, o["node_of_pod"])
    finally:
        lib.sr_snapshot_destroy(h)
        lib.sr_snapshot_destroy(ho)
    check_limited(checker, inp, "random", allowed, pod_group)  # and a limited call after them


def test_errors(checker):
    inp = case_input("c-last-allowance")
    allowed, pod_group = case_limits("c-last-allowance")
    lib = capi.load_planner()
    n = len(inp.cand_off) - 1
    h = inp.product_snapshot()

    def call(n_groups, a, g, **kw):
        c = capi.sr_candidates(n, capi.ptr(inp.cand_off, capi.P32), capi.ptr(inp.cand_pods, capi.P32), None)
        drained = np.full(n, -1, np.int32)
        remaining = np.full(8, 77, np.int32)
        o = capi.sr_sequence_out()
        o.max_drains, o.first_cand = kw.get("max_drains", 5), kw.get("first_cand", 0)
        o.drained = capi.ptr(drained, capi.P32)
        lim = capi.sr_pdb_limits(n_groups, capi.ptr(a, capi.P32) if a is not None else None,
                                 capi.ptr(g, capi.P32) if g is not None else None, capi.ptr(remaining, capi.P32))
        st = lib.sr_plan_sequence_pdb(checker.handle, h, inp.ptr, ctypes.byref(c), ctypes.byref(lim), ctypes.byref(o))
        return st, o.n_drained, list(remaining)

    try:
        before = node_states(h, len(inp.spot))
        untouched = [77] * 8
        bad = capi.SR_ERR_INVALID_ARG
        assert call(-1, allowed, pod_group) == (bad, 0, untouched)
        assert call(2, None, pod_group) == (bad, 0, untouched)
        assert call(2, allowed, None) == (bad, 0, untouched)
        assert call(2, np.array([1, -1], np.int32), pod_group) == (bad, 0, untouched)
        assert call(2, allowed, np.array([0, 2, 1], np.int32)) == (bad, 0, untouched)
        assert call(2, allowed, np.array([0, -2, 1], np.int32)) == (bad, 0, untouched)
        # sr_plan_sequence's own rules
        assert call(2, allowed, pod_group, max_drains=0)[:2] == (bad, 0)
        assert call(2, allowed, pod_group, first_cand=n + 1)[:2] == (bad, 0)
        assert lib.sr_snapshot_fork(h) == capi.SR_OK
        assert call(2, allowed, pod_group)[:2] == (capi.SR_ERR_STATE, 0)
        assert lib.sr_snapshot_revert(h) == capi.SR_OK
        assert node_states(h, len(inp.spot)) == before  # no commit on an argument error
        with pytest.raises(PlannerError):
            run_limited(checker, inp, h, np.array([1, -1], np.int32), pod_group)
        assert node_states(h, len(inp.spot)) == before
        st, n_drained, remaining = call(2, allowed, pod_group)  # and the same arrays, valid: case (c)
        assert (st, n_drained, remaining[:2]) == (capi.SR_OK, 2, CASES["c-last-allowance"].remaining)
    finally:
        lib.sr_snapshot_destroy(h)
