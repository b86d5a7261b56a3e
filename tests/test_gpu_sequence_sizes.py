"""sr_plan_sequence and sr_plan_sequence_pdb past the first step of every
size-dependent loop, bit-exact against the reference pass on the oracle: the
ledger kernels' strides (k3_pdb_winner's 1,024 threads, the 16,384 threads of
k3_sequence / k3_pdb_ledger), active indices apart from the caller's, winner
mappings longer than a wave from both publishing paths, K2's large-candidate
paths under a floor, needs lists of hundreds of entries, the default large-list
dispatch and a sliced candidate list.  The inputs are sequence_sizes.py's;
test_sequence_sizes_reference.py asserts on the CPU that they reach that far."""
import ctypes

import numpy as np
import pytest

from oracle_lib import oracle_plan
from sequence_pdb_ref import PDB, RANDOM_INPUTS, groups_for, pdb_reference
from sequence_ref import SKIPPED, get_input
from sequence_sizes import (FALLBACK_AT, KINDS, LADDERS, big_and_later, get_ladder, ladder_limits, large_drains,
                            many_needs, masking_large, sliced)
from spotplanner import capi
from spotplanner.rescheduler import plan_arrays
from test_gpu_parity import compare_plans
from test_gpu_sequence import (assert_equals_reference, check_sequence, make_checker, node_states, record_rounds,
                               run_sequence)
from test_gpu_sequence_pdb import assert_equals_limited, check_limited, run_limited

pytestmark = pytest.mark.gpu


def rounds_of(inp, got):
    """One round per drain, and one more that finds no winner unless the pass ended at its budget or nothing
    with pods is left above the last drain (then no round runs: plan_sequence's loop)."""
    if got.stop == capi.SR_SEQ_BUDGET:
        return len(got.drained)
    last = int(got.drained[-1]) if len(got.drained) else -1
    return len(got.drained) + int(inp.cand_off[-1] > inp.cand_off[last + 1])


@pytest.mark.parametrize("name", sorted(LADDERS))
def test_ladder_plain(checker, name, record_property):
    lad = get_ladder(name)
    got = check_sequence(checker, lad.inp)
    record_rounds(record_property, name, got)
    assert list(got.drained) == lad.caller(sorted(lad.wins + lad.twins))
    # the last active candidate drains: nothing is left for a round after it
    assert got.rounds == rounds_of(lad.inp, got) == len(got.drained)


@pytest.mark.parametrize("name", sorted(LADDERS))
def test_ladder_limited(checker, name, record_property):
    lad = get_ladder(name)
    inp = lad.inp
    allowed, pod_group = ladder_limits(lad)
    got, ref = check_limited(checker, inp, "ladder", allowed, pod_group)
    record_rounds(record_property, name + " limited", got)
    assert list(got.drained) == lad.caller(lad.wins) and list(got.remaining) == [0, 0, 0, 0]
    off = inp.cand_off - inp.cand_off[0]
    for c in lad.caller(lad.twins):
        assert got.status[c] == PDB and np.all(got.node_of_pod[off[c]:off[c + 1]] == -1)
    assert got.rounds == rounds_of(inp, got) == len(got.drained)


def test_ladder_budget_and_resume(checker):
    """A budget of 5 ends at active index 1,024; the second call (first_cand behind it, allowed = remaining, the
    same snapshot and context) starts with its floor above k3_pdb_winner's first step and composes with the
    first one to the uninterrupted pass."""
    lad = get_ladder("ladder-17k")
    inp = lad.inp
    allowed, pod_group = ladder_limits(lad)
    whole, states = pdb_reference(inp, "ladder", allowed, pod_group)
    h = inp.product_snapshot()
    try:
        first = run_limited(checker, inp, h, allowed, pod_group, 5)
        assert first.stop == capi.SR_SEQ_BUDGET and list(first.drained) == list(whole.drained[:5])
        fc = int(first.drained[-1]) + 1
        assert fc > 1024 and np.any(first.remaining > 0)
        second = run_limited(checker, inp, h, first.remaining, pod_group, None, fc)
        assert list(first.drained) + list(second.drained) == list(whole.drained)
        assert np.all(first.status[fc:] == SKIPPED) and np.all(second.status[:fc] == SKIPPED)
        assert list(first.status[:fc]) + list(second.status[fc:]) == list(whole.status)
        assert np.array_equal(np.maximum(first.node_of_pod, second.node_of_pod), whole.node_of_pod)
        assert np.array_equal(second.remaining, whole.remaining)
        assert (second.stop, second.stop_cand) == (whole.stop, whole.stop_cand)
        assert node_states(h, len(inp.spot)) == states
    finally:
        capi.load_planner().sr_snapshot_destroy(h)


def test_ladder_fallback_stop(checker):
    """A reference-path candidate at an active position above 16,384: the plain pass stops at it and the failed
    candidates between the last drain and it carry their status; refused, it is passed over and the pass ends."""
    lad = get_ladder("ladder-17k-fallback")
    inp = lad.inp
    fb = int(lad.active[FALLBACK_AT])
    got = check_sequence(checker, inp)
    assert (got.stop, got.stop_cand) == (capi.SR_SEQ_FALLBACK, fb)
    last = int(got.drained[-1])
    assert np.all(got.status[last + 1:fb] >= 0) and np.all(got.status[fb + 1:] == SKIPPED)
    assert got.rounds == len(got.drained) + 1
    allowed, pod_group = ladder_limits(lad, also_refused=[FALLBACK_AT])
    lim, _ = check_limited(checker, inp, "ladder-fb", allowed, pod_group)
    assert lim.status[fb] == PDB and (lim.stop, lim.stop_cand) == (capi.SR_SEQ_END, -1)
    assert list(lim.drained) == lad.caller(lad.wins) and np.all(lim.status[fb + 1:] >= 0)
    assert lim.rounds == len(lim.drained) + 1


@pytest.mark.parametrize("name", sorted(LADDERS))
def test_ladder_default_dispatch(name, record_property):
    """No threshold lowered: the lists are long enough for the cost-ordered work list (above 1,024 entries; the
    first two rounds of a planner record the durations and build the reuse index, the third reorders), four
    waves per block (above 2,048) and, with domain-path candidates, the split launch (above 4,096).  The
    timing describes the sequence's last round."""
    lad = get_ladder(name)
    allowed, pod_group = ladder_limits(lad)
    ck = make_checker()
    try:
        got, _ = check_limited(ck, lad.inp, "ladder", allowed, pod_group)
        t = ck.timing()
    finally:
        ck.close()
    print("%s: rounds %d, reused %d, K2 launches %d, by cost %d, cooperative %d" % (
        name, got.rounds, got.rounds_reused, t.k2_launches, t.k2_list_by_cost, t.k2_coop))
    for key in ("k2_launches", "k2_list_by_cost", "k2_coop"):
        record_property(key, getattr(t, key))
    assert got.rounds >= 4  # (reordered from the third round on)
    assert t.k2_list_by_cost == 1
    assert t.k2_launches == (2 if name == "ladder-4200-domain" else 1)


def first_winner(ck, inp, h, start=0):
    """sr_plan_first of the candidates from `start` on: (the winner in the caller's indices, its mapping)."""
    n = len(inp.cand_off) - 1 - start
    cand_off = np.ascontiguousarray(inp.cand_off[start:])
    c = capi.sr_candidates(n, capi.ptr(cand_off, capi.P32), capi.ptr(inp.cand_pods, capi.P32), None)
    wmap = np.full(int(np.max(np.diff(inp.cand_off))), -1, np.int32)
    o = capi.sr_plan_out()
    o.winner_map = capi.ptr(wmap, capi.P32)
    assert capi.load_planner().sr_plan_first(ck.handle, h, inp.ptr, ctypes.byref(c), ctypes.byref(o)) == capi.SR_OK
    assert o.winner >= 0
    return start + o.winner, wmap[:o.winner_npods].copy()


FORMS = {"default": {}, "pod_order": dict(SR_K2_MODE=1), "one_plan_slot": dict(SR_PLAN_SLOTS=1),
         "k0_every_round": dict(SR_K0_SKIP=0)}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kind", KINDS)
def test_large_drains(kind, form, record_property):
    inp = large_drains(kind)
    full, _ = inp.reference()
    off = inp.cand_off - inp.cand_off[0]
    ck = make_checker(**FORMS[form])
    try:
        got = check_sequence(ck, inp)
        record_rounds(record_property, "large %s %s" % (kind, form), got)
        assert got.rounds == rounds_of(inp, got)
        if form == "k0_every_round":
            assert got.rounds_k0 == got.rounds
        # budgets 1 and 2: the last drain's mapping, a word per pod through K2's own publishing, is
        # sr_plan_first's winner_map from the state the drain met
        for budget in (1, 2):
            part = check_sequence(ck, inp, budget)
            assert list(part.drained) == list(full.drained[:budget]) and part.stop == capi.SR_SEQ_BUDGET
            h = inp.product_snapshot()
            try:
                start = 0
                if budget == 2:
                    assert list(run_sequence(ck, inp, h, 1).drained) == [full.drained[0]]
                    start = int(full.drained[0]) + 1
                w, wmap = first_winner(ck, inp, h, start)
            finally:
                capi.load_planner().sr_snapshot_destroy(h)
            assert w == part.drained[-1] and len(wmap) == off[w + 1] - off[w] >= 64
            assert np.array_equal(part.node_of_pod[off[w]:off[w + 1]], wmap)
    finally:
        ck.close()


@pytest.mark.parametrize("which", ["needs", "needs_last", "masking"])
@pytest.mark.parametrize("kind", ["plain", "domain"])
def test_large_drains_limited(checker, kind, which):
    """needs: 512 needs committed at equality, and a 64-pod candidate behind it refused by needs that are not
    its first while a later candidate keeps the round running; needs_last: the 512-pod candidate refused by the
    last of its 512 needs alone; masking: a refused drainable candidate of more than 128 pods directly below a
    winner of more than 128 pods, whose words only the ledger step publishes."""
    inp = large_drains(kind)
    sizes = np.diff(inp.cand_off)
    big, other = big_and_later(inp)
    if which == "masking":
        plain, _ = inp.reference()
        c, allowed, pod_group = masking_large(inp, plain)
        budget = int(np.sum(plain.drained < c)) + 1  # the drains below c, and the one that passes over it
        got, _ = check_limited(checker, inp, "masking-large", allowed, pod_group, budget)
        w = int(got.drained[-1])
        assert got.status[c] == PDB and sizes[c] > 128 and w > c and sizes[w] > 128
        assert got.rounds == budget
        check_limited(checker, inp, "masking-large", allowed, pod_group)  # and the whole pass behind it
        return
    allowed, pod_group = many_needs(inp, refuse_last=which == "needs_last")
    got, _ = check_limited(checker, inp, ("needs", which == "needs_last"), allowed, pod_group)
    if which == "needs_last":
        assert list(np.nonzero(got.status == PDB)[0]) == [big] and got.drained[-1] > big
    else:
        assert big in got.drained and np.all(got.remaining[1:] == 0)
        assert got.status[other] == (PDB if other > big else capi.SR_CAND_OK)


def test_sliced_candidate_list(checker):
    """cand_pod_off[0] == 37: the results are those of the same candidates at offset 0, in sr_plan_sequence,
    sr_plan_sequence_pdb, sr_plan and sr_plan_first."""
    lib = capi.load_planner()
    for inp, (allowed, pod_group) in ((large_drains("plain"), many_needs(large_drains("plain"))),
                                      (get_input("features-11"),
                                       groups_for(get_input("features-11"), RANDOM_INPUTS["features-11"]))):
        s = sliced(inp)
        assert s.cand_off[0] == 37
        n_pods = int(inp.cand_off[-1] - inp.cand_off[0])
        ref, states = inp.reference()
        lim, lim_states = pdb_reference(inp, "sliced", allowed, pod_group)
        h = s.product_snapshot()
        try:
            got = run_sequence(checker, s, h)
            assert_equals_reference(s, h, got, ref, states)
        finally:
            lib.sr_snapshot_destroy(h)
        h = s.product_snapshot()
        try:
            got = run_limited(checker, s, h, allowed, pod_group)
            assert_equals_limited(s, h, got, lim, lim_states)
        finally:
            lib.sr_snapshot_destroy(h)
        h = s.product_snapshot()
        try:
            o = inp.base_plan()
            p = plan_arrays(checker, h, s.ptr, s.cand_off, s.cand_pods)
            compare_plans(o, p, s.cand_off - s.cand_off[0])
            u = plan_arrays(checker, h, inp.ptr, inp.cand_off, inp.cand_pods)  # the unsliced list
            assert np.array_equal(p.status, u.status) and np.array_equal(p.node_of_pod[:n_pods], u.node_of_pod)
            assert p.winner == u.winner >= 0 and np.array_equal(p.winner_map, u.winner_map)
            w, wmap = first_winner(checker, s, h)
            assert w == p.winner and np.array_equal(wmap, p.winner_map)
        finally:
            lib.sr_snapshot_destroy(h)


def test_no_state_leaks_after_large(checker):
    """A limited sequence over 16,900 candidates, then a small limited one and an sr_plan on the same context:
    the ledger, the needs and the refused flags shrink in use, not in size."""
    lad = get_ladder("ladder-17k")
    allowed, pod_group = ladder_limits(lad)
    check_limited(checker, lad.inp, "ladder", allowed, pod_group)
    small = get_input("plain-4")
    a4, g4 = groups_for(small, RANDOM_INPUTS["plain-4"])
    got, _ = check_limited(checker, small, "random", a4, g4)
    assert np.any(got.status == PDB) and len(got.drained) >= 1
    c5 = get_input("c5")
    o = oracle_plan(c5.oracle_snapshot(), c5.ptr, c5.cand_off, c5.cand_pods, mode=1, threads=8)
    h = c5.product_snapshot()
    try:
        p = plan_arrays(checker, h, c5.ptr, c5.cand_off, c5.cand_pods)
        compare_plans(o, p, c5.cand_off)
        assert np.array_equal(p.status, o["status"]) and np.array_equal(p.node_of_pod, o["node_of_pod"])
    finally:
        capi.load_planner().sr_snapshot_destroy(h)
