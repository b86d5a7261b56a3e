"""sr_plan_sequence_pdb on the CPU: the entry point is exported and bound, the
reference pass (sequence_pdb_ref.py) gives the hand-derived answers of
pdb_cases.py, and the random inputs test_gpu_sequence_pdb.py runs are not
vacuous: on each one a candidate is refused that the oracle finds drainable
below a later drain, a drain lands elsewhere than in the unlimited pass, and
the pass drains after a refusal."""
import ctypes

import numpy as np
import pytest

from pdb_cases import CASES, case_input, case_limits
from sequence_pdb_ref import (PDB, RANDOM_INPUTS, groups_for, masking_groups, pdb_facts, pdb_reference,
                              reference_sequence_pdb)
from sequence_ref import OK, get_input
from spotplanner import capi


def test_sr_plan_sequence_pdb_is_exported_and_bound():
    lib = capi.load_planner()
    assert "sr_plan_sequence_pdb" in capi.EXPORTED
    assert lib.sr_plan_sequence_pdb.restype is ctypes.c_int32 and len(lib.sr_plan_sequence_pdb.argtypes) == 6
    assert len(lib.sr_plan_sequence.argtypes) == 5  # the parent's entry point stays
    assert capi.SR_ABI_VERSION == 11 == lib.sr_abi_version()
    assert capi.SR_CAND_PDB == -5
    P = ctypes.sizeof(ctypes.c_void_p)
    L = capi.sr_pdb_limits
    assert ctypes.sizeof(L) == 4 * P  # an int32 padded to the pointers' alignment, three pointers
    assert (L.n_groups.offset, L.allowed.offset, L.pod_group.offset, L.remaining.offset) == (0, P, 2 * P, 3 * P)
    # 8 int32 and three pointers, as before
    assert ctypes.sizeof(capi.sr_sequence_out) == 32 + 3 * P


def test_error_returns_with_null_handles():
    lib = capi.load_planner()
    o = capi.sr_sequence_out()
    o.max_drains = 1
    c = capi.sr_candidates()
    allowed = np.array([1], np.int32)
    lim = capi.sr_pdb_limits(1, capi.ptr(allowed, capi.P32), None, None)
    for limits in (None, ctypes.byref(lim)):
        assert lib.sr_plan_sequence_pdb(None, None, None, ctypes.byref(c), limits,
                                        ctypes.byref(o)) == capi.SR_ERR_INVALID_ARG
    assert lib.sr_plan_sequence_pdb(None, None, None, None, ctypes.byref(lim), None) == capi.SR_ERR_INVALID_ARG


def test_limits_struct_keeps_its_arrays():
    lim = capi.sr_pdb_limits(2, capi.ptr(np.array([3, 4], np.int32), capi.P32),
                             capi.ptr(np.array([0, 1, -1], np.int32), capi.P32), None)
    import gc
    gc.collect()
    assert [lim.allowed[i] for i in range(2)] == [3, 4] and [lim.pod_group[i] for i in range(3)] == [0, 1, -1]


def _run_case(name, first_cand=0, allowed=None, after=None):
    case, inp = CASES[name], case_input(name)
    a, g = case_limits(name)
    osnap = inp.oracle_snapshot()
    try:
        if after is not None:
            reference_sequence_pdb(osnap, inp.ptr, inp.cand_off, inp.cand_pods, *after)
        return reference_sequence_pdb(osnap, inp.ptr, inp.cand_off, inp.cand_pods, a if allowed is None else allowed,
                                      g, case.max_drains, first_cand, probe=True)
    finally:
        osnap.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_pass_gives_the_hand_derived_answers(name):
    case = CASES[name]
    ref = _run_case(name)
    assert list(ref.drained) == case.drained
    assert (ref.stop, ref.stop_cand) == (case.stop, case.stop_cand)
    assert list(ref.status) == case.status
    assert list(ref.node_of_pod) == case.node_of_pod
    assert list(ref.remaining) == case.remaining
    if case.equals_plain:
        plain, _ = case_input(name).reference()
        assert list(plain.drained) == case.drained and list(plain.status) == case.status
        assert list(plain.node_of_pod) == case.node_of_pod


def test_case_premises():
    """What the cases claim about their refused candidates, on the oracle."""
    assert _run_case("b-refused-though-fits").would == {0: OK}
    assert _run_case("c-last-allowance").would == {1: OK}
    assert _run_case("d-refused-would-fail").would == {0: 0}
    assert _run_case("e-fallbacks").would == {0: capi.SR_CAND_FALLBACK}
    # (b): candidate 1 lands where candidate 0 would have gone, and would not have fitted there beside it
    inp = case_input("b-refused-though-fits")
    plain, _ = inp.reference()
    assert list(plain.status) == [OK, OK] and list(plain.node_of_pod) == [0, 0, 1]


def test_resume_equals_one_uninterrupted_pass():
    """(h): max_drains reached with allowances left, then first_cand = 1 and allowed = remaining."""
    inp = case_input("h-budget-one")
    a, g = case_limits("h-budget-one")
    first = _run_case("h-budget-one")
    assert first.stop == capi.SR_SEQ_BUDGET and np.all(first.remaining > 0)
    second = _run_case("h-uninterrupted", first_cand=1, allowed=first.remaining, after=(a, g, 1, 0))
    whole = CASES["h-uninterrupted"]
    assert list(first.drained) + list(second.drained) == whole.drained
    assert list(first.status[:1]) + list(second.status[1:]) == whole.status
    assert list(np.maximum(first.node_of_pod, second.node_of_pod)) == whole.node_of_pod
    assert list(second.remaining) == whole.remaining


@pytest.mark.parametrize("name", sorted(RANDOM_INPUTS))
def test_random_inputs_are_not_vacuous(name):
    inp = get_input(name)
    allowed, pod_group = groups_for(inp, RANDOM_INPUTS[name])
    assert 3 <= len(allowed) <= 40 and allowed.min() >= 0 and allowed.max() <= 6
    assert len(pod_group) == inp.cand_off[-1] - inp.cand_off[0] and pod_group.min() >= -1
    a2, g2 = groups_for(inp, RANDOM_INPUTS[name])
    assert np.array_equal(allowed, a2) and np.array_equal(pod_group, g2)  # deterministic
    refused, masked, moved, after = pdb_facts(inp, allowed, pod_group)
    print("%s: %d groups, %d refused, %d of them drainable below a later drain, %d drains moved, %d drains after "
          "a refusal" % (name, len(allowed), refused, masked, moved, after))
    assert refused >= 1 and masked >= 1 and moved >= 1 and after >= 1


@pytest.mark.parametrize("name", ["b-refused-though-fits", "c5"])
def test_masking_inputs(name):
    """The refused candidate is the first drainable one from the base snapshot -- the one whose mapping K2
    writes to the host -- and the pass drains a later candidate."""
    if name == "c5":
        inp = get_input(name)
        c, allowed, pod_group = masking_groups(inp)
    else:
        inp, c = case_input(name), 0
        allowed, pod_group = case_limits(name)
    ref, _ = pdb_reference(inp, "masking", allowed, pod_group, probe=True)
    base = inp.base_plan()["status"]
    assert base[c] == OK and not np.any(base[:c] == OK)
    assert ref.status[c] == PDB and ref.would[c] == OK
    assert len(ref.drained) >= 1 and ref.drained[0] > c
    assert np.all(ref.status[c + 1:ref.drained[0]] != OK)  # directly below the round's winner
