"""sr_plan_sequence on the CPU: the entry point is exported and bound, and the
inputs the GPU tests (test_gpu_sequence.py) run meet their preconditions on
the oracle -- above all that the commits matter: on an input where every
candidate drainable from the base snapshot also drains in sequence, an
implementation that never commits would pass."""
import ctypes

import numpy as np
import pytest

from oracle_lib import oracle_plan
from sequence_ref import BUILDERS, FALLBACK_STOPS, OK, SKIPPED, divergence, from_synth, get_input, reference_sequence
from spotplanner import capi
from spotplanner.synth import SynthCluster


def test_sr_plan_sequence_is_exported_and_bound():
    lib = capi.load_planner()
    assert "sr_plan_sequence" in capi.EXPORTED
    assert lib.sr_plan_sequence.restype is ctypes.c_int32 and len(lib.sr_plan_sequence.argtypes) == 5
    assert capi.SR_ABI_VERSION >= 10
    assert (capi.SR_SEQ_END, capi.SR_SEQ_BUDGET, capi.SR_SEQ_FALLBACK) == (0, 1, 2)
    o = capi.sr_sequence_out()
    o.max_drains = 1
    c = capi.sr_candidates()
    assert lib.sr_plan_sequence(None, None, None, ctypes.byref(c), ctypes.byref(o)) == capi.SR_ERR_INVALID_ARG
    # 8 int32 (padded to the pointers' alignment) and three pointers
    assert ctypes.sizeof(capi.sr_sequence_out) == 32 + 3 * ctypes.sizeof(ctypes.c_void_p)


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_budget_one_is_the_reference_tick(name):
    """With max_drains = 1 the pass is run()'s own loop: oracle_plan(mode=0)'s winner and mapping."""
    inp = get_input(name)
    ref, _ = inp.reference(1)
    o = oracle_plan(inp.oracle_snapshot(), inp.ptr, inp.cand_off, inp.cand_pods, mode=0)
    assert o["winner"] >= 0
    assert list(ref.drained) == [o["winner"]] and ref.stop == capi.SR_SEQ_BUDGET
    w = o["winner"]
    off = inp.cand_off - inp.cand_off[0]
    assert np.array_equal(ref.node_of_pod[off[w]:off[w + 1]], o["winner_map"])
    assert np.all(ref.status[w + 1:] == SKIPPED)


@pytest.mark.parametrize("name", sorted(n for n in BUILDERS if not n.startswith("fallback")))
def test_commits_matter(name):
    """Some judged candidate's status or mapping differs from its plan on the base snapshot."""
    inp = get_input(name)
    ref, _ = inp.reference()
    assert ref.stop == capi.SR_SEQ_END and ref.stop_cand == -1
    assert len(ref.drained) >= 2
    assert np.all(np.diff(ref.drained) > 0)
    assert divergence(inp, ref)[3] >= 1
    if name.startswith("plain"):
        assert 3 <= len(ref.drained) <= 5


def test_synthetic_inputs_diverge_as_recorded():
    ref, _ = get_input("c5").reference()
    fail_now, maps, _, _ = divergence(get_input("c5"), ref)
    assert (len(ref.drained), fail_now, maps) == (44, 56, 42)
    assert len(get_input("c5").spot) == 200  # rows of 4 words
    ref, _ = get_input("c3-affinity").reference()
    assert (len(ref.drained), divergence(get_input("c3-affinity"), ref)[1]) == (42, 38)
    ref, _ = get_input("c3-tight").reference()
    assert (len(ref.drained), divergence(get_input("c3-tight"), ref)[2]) == (38, 20)


def test_full_size_like_c3_is_no_sequence_input():
    """Every candidate it drains in sequence is also drainable from the base snapshot: not used on the GPU."""
    inp = from_synth(SynthCluster(3, seed=41, n_on_demand=300, n_spot=600))
    ref = reference_sequence(inp.oracle_snapshot(), inp.ptr, inp.cand_off, inp.cand_pods)
    assert len(ref.drained) == 31
    assert np.all(inp.base_plan()["status"][ref.drained] == OK)
    assert divergence(inp, ref)[0] == 0


@pytest.mark.parametrize("seed", sorted(FALLBACK_STOPS))
def test_fallback_inputs_stop_after_two_drains(seed):
    ref, _ = get_input("fallback-%d" % seed).reference()
    assert len(ref.drained) == 2
    assert (ref.stop, ref.stop_cand) == (capi.SR_SEQ_FALLBACK, FALLBACK_STOPS[seed])
    assert np.all(ref.status[ref.stop_cand + 1:] == SKIPPED)
