"""sr_plan_sequence on the CPU: the entry point is exported and bound, and the
inputs the GPU tests (test_gpu_sequence.py) run meet their preconditions on
the oracle -- above all that the commits matter: on an input where every
candidate drainable from the base snapshot also drains in sequence, an
implementation that never commits would pass."""
import ctypes

import numpy as np
import pytest

from oracle_lib import oracle_plan
from sequence_ref import (BUILDERS, DYNAMIC_STOPS, EMPTY, FALLBACK_STOPS, FB, FLIP_ROUND, OK, RECORDED, SKIPPED,
                          VOLFLIP, divergence, from_synth, get_input, reference_sequence)
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


def _stops_at_fallback(name):
    return name.startswith("fallback") or (name in RECORDED and RECORDED[name][1] == capi.SR_SEQ_FALLBACK)


@pytest.mark.parametrize("name", sorted(n for n in BUILDERS if not _stops_at_fallback(n)))
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


@pytest.mark.parametrize("name", sorted(RECORDED))
def test_volume_spread_and_extension_inputs_as_recorded(name):
    """The drains, the stop and the divergence from the base plan of the inputs with volumes, spread constraints
    and extension records, exactly; a dynamic stop's candidate is planned from the base snapshot."""
    inp = get_input(name)
    ref, _ = inp.reference()
    drains, stop, stop_cand, div = RECORDED[name]
    assert (len(ref.drained), ref.stop, ref.stop_cand) == (drains, stop, stop_cand)
    if div is not None:
        assert tuple(int(x) for x in divergence(inp, ref)) == div
    base = inp.base_plan()["status"]
    if name in DYNAMIC_STOPS:
        assert base[stop_cand] != FB and not np.any(base == FB)
        assert ref.status[stop_cand] == FB and np.all(ref.status[stop_cand + 1:] == SKIPPED)
        flips = []  # is the stop candidate FALLBACK from the snapshot k drains leave?
        for k in range(drains + 1):
            osnap = inp.oracle_snapshot()
            if k:
                reference_sequence(osnap, inp.ptr, inp.cand_off, inp.cand_pods, k)
            flips.append(oracle_plan(osnap, inp.ptr, inp.cand_off, inp.cand_pods, mode=1)["status"][stop_cand] == FB)
            osnap.close()
        assert flips.index(True) + 1 == FLIP_ROUND[name] and all(flips[FLIP_ROUND[name] - 1:])
    elif stop == capi.SR_SEQ_FALLBACK:
        assert base[stop_cand] == FB  # static
    if name in VOLFLIP:
        assert np.all(base == OK)
        assert list(ref.drained) == [0, 1, 2, 3, 4]
        assert list(ref.status) == [OK, OK, OK, OK, OK, FB, SKIPPED] == [-1, -1, -1, -1, -1, -2, -4]


def _arr(p, n):
    return np.ctypeslib.as_array(p, shape=(n,))


def extension_record_candidates(inp, judged):
    """The judged candidates with a reason for extension records, read off the cluster arrays: (candidates with a
    pod whose AddPod accounting differs from its fit request and which is not the candidate's last pod,
    candidates where two pods list one scalar name or one volume-limit key, candidates with either)."""
    cl = inp.keep[0].cluster
    n = cl.pods.n
    differs = np.zeros(n, bool)
    for req, acc in ((cl.pods.req_milli_cpu, cl.acc_milli_cpu), (cl.pods.req_memory, cl.acc_memory),
                     (cl.pods.req_ephemeral, cl.acc_ephemeral)):
        differs |= _arr(req, n) != _arr(acc, n)
    s_off = _arr(cl.pod_scalar_off, n + 1)
    s_name = _arr(cl.pod_scalar_name, max(1, int(s_off[-1])))
    v = cl.volumes.contents
    a_off = _arr(v.att_off, n + 1)
    a_key = _arr(v.att_key, max(1, int(a_off[-1])))
    init = shared = either = 0
    for c in judged:
        pods = inp.cand_pods[inp.cand_off[c]:inp.cand_off[c + 1]]
        by_init = bool(np.any(differs[pods[:-1]]))
        seen, by_shared = set(), False
        for p in pods:
            names = {("scalar", int(x)) for x in s_name[s_off[p]:s_off[p + 1]]}
            names |= {("limit", int(x)) for x in a_key[a_off[p]:a_off[p + 1]]}
            by_shared |= bool(names & seen)
            seen |= names
        init += by_init
        shared += by_shared
        either += by_init or by_shared
    return init, shared, either


def test_realistic_80_has_extension_record_candidates():
    """The forms of test_gpu_sequence.py run realistic-80 for its extension records: at least 20 of its judged
    candidates have a reason for them (a guard for the witness, not a measurement)."""
    inp = get_input("realistic-80")
    ref, _ = inp.reference()
    judged = [c for c in range(len(ref.status)) if ref.status[c] not in (SKIPPED, FB, EMPTY)]
    init, shared, either = extension_record_candidates(inp, judged)
    print("realistic-80: %d judged, init accounting %d, shared names %d, either %d" % (len(judged), init, shared,
                                                                                      either))
    assert either >= 20


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
