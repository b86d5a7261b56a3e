"""K2's 64-bit state word at its high bits and at its 64 / 65-bit limit on the
GPU: every call of state_word.py through sr_plan, the winner-only run and
sr_plan_first under nine planner forms, bit-exact against the hand-derived
plans (status, node_of_pod, winner, first_ok, first_fallback, fallback_pods).
The expected values are state_word.py's own; test_state_word_reference.py has
proved them on the oracle, shown with each twin that the bit is what decides,
and checked the bit positions on the encoder's host view -- nothing here is
recomputed from the planner.  SR_CAND_FALLBACK is accepted only where a case
lists it.  A planner that drops the word's high half in fits32 or in the
exclusive step, swaps pairs with a 32-bit constant, wraps swap_mask at 64,
tests ports on the low half in the pod-order or the domain path, or moves the
overflow test by one fails here."""
import numpy as np
import pytest

import state_word as S
from sequence_ref import from_scenario
from spotplanner import capi
from spotplanner.rescheduler import plan_arrays
from test_gpu_sequence import check_sequence, make_checker
from test_gpu_ticks import plan_first

pytestmark = pytest.mark.gpu

FORMS = {
    "default": {},
    "narrow_off": dict(SR_K2_NARROW=0),          # 64-bit place_window
    "excl_off": dict(SR_K2_EXCL=0),              # the non-X step for exclusive candidates
    "pod_order": dict(SR_K2_MODE=1),
    "general_kernel": dict(SR_K2_NODE_KERNEL=0),
    "wpb4": dict(SR_K2_WPB=4),
    # cooperative blocks (without the init-container case: a launch with extension records has none)
    "coop": dict(SR_LIST_COST_MIN=0, SR_K2_WPB=4, SR_K2_COOP=4096),
    "one_plan_slot": dict(SR_PLAN_SLOTS=1),
    "k0_every_call": dict(SR_K0_SKIP=0),
}
CALLS = [(name, form) for name in sorted(S.CASES) for form in FORMS if not (form == "coop" and name in S.EXT_CASES)]


@pytest.fixture(scope="module")
def planners():
    """One planner per form for the whole module: the calls follow one another on it."""
    made = {}

    def get(form):
        if form not in made:
            made[form] = make_checker(**FORMS[form])
        return made[form]

    yield get
    for ck in made.values():
        ck.close()


def run_call(ck, inp, drop=(), fillers=(), want=None):
    """One call through sr_plan (every output, then the winner only) and sr_plan_first against the hand-derived
    values; returns the first run's timing."""
    cands, _, cand_off, cand_pods = inp.arrays(drop)
    status, nodes, first_ok, first_fb, winner, fb_pods = S.expected(cands, want)
    lib = capi.load_planner()
    h = inp.sc.product_snapshot()
    try:
        for pod, pos in fillers:
            assert lib.sr_snapshot_add_pod(h, inp.sc.ptr, pod, pos) == capi.SR_OK
        p = plan_arrays(ck, h, inp.sc.ptr, cand_off, cand_pods)
        t = ck.timing()
        q = plan_arrays(ck, h, inp.sc.ptr, cand_off, cand_pods, full=False)
        f, f_status, f_nodes, f_map = plan_first(ck, h, inp.sc.ptr, cand_off, cand_pods)
    finally:
        lib.sr_snapshot_destroy(h)
    planned = np.repeat(status != S.FB, np.diff(cand_off))
    assert list(p.status) == list(status), (list(p.status), list(status))
    bad = np.flatnonzero((p.node_of_pod != nodes) & planned)
    assert bad.size == 0, (bad[:8], p.node_of_pod[bad[:8]], nodes[bad[:8]])
    assert (p.winner, p.first_ok, p.first_fallback, p.fallback_pods) == (winner, first_ok, first_fb, fb_pods)
    seg = slice(int(cand_off[first_ok]), int(cand_off[first_ok + 1])) if first_ok >= 0 else slice(0, 0)
    assert list(p.winner_map) == list(nodes[seg])  # the first drainable candidate's, winner or not
    assert (q.winner, q.first_ok, q.first_fallback) == (winner, first_ok, first_fb)
    assert list(q.winner_map) == list(p.winner_map)
    # sr_plan_first stops at the first drainable candidate: the ones behind it may be left unjudged
    assert (f.winner, f.first_ok) == (winner, first_ok)
    if 0 <= first_fb and (first_ok < 0 or first_fb < first_ok):
        assert f.first_fallback == first_fb
    else:
        assert f.first_fallback in (-1, first_fb)
    assert list(f_map) == list(p.winner_map)
    for c in range(len(cands)):
        if f_status[c] == capi.SR_CAND_SKIPPED:
            assert 0 <= first_ok < c, c
            continue
        assert f_status[c] == status[c], (c, f_status[c], status[c])
        if status[c] != S.FB:
            assert list(f_nodes[cand_off[c]:cand_off[c + 1]]) == list(nodes[cand_off[c]:cand_off[c + 1]]), c
    return t


@pytest.mark.parametrize("name,form", CALLS, ids=["%s-%s" % nf for nf in CALLS])
def test_calls(planners, name, form):
    run_call(planners(form), S.get_input(name))


@pytest.mark.parametrize("form", sorted(FORMS))
def test_ticks_on_one_planner(form, record_property):
    """Pads and probe (bit 63), the probe alone (bit 2, another swap_mask), pads and probe again -- three times,
    so that the planner keeps the candidate side -- and then, twice, after node 1 gained a base pod on the probe's
    port (a reused tick with one changed node); a planner of its own."""
    inp = S.get_input("ticks")
    ck = make_checker(**FORMS[form])
    path = []
    try:
        for drop, filler, nodes, _, _ in [S.TICKS[k] for k in S.TICK_SCRIPT]:
            fillers = ((inp.extra_pod[0], S.TICK_FILLER_NODE),) if filler else ()
            t = run_call(ck, inp, drop, fillers, want={"probe_tick": nodes})
            path.append((t.enc_reused, t.k0_columns))
    finally:
        ck.close()
        print("\nticks %s: (enc_reused, k0_columns) %s" % (form, path))
        record_property("path", str(path))
    if form != "one_plan_slot":
        # the tick with the new base pod keeps the candidate side; the base port is an S-row atom, so the tick is
        # not K0-less: the incremental K0 rewrites the one changed row word
        assert path[S.TICK_SCRIPT.index(2)] == (1, 1), path


@pytest.mark.parametrize("form", sorted(FORMS))
def test_sequence(planners, form):
    """After the first probe drains, its ports are base UsedPorts: the second probe on the same port (bit 63)
    avoids those nodes; against the reference pass and the hand-derived nodes."""
    nodes, base, cands, want, drained = S.sequence_case()
    inp = _sequence_input(nodes, base, cands)
    got = check_sequence(planners(form), inp)
    assert list(got.drained) == drained
    assert list(got.node_of_pod) == want


_seq = {}


def _sequence_input(nodes, base, cands):
    if "inp" not in _seq:
        _seq["inp"] = from_scenario(nodes, base, cands, stamped="state-word-sequence")
    return _seq["inp"]
