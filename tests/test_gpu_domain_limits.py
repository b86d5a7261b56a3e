"""K2's domain path at its limits on the GPU: the calls of domain_limits.py
through the C ABI, every candidate bit-exact against the oracle (status,
node_of_pod, winner, first_ok, first_fallback, the winner-only run) and against
its hand-derived plan.  A candidate at a limit (64 values of a shared key, four
key slots, four terms of an affinity set, two interacting spread constraints)
is planned on the device; one step over it the candidate -- and only it -- is
SR_CAND_FALLBACK.  The wide pools put the deciding nodes into the second and
third 4,096-node chunk.  test_domain_limits_reference.py asserts on the CPU
that each case is decisive: a k2_domain that shifts a domain bit in 32 bits,
takes the spread minimum over half the wave, rechecks touched nodes in the
first chunk only, tests a node-local bit against the lane or ignores key slot
3 fails here."""
import dataclasses

import numpy as np
import pytest

import domain_limits as D
from spotplanner import capi
from spotplanner.rescheduler import plan_arrays
from test_domain_limits_reference import check_hand_answers, oracle_with_filler
from test_gpu_parity import compare_plans
from test_gpu_sequence import check_sequence, make_checker
from test_gpu_sequence_pdb import check_limited

pytestmark = pytest.mark.gpu

FB = capi.SR_CAND_FALLBACK
FORMS = {
    "default": {},
    "pod_order": dict(SR_K2_MODE=1),
    "split": dict(SR_K2_SPLIT_MIN=0),  # node-order and domain-path candidates in two kernels side by side
    "k0_every_call": dict(SR_K0_SKIP=0),
    "one_plan_slot": dict(SR_PLAN_SLOTS=1),
}
# calls that hold node-order and domain-path candidates: the forced split launch runs two kernels
SPLIT_CALLS = {("z64", "main"), ("wide3", "main"), ("wide2", "with")}


@pytest.fixture(scope="module")
def planners():
    """One planner per form for the whole module: the calls follow one another on it, pools of 192 to 8,300
    nodes in turn."""
    made = {}

    def get(form):
        if form not in made:
            made[form] = make_checker(**FORMS[form])
        return made[form]

    yield get
    for ck in made.values():
        ck.close()


def run_call(ck, P, call, filler=False):
    """One call in full and winner-only against the oracle and the hand answers; returns the full run's timing."""
    cands = P.calls[call].cands
    cand_off, cand_pods = P.arrays(call)
    o = oracle_with_filler(P, call) if filler else P.oracle(call)
    lib = capi.load_planner()
    h = P.sc.product_snapshot()
    try:
        if filler:
            pod = P.pod_index(P.calls["filler"].cands[0].pods[0])
            assert lib.sr_snapshot_add_pod(h, P.sc.ptr, pod, D.CHANGED_NODE) == capi.SR_OK
        q = plan_arrays(ck, h, P.sc.ptr, cand_off, cand_pods, full=False)  # winner only
        p = plan_arrays(ck, h, P.sc.ptr, cand_off, cand_pods)
        t = ck.timing()
    finally:
        lib.sr_snapshot_destroy(h)
    # at a limit no fallback, one over it the candidate alone
    assert [int(s) == FB for s in p.status] == [cd.fallback for cd in cands], (call, list(p.status))
    compare_plans(o, p, cand_off, extra_fallback=lambda c: cands[c].fallback)
    planned = [dataclasses.replace(cd, want=None) if cd.fallback else cd for cd in cands]
    check_hand_answers(dict(status=p.status, node_of_pod=p.node_of_pod), planned, cand_off,
                       changed=D.CHANGED if filler else None)
    assert (q.first_ok, q.first_fallback, q.winner) == (p.first_ok, p.first_fallback, p.winner)
    assert np.array_equal(q.winner_map, p.winner_map)
    if p.first_ok >= 0:
        assert np.array_equal(p.winner_map, o["node_of_pod"][cand_off[p.first_ok]:cand_off[p.first_ok + 1]])
    return t


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("pool,call", D.CALLS, ids=["%s-%s" % pc for pc in D.CALLS])
def test_calls(planners, pool, call, form):
    t = run_call(planners(form), D.get_pool(pool), call)
    if form == "split" and (pool, call) in SPLIT_CALLS:
        assert t.k2_launches == 2, t.k2_launches


def test_key_slots_are_per_call(checker):
    """Four keys, four other keys, the first four again, then a call one key over the limit and one within it:
    a call's slots are its own."""
    P = D.get_pool("z64")
    for call in ("keys_four_a", "keys_four_b", "keys_four_a", "keys_forward", "keys_four_b", "keys_reverse",
                 "keys_four_a"):
        run_call(checker, P, call)


WIDE2_FORMS = {"default": {}, "split": dict(SR_K2_SPLIT_MIN=0), "s_full": dict(SR_S_HEAD_ONLY=0),
               "one_plan_slot": dict(SR_PLAN_SLOTS=1)}


@pytest.mark.parametrize("form", sorted(WIDE2_FORMS))
def test_wide2_consecutive_calls(form, record_property):
    """One planner of its own on the 68-word pool: a list without a domain-path candidate (head-only S rows by
    default), the same list with one (full S rows for the whole launch), without it again -- three times, so that
    the last of them, after the filler pod changed s4298, is a reused tick -- and with it on the changed node."""
    P = D.get_pool("wide2")
    ck = make_checker(**WIDE2_FORMS[form])
    script = [("without", False), ("with", False), ("without", False), ("without", False), ("without", True),
              ("with", True)]
    path = []
    try:
        for call, filler in script:
            t = run_call(ck, P, call, filler)
            path.append((call, filler, t.k2_launches, t.enc_reused))
    finally:
        ck.close()
        print("wide2 %s: (call, changed, k2_launches, enc_reused) %s" % (form, path))
        record_property("path", str(path))
    launches = [x[2] for x in path]
    assert launches[0] == launches[2] == launches[3] == launches[4] == 1, path
    assert launches[1] == launches[5] == (2 if form == "split" else 1), path
    if form != "one_plan_slot":
        assert path[4][3] == 1, path  # saved by the third call, indexed by the fourth, reused by the fifth


@pytest.mark.parametrize("name", sorted(D.sequence_cases()))
def test_sequences(checker, name):
    """sr_plan_sequence and sr_plan_sequence_pdb (one group that allows every eviction: `remaining`) against the
    reference pass: drains, stop, statuses, mappings and node states, and the hand-derived mappings."""
    case, inp = D.get_sequence(name)
    got = check_sequence(checker, inp)
    assert list(got.drained) == case.drained
    check_hand_answers(dict(status=got.status, node_of_pod=got.node_of_pod), case.cands, inp.cand_off)
    n_pods = int(inp.cand_off[-1])
    allowed, pod_group = np.array([n_pods], np.int32), np.zeros(n_pods, np.int32)
    lim, ref = check_limited(checker, inp, "domain-limits", allowed, pod_group)
    assert list(lim.drained) == case.drained
    assert list(lim.remaining) == [n_pods - sum(len(case.cands[c].pods) for c in case.drained)]
    assert np.array_equal(lim.node_of_pod, got.node_of_pod)
