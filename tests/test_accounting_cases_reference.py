"""tests/accounting_cases.py without a GPU: the plain statement of the loop against the oracle (the contract's loop
of tests/blockers_ref.py for the candidates, really reduced snapshots of tests/evacuate_ref.py for the scenarios)
and against the host views (blockers_candidate / evacuate_scenario through sr_blockers_plan_view and
sr_evacuate_plan_view), the way every group must go, and the fault models: under each wrong variant a group is
meant to catch, the statement's answer differs from the right one.  No case is skipped."""
import functools

import numpy as np
import pytest

import accounting_cases as A
from blockers_ref import oracle_blockers_plan
from evacuate_ref import oracle_evacuate_plan
from spotplanner import capi
from test_blockers_reference import blockers_view
from test_evacuate_reference import evacuate_view

CASES = A.cases()
IDS = [c.name for c in CASES]
FOUR = [bit.bit_length() - 1 for bit in (A.PODS,) + A.BITS]


@functools.lru_cache(maxsize=None)
def built(name):
    return A.Built(next(c for c in CASES if c.name == name))


def test_constants_are_the_product_s():
    assert A.CAP == capi.SR_BLOCKERS_BATCH_PODS
    assert (A.JUDGED, A.NOT_PLAIN) == (capi.SR_EVAC_JUDGED, capi.SR_EVAC_NOT_PLAIN)
    assert (A.BATCHED, A.SINGLE) == (capi.SR_EXPLAIN_BATCHED, capi.SR_EXPLAIN_SINGLE)
    assert [capi.WHY_NAMES[r] for r in FOUR] == ["PODS", "CPU", "MEMORY", "EPHEMERAL"]


def test_pools_and_groups_are_what_the_cases_promise():
    assert {len(c.nodes) for c in CASES} == {65, 130, 257}
    for c in CASES:
        n = len(c.nodes)
        assert n % 64 != 0
        # another unit and another magnitude per dimension, cpu below 4,000 millicores where it is not a 64-bit case
        if not c.name.startswith("sums_of_64_bits"):
            assert all(nd.cpu_milli < 4000 for nd in c.nodes)
        assert all(len({nd.cpu_milli, nd.memory, nd.ephemeral}) == 3 for nd in c.nodes)
    named = {c.name.rsplit("_", 1)[0] for c in CASES}
    assert {"dimensions_apart", "crossed", "acc_apart_from_req", "zero_and_partial", "sums_of_64_bits", "the_undo"} <= named


def rows_of(counts, p0, rows):
    """The statement's rows against a counts array: the four fitsRequest reasons, and no other reason anywhere."""
    for k, row in rows.items():
        assert list(counts[p0 + k]) == A.why_row(row), (k, list(counts[p0 + k]), row)


@pytest.mark.parametrize("name", IDS)
def test_the_right_answer_is_the_oracle_s(name):
    b = built(name)
    case = b.case
    if b.cands:
        ref = oracle_blockers_plan(b.sc, b.sc.oracle_snapshot(), b.cand_off, b.cand_pods, b.ask, b.n_spot)
        assert not ref["fallback"].any()
        for c, i in enumerate(b.cands):
            mapping = b.right[i][0]
            lo, hi = int(b.cand_off[c]), int(b.cand_off[c + 1])
            assert list(ref["node_of_pod"][lo:hi]) == mapping, (case.groups[i].name, list(ref["node_of_pod"][lo:hi]))
            assert ref["blockers"][c] == mapping.count(-1)
            assert ref["first"][c] == (mapping.index(-1) if -1 in mapping else -1)
    args = b.scen_args()
    ref = oracle_evacuate_plan(b.sc, *args)
    assert not ref["fallback"].any()
    for i, g in enumerate(case.groups):
        mapping = b.right[i][0]
        lo, hi = int(args[0][i]), int(args[0][i + 1])
        assert list(ref["node_of_pod"][lo:hi]) == mapping, (g.name, list(ref["node_of_pod"][lo:hi]))
        assert ref["stranded"][i] == mapping.count(-1)


@pytest.mark.parametrize("name", IDS)
def test_the_host_views_follow_the_statement(name):
    b = built(name)
    case = b.case
    if b.cands:
        v = blockers_view(b.sc, b.cand_off, b.cand_pods, b.ask)
        bare = blockers_view(b.sc, b.cand_off, b.cand_pods, b.ask, counts=False)
        assert list(v["how"]) == list(b.how_b) and not v["fallback"].any()
        for key in ("how", "node_of_pod", "blockers", "first", "fallback"):
            assert np.array_equal(v[key], bare[key]), key
        for c, i in enumerate(b.cands):
            mapping, rows = b.right[i]
            lo, hi = int(b.cand_off[c]), int(b.cand_off[c + 1])
            assert list(v["node_of_pod"][lo:hi]) == mapping, case.groups[i].name
            assert v["blockers"][c] == mapping.count(-1)
            rows_of(v["counts"], lo, rows)
            assert not v["counts"][lo:hi][[k for k in range(hi - lo) if mapping[k] >= 0]].any()
        for p, row in b.pinned_cands().items():
            assert list(v["counts"][p]) == row
    args = b.scen_args()
    v = evacuate_view(b.sc, *args)
    bare = evacuate_view(b.sc, *args, counts=False)
    for key in ("how", "node_of_pod", "stranded", "first"):
        assert np.array_equal(v[key], bare[key]), key
    assert list(v["how"]) == [g.how_e for g in case.groups]
    for i, g in enumerate(case.groups):
        mapping, rows = b.right[i]
        lo, hi = int(args[0][i]), int(args[0][i + 1])
        if g.how_e != A.JUDGED:  # nothing is reported
            assert v["stranded"][i] == -1 and (v["node_of_pod"][lo:hi] == -1).all() and not v["counts"][lo:hi].any()
            continue
        assert list(v["node_of_pod"][lo:hi]) == mapping, g.name
        assert v["stranded"][i] == mapping.count(-1)
        assert v["first"][i] == (mapping.index(-1) if -1 in mapping else -1)
        rows_of(v["counts"], lo, rows)
    for p, row in b.pinned().items():
        assert list(v["counts"][p]) == row


@pytest.mark.parametrize("name", IDS)
def test_every_named_wrong_variant_changes_the_answer(name):
    b = built(name)
    for i, g in enumerate(b.case.groups):
        for wrong in g.catches:
            assert b.wrong(i, wrong) != b.right[i], (g.name, wrong)
    for order in b.case.orders:
        right = b.sequence(order)
        assert right == [b.right[i] for i in order]  # a right loop does not care what the block took before
        for wrong in b.case.seq_catches:
            if wrong == "undo_first" and order[0] != 0:
                continue  # only X has more pods than the first stride visits
            got = b.sequence(order, wrong)
            assert got[0] == right[0]
            assert all(got[s] != right[s] for s in range(1, len(order))), (order, wrong)


def test_every_variant_is_caught_by_the_groups_meant_to():
    caught = {}
    for c in CASES:
        for g in c.groups:
            for wrong in g.catches:
                caught.setdefault(wrong, set()).add(c.name.rsplit("_", 1)[0] if c.name[-1].isdigit() else c.name)
        for wrong in c.seq_catches:
            caught.setdefault(wrong, set()).add("the_undo")
    assert set(caught) == set(A.WRONG)
    assert caught["own_use_dim0_only"] >= {"dimensions_apart", "crossed", "acc_apart_from_req", "zero_and_partial",
                                           "the_list_in_memory", "the_list_in_ephemeral"}
    assert caught["account_req"] == {"acc_apart_from_req"} and caught["trunc32"] == {"sums_of_64_bits"}
    assert caught["shift_dim0_only"] == {"the_list_in_memory", "the_list_in_ephemeral"}
    assert caught["dims_swapped"] >= {"dimensions_apart", "crossed"}
    for wrong in ("stale_deltas", "undo_first", "undo_dim0_only"):
        assert caught[wrong] == {"the_undo"}
    # in every pool size, both in memory and in ephemeral storage
    for n in (65, 130, 257):
        for name in ("dimensions_apart_%d" % n, "acc_apart_from_req_%d" % n):
            groups = built(name).case.groups
            assert any("memory" in g.name and g.catches for g in groups) and any("ephemeral" in g.name and g.catches for g in groups)


@pytest.mark.parametrize("name", ["the_list_in_memory", "the_list_in_ephemeral"])
def test_the_list_is_shifted_across_its_slots(name):
    """What the docstring of the list case claims, on the right answer: inserts in front of and between held
    entries while the list holds more than 64 and more than 128, a tail that returns to shifted entries, 256
    entries' worth of pods at the capacity and one pod more the SINGLE way."""
    b = built(name)
    at_cap, past, twenty = b.case.groups
    assert len(at_cap.pods) == A.CAP and len(past.pods) == A.CAP + 1
    assert (at_cap.how_b, past.how_b, twenty.how_b) == (A.BATCHED, A.SINGLE, A.BATCHED)
    mapping = b.right[0][0]
    assert b.right[1][0][:A.CAP] == mapping
    held, between, crossing = [], {64: 0, 128: 0}, {64: 0, 128: 0, 192: 0}
    shifted = set()
    returns = on_shifted = 0
    for k, j in enumerate(mapping):
        assert j >= 0
        if j in held:
            returns += 1
            on_shifted += j in shifted
            continue
        pos = sum(1 for x in held if x < j)
        if pos < len(held):
            for limit in between:
                between[limit] += len(held) > limit
            for edge in crossing:
                # the tail [pos, len) moves up by one: the entry at edge - 1, lane 63 of a slot, goes to lane 0 of the next
                crossing[edge] += pos <= edge - 1 < len(held)
            shifted.update(x for x in held if x > j)
        held.append(j)
        held.sort()
    assert len(held) == 220 and between[64] >= 100 and between[128] >= 40
    assert crossing[64] >= 30 and crossing[128] >= 5 and crossing[192] >= 10
    assert returns == A.CAP - 220 and on_shifted >= 24  # every tail pod lands on a held entry, most on shifted ones
    assert b.right[2][0] == [0] * 20 + [1]


@pytest.mark.parametrize("name", ["the_undo_130", "the_undo_257"])
def test_the_undo_case_is_what_it_says(name):
    b = built(name)
    n = b.n_spot
    x, y, z = b.case.groups
    assert len(x.pods) == 300 > A.BLOCK_THREADS
    mx = b.right[0][0]
    S, M, E = 0, 64, n - 1
    assert not {S, M, E} & set(mx[:A.BLOCK_THREADS])            # the first stride's pods never touch them
    assert mx[256:260] == [S, S, M, E]                           # ... the second stride's fill them
    assert mx.count(-1) >= 5 and -1 in mx[:A.BLOCK_THREADS] and mx[299] == -1
    assert {j >> 6 for j in mx if j >= 0} == set(range((n + 63) // 64))
    for d in (1, 2):  # memory and ephemeral storage are used in every row word that has a node beside S, M and E
        words = {j >> 6 for k, j in enumerate(mx) if j >= 0 and b.mpods[0][k].acc[d] > 0}
        assert words >= {j >> 6 for j in range(n) if j not in (S, M, E)}, (d, words)
    assert b.right[1][0] == [S, M, E]
    assert M in z.lost and M in mx and b.right[2][0].count(-1) == 1
    # each pod of Y is decided by one thing: on what X leaves behind, y_s meets the pod count alone on S, y_m
    # memory alone on M, y_e ephemeral storage alone on E
    stale = b.sequence((0, 1), "stale_deltas")[1]
    assert stale[0] == [-1, -1, -1]


@pytest.mark.parametrize("name", ["sums_of_64_bits_65", "sums_of_64_bits_130"])
def test_the_quantity_limit_is_met_exactly(name):
    b = built(name)
    top = max(nd.memory - f[1] for nd, f in zip(b.case.nodes, b.free))
    groups = {g.name: i for i, g in enumerate(b.case.groups)}
    at = sum(p.acc[1] for p in b.mpods[groups["at_the_quantity_limit"]])
    past = sum(p.acc[1] for p in b.mpods[groups["past_the_quantity_limit"]])
    assert top + at == A.QUANTITY_END - 1 and top + past == A.QUANTITY_END
    assert len(set(b.right[groups["past_the_quantity_limit"]][0])) == 2  # different nodes: every Requested stays in range
    for i, g in enumerate(b.case.groups):
        sums = {}
        for p, j in zip(b.mpods[i], b.right[i][0]):
            if j >= 0:
                sums[j] = sums.get(j, 0) + p.acc[1]
        if g.name == "past_2_53":
            assert (1 << 53) + 1 in _prefix_sums(b, i)
        if g.name.startswith("past_2_"):
            assert max(sums.values()) > 1 << int(g.name.rsplit("_", 1)[1])


def _prefix_sums(b, i):
    out, s = [], 0
    for p in b.mpods[i]:
        s += p.acc[1]
        out.append(s)
    return out
