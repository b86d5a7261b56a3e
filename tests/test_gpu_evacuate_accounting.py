"""sr_evacuate_plan on the accounting cases of tests/accounting_cases.py: memory and ephemeral storage in the
scenario's own deltas, accounting apart from the fit request, zero and partial requests on overcommitted nodes,
64-bit sums and the quantity limit of the rule, and the undo: a block that takes a 300-pod scenario, then one
whose pods fit only where the first left nothing, in one launch and from call to call on one context.  Every
comparison is bit-exact: the oracle on really reduced snapshots (tests/evacuate_ref.py), the hand values where the
case writes them out, sr_explain_candidate on the reduced product snapshot for the rows; and every launch shape
-- the default, one block for all scenarios, 1, 2 and 16 waves a block, each also with one block -- gives the
same arrays."""
import numpy as np
import pytest

import accounting_cases as A
from evacuate_ref import compacted, oracle_evacuate_plan, reduced_product
from spotplanner import capi
from spotplanner.rescheduler import evacuate_plan_arrays, explain_candidate_arrays
from test_accounting_cases_reference import built
from test_gpu_evacuate import check_rows, same_but_counts
from test_gpu_k2_dispatch import make_checker
from test_gpu_shortfall import snapshot

pytestmark = pytest.mark.gpu

CASES = A.cases()
UNDO = [c for c in CASES if c.orders]
# (SR_EVAC_GRID, SR_EVAC_WAVES); None: the default
FORMS = [(None, None), ("1", None), (None, "1"), ("1", "1"), (None, "2"), ("1", "2"), (None, "16"), ("1", "16")]


def set_form(monkeypatch, form):
    for key, value in zip(("SR_EVAC_GRID", "SR_EVAC_WAVES"), form):
        if value is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, value)


def same(a, b):
    same_but_counts(a, b)
    assert np.array_equal(a.counts, b.counts)


def check_one_row(checker, sc, scen_off, scen_pods, lost, res, s, k):
    """check_rows for one stranded pod: its counts row is sr_explain_candidate's for the compacted list on a
    product snapshot built without the lost nodes."""
    lo, hi = int(scen_off[s]), int(scen_off[s + 1])
    row = res.node_of_pod[lo:hi]
    assert row[k] < 0
    h, keep = reduced_product(sc, lost)
    back = {j: i for i, j in enumerate(keep)}
    try:
        pods, mapping, at = compacted(scen_pods[lo:hi], row, k)
        mapping = [back[j] if j >= 0 else -1 for j in mapping]
        one = explain_candidate_arrays(checker, h, sc.ptr, np.array(pods, np.int32), np.array(mapping, np.int32), at,
                                       node_mask=False)
        assert one.fallback[0] == 0 and one.feasible[0] == 0 and one.first[0] == -1, (s, k)
        assert np.array_equal(res.counts[lo + k], one.counts[0]), (s, k)
    finally:
        capi.load_planner().sr_snapshot_destroy(h)


def against_the_statement(b, order, res):
    """The call's arrays for the groups `order` against the right answer of every group on its own (the oracle's:
    tests/test_accounting_cases_reference.py) and the hand values."""
    groups = b.case.groups
    assert list(res.how) == [groups[i].how_e for i in order]
    for s, i in enumerate(order):
        g = groups[i]
        lo, hi = int(res.scen_off[s]), int(res.scen_off[s + 1])
        if g.how_e != A.JUDGED:  # nothing is reported
            assert res.stranded[s] == -1 and res.first[s] == -1
            assert (res.node_of_pod[lo:hi] == -1).all() and not res.counts[lo:hi].any()
            continue
        mapping, rows = b.right[i]
        assert list(res.node_of_pod[lo:hi]) == mapping, (order, s, g.name)
        if g.want is not None:
            assert list(res.node_of_pod[lo:hi]) == g.want
        assert res.stranded[s] == mapping.count(-1)
        assert res.first[s] == (mapping.index(-1) if -1 in mapping else -1)
        for k in range(hi - lo):
            if k in rows:
                assert list(res.counts[lo + k]) == A.why_row(rows[k]), (order, s, k)
            else:
                assert not res.counts[lo + k].any()
        for k, row in g.rows.items():
            assert list(res.counts[lo + k]) == A.why_row(row)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_accounting_cases(checker, monkeypatch, case):
    b = built(case.name)
    sc = b.sc
    args = b.scen_args()
    order = list(range(len(case.groups)))
    ref = oracle_evacuate_plan(sc, *args)
    with snapshot(sc) as h:
        set_form(monkeypatch, FORMS[0])
        res = evacuate_plan_arrays(checker, h, sc.ptr, *args)
        bare = evacuate_plan_arrays(checker, h, sc.ptr, *args, counts=False)
        assert bare.counts is None
        same_but_counts(res, bare)
        for form in FORMS[1:]:
            set_form(monkeypatch, form)
            same(evacuate_plan_arrays(checker, h, sc.ptr, *args), res)
            same_but_counts(evacuate_plan_arrays(checker, h, sc.ptr, *args, counts=False), res)
    against_the_statement(b, order, res)
    scen_off, scen_pods = args[0], args[1]
    for s, g in enumerate(case.groups):
        if g.how_e != A.JUDGED:
            continue
        lo, hi = int(scen_off[s]), int(scen_off[s + 1])
        assert res.stranded[s] == ref["stranded"][s] and res.first[s] == ref["first"][s]
        assert np.array_equal(res.node_of_pod[lo:hi], ref["node_of_pod"][lo:hi]), g.name
        if case.all_rows:
            check_rows(checker, sc, scen_off, scen_pods, g.lost, res, s)
        else:
            for k in g.rows:
                check_one_row(checker, sc, scen_off, scen_pods, g.lost, res, s, k)


@pytest.mark.parametrize("case", UNDO, ids=[c.name for c in UNDO])
def test_the_undo_in_any_order_and_shape(checker, monkeypatch, case):
    """X Y Z, Z Y X and X Y X Y: with one block every scenario behind the first meets the slice the one before it
    left, under every number of waves (the undo's stride is the block's threads)."""
    b = built(case.name)
    sc = b.sc
    with snapshot(sc) as h:
        for order in case.orders:
            args = b.scen_args(order)
            for form in FORMS:
                set_form(monkeypatch, form)
                against_the_statement(b, order, evacuate_plan_arrays(checker, h, sc.ptr, *args))


@pytest.mark.parametrize("case", UNDO, ids=[c.name for c in UNDO])
def test_the_undo_across_calls_on_one_context(monkeypatch, case):
    """One context takes X alone, Y alone, Y again and then the whole list: the scratch is trusted to be zero from
    call to call, so each result must be what a context that never saw another call gives."""
    set_form(monkeypatch, FORMS[0])
    b = built(case.name)
    sc = b.sc
    calls = [(0,), (1,), (1,), (0, 1, 2)]
    fresh = {}
    with snapshot(sc) as h:
        for order in sorted(set(calls)):
            ck = make_checker()
            try:
                fresh[order] = evacuate_plan_arrays(ck, h, sc.ptr, *b.scen_args(order))
            finally:
                ck.close()
            against_the_statement(b, order, fresh[order])
        ck = make_checker()
        try:
            for order in calls:
                same(evacuate_plan_arrays(ck, h, sc.ptr, *b.scen_args(order)), fresh[order])
        finally:
            ck.close()
