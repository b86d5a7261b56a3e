"""sr_blockers_plan on the accounting cases of tests/accounting_cases.py: memory and ephemeral storage in the
candidate's own context, accounting apart from the fit request, zero and partial requests on overcommitted nodes,
the sorted list shifted across its slots with memory and ephemeral values in it, in-place updates, 64-bit sums
and the quantity limit of the plain rule.  Every comparison is bit-exact: the oracle loop
(tests/blockers_ref.py), the hand values where the case writes them out, sr_explain_candidate on the compacted
list for the rows, and sr_evacuate_plan on the same candidates as nothing-lost scenarios."""
import numpy as np
import pytest

import accounting_cases as A
from blockers_ref import compacted, oracle_blockers_plan
from spotplanner.rescheduler import blockers_plan_arrays, evacuate_plan_arrays, explain_candidate_arrays
from test_accounting_cases_reference import built
from test_gpu_blockers import check_rows, same_but_counts
from test_gpu_shortfall import snapshot

pytestmark = pytest.mark.gpu

CASES = [c for c in A.cases() if any(not g.lost for g in c.groups)]


def check_one_row(checker, h, sc, cand_off, cand_pods, res, c, k):
    """check_rows for one blocker: its counts row is sr_explain_candidate's for the compacted list."""
    lo, hi = int(cand_off[c]), int(cand_off[c + 1])
    row = res.node_of_pod[lo:hi]
    assert row[k] < 0
    pods, mapping, at = compacted(cand_pods[lo:hi], row, k)
    one = explain_candidate_arrays(checker, h, sc.ptr, np.array(pods, np.int32), np.array(mapping, np.int32), at,
                                   node_mask=False)
    assert one.fallback[0] == 0 and one.feasible[0] == 0 and one.first[0] == -1, (c, k)
    assert np.array_equal(res.counts[lo + k], one.counts[0]), (c, k)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_accounting_cases(checker, case):
    b = built(case.name)
    sc = b.sc
    ref = oracle_blockers_plan(sc, sc.oracle_snapshot(), b.cand_off, b.cand_pods, b.ask, b.n_spot)
    with snapshot(sc) as h:
        res = blockers_plan_arrays(checker, h, sc.ptr, b.cand_off, b.cand_pods, b.ask)
        bare = blockers_plan_arrays(checker, h, sc.ptr, b.cand_off, b.cand_pods, b.ask, counts=False)
        assert bare.counts is None
        same_but_counts(res, bare)
        assert list(res.how) == list(b.how_b)
        for f in ("blockers", "first", "node_of_pod", "fallback"):
            assert np.array_equal(getattr(res, f), ref[f]), f
        for c, i in enumerate(b.cands):
            g = case.groups[i]
            lo, hi = int(b.cand_off[c]), int(b.cand_off[c + 1])
            if g.want is not None:
                assert list(res.node_of_pod[lo:hi]) == g.want, g.name
            assert list(res.node_of_pod[lo:hi]) == b.right[i][0], g.name
            for k, row in g.rows.items():
                assert list(res.counts[lo + k]) == A.why_row(row), (g.name, k)
                if not case.all_rows:
                    check_one_row(checker, h, sc, b.cand_off, b.cand_pods, res, c, k)
            if case.all_rows:
                check_rows(checker, h, sc, b.cand_off, b.cand_pods, res, c)
            else:  # a placed pod has a zero row
                assert not res.counts[lo:hi][res.node_of_pod[lo:hi] >= 0].any()
        # every candidate as a scenario with nothing lost: the two calls agree in every output
        ev = evacuate_plan_arrays(checker, h, sc.ptr, *b.scen_args(b.cands, nothing_lost=True))
    assert list(ev.how) == [case.groups[i].how_e for i in b.cands]
    for c, i in enumerate(b.cands):
        lo, hi = int(b.cand_off[c]), int(b.cand_off[c + 1])
        if ev.how[c] != A.JUDGED:  # the rule refused it: nothing is reported, the SINGLE way answered above
            assert res.how[c] == A.SINGLE and ev.stranded[c] == -1 and (ev.node_of_pod[lo:hi] == -1).all()
            continue
        assert ev.stranded[c] == res.blockers[c] and ev.first[c] == res.first[c]
        assert np.array_equal(ev.node_of_pod[lo:hi], res.node_of_pod[lo:hi])
        assert np.array_equal(ev.counts[lo:hi], res.counts[lo:hi])
