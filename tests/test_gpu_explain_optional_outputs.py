"""The optional outputs of the explain / shortfall calls do not move the others.

Where a part of the calls' two device buffers lies depends on four switches: context lists, shortfall, node_mask,
node_short (csrc/explain_stage.hpp).  On hand-built clusters sr_shortfall_pods and sr_shortfall_plan run with every
combination of `why` x node_mask x node_short, sr_explain_pods and sr_explain_plan with and without node_mask;
every array two runs share must be identical, and the full run must be what the host statements give
(lib/libsrexplainview.so through shortfall_ref.view_pods / view_plan; counts, feasible, first and the reductions
follow from its masks and shortfalls).

The shapes are the ones where alignment shows: 5 spot nodes, so a pod's 10 bytes of mask leave the masks off an
8-byte boundary and the blocks' partials behind them start after padding; three queries with a fallback pod in the
middle, so the active order is not the asked order and a cleared slot sits between filled ones; and 65 spot nodes
(two row words, one shortfall block) for the pods calls."""
import contextlib
import itertools

import numpy as np
import pytest

import explain_plan_cases as C
import shortfall_ref as R
from helpers import Scenario
from known_answer import N, P, used
from spotplanner import capi
from spotplanner.model import Container, Pod, Taint
from spotplanner.rescheduler import explain_arrays, explain_plan_arrays, shortfall_arrays, shortfall_plan_arrays

pytestmark = pytest.mark.gpu

KEY = Taint("k", "v", "NoSchedule")
SWITCHES = list(itertools.product((True, False), repeat=3))  # why, node_mask, node_short; the full run first


@contextlib.contextmanager
def snapshot(sc):
    h = sc.product_snapshot()
    try:
        yield h
    finally:
        capi.load_planner().sr_snapshot_destroy(h)


def _fb(name):
    return Pod(name, containers=[Container(cpu_milli=100)], has_pvc=True)  # outside the encoded predicate set


def _filler(name):
    return Pod(name, containers=[Container()])


def _pool(n):
    """n 1000m nodes by j % 5: 0 holds 950m, 1 is tainted, 2 has its one pod slot taken, 3 holds 450m, 4 is empty."""
    nodes, base = [], []
    for j in range(n):
        k = j % 5
        nodes.append(N("n%d" % j, cpu=1000, pods=1 if k == 2 else 110, taints=[KEY] if k == 1 else []))
        base.append([used(cpu=950, name="u%d" % j)] if k == 0 else [_filler("f%d" % j)] if k == 2 else
                    [used(cpu=450 + j, name="u%d" % j)] if k == 3 else [])
    return nodes, base


def _arrays(why, short):
    """{field: array} of what a run returned."""
    out = {}
    for res, fields in ((why, ("feasible", "first", "counts", "fallback", "node_mask", "how")),
                        (short, ("near", "only_nodes", "only_min", "only_at", "node_short"))):
        for f in fields:
            if res is not None and getattr(res, f) is not None:
                out[f] = np.array(getattr(res, f))
    return out


def _same_shared(runs):
    """Every array two runs share is identical (each run against the first, the full one)."""
    full = runs[0][1]
    for what, got in runs[1:]:
        for f in sorted(set(full) & set(got)):
            assert np.array_equal(full[f], got[f]), (what, f)
    return full


def _equals_view(full, view, judged, none):
    """The full run against the host statements: rows `judged` evaluated, rows `none` cleared."""
    why = type("Why", (), full)
    for i in judged:
        m, s = view["masks"][i], view["shorts"][i]
        assert np.array_equal(full["node_mask"][i], m) and np.array_equal(full["node_short"][i], s), i
        ok = np.flatnonzero(m == 0)
        assert full["feasible"][i] == len(ok) and full["first"][i] == (ok[0] if len(ok) else -1), i
        assert list(full["counts"][i]) == [int(np.sum(m >> r & 1)) for r in range(capi.SR_WHY_COUNT)], i
        assert full["fallback"][i] == 0
        R.check_reduced(why, i, R.reduce_row(m, s), i)
    for i in none:
        assert full["feasible"][i] == -1 and full["first"][i] == -1 and not full["counts"][i].any(), i
        assert not full["node_mask"][i].any(), i
        R.check_none(why, i, i)


@pytest.mark.parametrize("n_spot", [5, 65])
def test_pods_calls(checker, n_spot):
    nodes, base = _pool(n_spot)
    sc = Scenario(nodes, base, [P("p0", cpu=100), _fb("fb"), P("p2", cpu=600)])
    pods = np.array([sc.qidx(i) for i in range(3)], np.int32)
    runs = []
    with snapshot(sc) as h:
        for why, mask, short in SWITCHES:
            runs.append((("shortfall", why, mask, short),
                         _arrays(*shortfall_arrays(checker, h, sc.ptr, pods, node_short=short, node_mask=mask, why=why))))
        for mask in (True, False):
            runs.append((("explain", mask), _arrays(explain_arrays(checker, h, sc.ptr, pods, node_mask=mask), None)))
    full = _same_shared(runs)
    view = R.view_pods(sc, pods)
    assert list(view["fallback"]) == [0, 1, 0] and list(full["fallback"]) == [0, 1, 0]
    _equals_view(full, view, judged=(0, 2), none=(1,))
    assert full["near"][0] >= 1 and full["near"][2] >= 1  # the pool shows shortfalls to both pods


def test_plan_calls(checker):
    """Three candidates on the 5-node pool: one asked at its only pod (an empty context), the fallback pod asked at
    pod 0 of two (handed back by the batched encode, so it goes alone and stays cleared), one asked at its third pod
    with both earlier pods on node 4."""
    nodes, base = _pool(5)
    b = C.Built(C.PlanCase("optional_outputs", nodes, base, [
        C.Cand([P("a0", cpu=600)], 0, [-1], C.BATCHED),
        C.Cand([_fb("b0"), P("b1", cpu=10)], 0, [-1, -1], C.SINGLE),
        C.Cand([P("c0", cpu=300), P("c1", cpu=300), P("c2", cpu=500)], 2, [4, 4, -1], C.BATCHED)]))
    args = (b.sc.ptr, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
    runs = []
    with snapshot(b.sc) as h:
        for why, mask, short in SWITCHES:
            runs.append((("shortfall", why, mask, short),
                         _arrays(*shortfall_plan_arrays(checker, h, *args, node_short=short, node_mask=mask, why=why))))
        for mask in (True, False):
            runs.append((("explain", mask), _arrays(explain_plan_arrays(checker, h, *args, node_mask=mask), None)))
    full = _same_shared(runs)
    view = R.view_plan(b.sc, b.cand_off, b.cand_pods, b.at_pod, b.node_of_pod)
    assert list(full["how"]) == [C.BATCHED, C.SINGLE, C.BATCHED] == list(view["how"])
    assert list(full["fallback"]) == [0, 1, 0]
    _equals_view(full, view, judged=(0, 2), none=(1,))
    # node 4 after 600m of earlier pods: 100m short for the 500m pod, and nowhere else cpu alone by less
    assert full["node_short"][2][4][capi.SR_SHORT_CPU] == 100 and full["only_at"][2][capi.SR_SHORT_CPU] == 4
