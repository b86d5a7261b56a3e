"""Every kind of query call in turn on one context: they share one staged pass and one pair of buffers
(csrc/query.cpp), so what one call leaves there must not show in the next."""
import dataclasses

import numpy as np
import pytest

import evacuate_cases as E
import explain_plan_cases as C
from spotplanner import capi
from spotplanner.model import Container, ContainerPort, Pod
from spotplanner.rescheduler import (blockers_plan_arrays, evacuate_plan_arrays, explain_arrays, explain_plan_arrays,
                                     node_view_arrays, node_view_plan_arrays, plan_arrays,
                                     shortfall_plan_arrays)
from test_gpu_explain import _steady_scenario
from test_gpu_k2_dispatch import make_checker

pytestmark = pytest.mark.gpu


def _same(a, b, what):
    """Two results of one call, field by field (a tuple of results part by part)."""
    if isinstance(a, tuple):
        assert len(a) == len(b), what
        for k, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (what, k))
        return
    for f in dataclasses.fields(a):
        if f.name == "checks":  # (PlanResult: work done, not an answer)
            continue
        x, y = getattr(a, f.name), getattr(b, f.name)
        if x is None or y is None:
            assert x is None and y is None, (what, f.name)
        else:
            assert np.array_equal(x, y), (what, f.name, x, y)


class _Input:
    """A steady scenario `scale` times the usual size with two pods of one host port behind it, and the calls
    over it.  The blockers call asks the plan's stuck candidates and one more, the two host-port pods, which goes
    SINGLE; the evacuate call has one scenario per spot node: the node lost, the pods of a candidate moved."""

    def __init__(self, scale):
        hp = [Pod("hp%d" % k, containers=[Container(cpu_milli=10, ports=[ContainerPort(80)])]) for k in range(2)]
        self.sc, self.cand_off, self.cand_pods, _ = _steady_scenario(scale, hp)
        self.n_spot, n_cand = 8 * scale, len(self.cand_off) - 1
        self.b_off = np.append(self.cand_off, self.cand_off[-1] + 2).astype(np.int32)
        self.b_pods = np.append(self.cand_pods, [self.sc.qidx(len(self.cand_pods) + 1 + k) for k in range(2)]).astype(np.int32)
        lists = [self.cand_pods[self.cand_off[s % n_cand]:self.cand_off[s % n_cand + 1]] for s in range(self.n_spot)]
        self.scen_off = np.zeros(self.n_spot + 1, np.int32)
        self.scen_off[1:] = np.cumsum([len(x) for x in lists])
        self.scen_pods = np.concatenate(lists).astype(np.int32)
        self.lost_off = np.arange(self.n_spot + 1, dtype=np.int32)
        self.lost_pos = np.arange(self.n_spot, dtype=np.int32)

    def calls(self, full):
        """The calls after the plan, in the order of a round, as (name, f(checker, snapshot, plan)); `full`: the
        optional outputs (counts, node_mask, node_short) are wanted."""
        sc, off, pods = self.sc.ptr, self.cand_off, self.cand_pods

        def evacuate(ck, h, plan):
            return evacuate_plan_arrays(ck, h, sc, self.scen_off, self.scen_pods, self.lost_off, self.lost_pos, counts=full)

        return [
            ("explain_pods", lambda ck, h, plan: explain_arrays(ck, h, sc, pods, node_mask=full)),
            ("evacuate_plan", evacuate),
            ("node_view_plan", lambda ck, h, plan: node_view_plan_arrays(ck, h, sc, off, pods, plan.status, plan.node_of_pod)),
            ("blockers_plan", lambda ck, h, plan: blockers_plan_arrays(ck, h, sc, self.b_off, self.b_pods,
                                                                       np.append(plan.status, 0), counts=full)),
            ("shortfall_plan", lambda ck, h, plan: shortfall_plan_arrays(ck, h, sc, off, pods, plan.status, plan.node_of_pod,
                                                                         node_short=full, node_mask=full)),
            ("explain_plan", lambda ck, h, plan: explain_plan_arrays(ck, h, sc, off, pods, plan.status, plan.node_of_pod,
                                                                     node_mask=full)),
            ("node_view_pods", lambda ck, h, plan: node_view_arrays(ck, h, sc, pods)),
            ("evacuate_plan again", evacuate),
        ]

    def alone(self):
        """Every call made alone, each on a fresh context and a fresh snapshot: the plan, then {full: {name: result}}."""
        lib = capi.load_planner()

        def fresh(f):
            ck, h = make_checker(), self.sc.product_snapshot()
            try:
                return f(ck, h)
            finally:
                lib.sr_snapshot_destroy(h)
                ck.close()

        plan = fresh(lambda ck, h: plan_arrays(ck, h, self.sc.ptr, self.cand_off, self.cand_pods))
        want = {full: {name: fresh(lambda ck, h: f(ck, h, plan)) for name, f in self.calls(full)[:-1]}
                for full in (True, False)}
        for full in want:
            want[full]["evacuate_plan again"] = want[full]["evacuate_plan"]
        return plan, want


def test_every_query_kind_on_one_context():
    """Plan, sr_explain_pods, sr_evacuate_plan, sr_node_view_plan, sr_blockers_plan, sr_shortfall_plan,
    sr_explain_plan, sr_node_view_pods and sr_evacuate_plan again, three rounds over a small and a twice as large
    input (the buffers grow, then are larger than needed), the optional outputs wanted on even rounds only:
    every result is the one the same call gives alone on a fresh context."""
    inputs = [_Input(1), _Input(2)]
    alone = [x.alone() for x in inputs]
    for x, (plan, want) in zip(inputs, alone):  # the shared pass was gone through in every way
        b, e = want[True]["blockers_plan"], want[True]["evacuate_plan"]
        assert (b.how == C.BATCHED).any() and (b.how == C.SINGLE).any(), list(b.how)
        assert (e.how == E.JUDGED).any(), list(e.how)
        assert (want[True]["explain_plan"].how == C.BATCHED).any()
    lib = capi.load_planner()
    ck = make_checker()
    snaps = [x.sc.product_snapshot() for x in inputs]
    try:
        for rnd in range(3):
            full = rnd % 2 == 0
            for x, h, (plan_alone, want) in zip(inputs, snaps, alone):
                plan = plan_arrays(ck, h, x.sc.ptr, x.cand_off, x.cand_pods)
                _same(plan, plan_alone, "round %d plan" % rnd)
                for name, f in x.calls(full):
                    _same(f(ck, h, plan), want[full][name], "round %d scale %d %s" % (rnd, x.n_spot // 8, name))
    finally:
        for h in snaps:
            lib.sr_snapshot_destroy(h)
        ck.close()
