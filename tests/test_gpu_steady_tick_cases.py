"""Steady ticks whose changed spot node decides the plan, on the GPU: the
scripts of steady_tick_cases.py through one planner per form, every tick
bit-exact against the oracle on the same state and against the hand-derived
nodes, with the path each tick takes (no K0 while at most 16 nodes changed
since the tables were written, K0 on the 17th, no K0 again after it).
test_steady_tick_cases_reference.py asserts on the CPU that each listed pod
has another node on the state the tables were written from: a K2 that leaves a
changed node's bit, S row, running state or pod group uncorrected fails here."""
import numpy as np
import pytest

import steady_tick_cases as S
from spotplanner import capi
from spotplanner.rescheduler import plan_arrays
from test_gpu_k2_dispatch import make_checker
from test_steady_tick_cases_reference import oracle_tick, pod_slot

pytestmark = pytest.mark.gpu

FORMS = {
    "default": {},
    "k0_skip_off": dict(SR_K0_SKIP=0),                       # the same ticks through the incremental K0's columns
    "k0_full": dict(SR_K0_SKIP=0, SR_K0_INCREMENTAL=0),      # ... through a K0 that rewrites every row
    "node_patch_off": dict(SR_NODE_PATCH=0),                 # the changed node section goes up whole
    "narrow_off": dict(SR_K2_NARROW=0),                      # 64-bit window state only
    "general_kernel": dict(SR_K2_NODE_KERNEL=0),
    "s_full": dict(SR_S_HEAD_ONLY=0),                        # wide: full S rows on rows wider than 64 words
    "wpb4": dict(SR_K2_WPB=4),
    # the far probes through coop_scan (without ext_any / ext_far: a launch with extension records has no
    # cooperative blocks)
    "coop": dict(SR_LIST_COST_MIN=0, SR_K2_WPB=4, SR_K2_COOP=4096),
    "one_slot": dict(SR_PLAN_SLOTS=1),
}
HEAD_FORMS = ("default", "k0_skip_off", "k0_full", "node_patch_off", "narrow_off")
CASES = [(pool, form, big) for pool in sorted(S.POOLS) for form in FORMS for big in (True, False)
         if (pool != "head" or form in HEAD_FORMS) and (form != "s_full" or pool == "wide")]


def product_snapshot(P, tick):
    lib = capi.load_planner()
    h = P.sc.product_snapshot()
    for pod, pos in P.fillers_of(tick):
        assert lib.sr_snapshot_add_pod(h, P.sc.ptr, pod, pos) == capi.SR_OK
    return h


@pytest.mark.parametrize("pool,form,big", CASES,
                         ids=["%s-%s-%s" % (p, f, "big" if b else "small") for p, f, b in CASES])
def test_steady_ticks(pool, form, big, record_property):
    """`small`: without the 100- and the 200-pod candidate, so that the launch is the one-group kernel
    instance."""
    P = S.get_pool(pool)
    ext = form != "coop"
    names, cand_off, cand_pods = P.candidate_arrays(big, ext)
    entries = [e for e in S.entries(pool) if e.cand in names]
    lib = capi.load_planner()
    ck = make_checker(**FORMS[form])
    path = []
    try:
        for tick in range(S.N_TICKS):
            o = oracle_tick(pool, tick, big, ext)
            h = product_snapshot(P, tick)
            try:
                p = plan_arrays(ck, h, P.sc.ptr, cand_off, cand_pods)
                t = ck.timing()
                q = plan_arrays(ck, h, P.sc.ptr, cand_off, cand_pods, full=False)  # winner only
            finally:
                lib.sr_snapshot_destroy(h)
            path.append((t.enc_reused, t.k0_columns, t.k0_dirty_nodes, t.enc_pod_patches))
            print("%s %s t%d: enc_reused %d k0_columns %d k0_dirty_nodes %d enc_pod_patches %d k2_coop %d" % (
                pool, form, tick, t.enc_reused, t.k0_columns, t.k0_dirty_nodes, t.enc_pod_patches, t.k2_coop))
            assert np.array_equal(p.status, o["status"]), (tick, p.status, o["status"])
            bad = np.flatnonzero(p.node_of_pod != o["node_of_pod"])
            assert bad.size == 0, (tick, bad[:8], p.node_of_pod[bad[:8]], o["node_of_pod"][bad[:8]])
            assert (p.winner, p.first_ok, p.first_fallback) == (o["winner"], o["first_ok"], o["first_fallback"]), tick
            for c, name in enumerate(names):
                assert int(p.status[c]) == S.expected_status(pool, tick, name), (tick, name)
            for e in entries:
                if e.tick == tick:
                    k, _ = pod_slot(pool, e.cand, e.pod, big, ext)
                    assert int(p.node_of_pod[k]) == (-1 if e.now is None else e.now), e
            assert (q.winner, q.first_ok, q.first_fallback) == (p.winner, p.first_ok, p.first_fallback), tick
            assert np.array_equal(q.winner_map, p.winner_map) and np.array_equal(p.winner_map, o["winner_map"]), tick
            if tick >= 2 and form != "one_slot":
                assert t.enc_reused == 1, (tick, t.enc_reused)
            if form == "default":
                if tick in S.K0_LESS:
                    n = len(S.changed_nodes(pool, S.TABLES_OF[tick], tick))
                    assert (t.k0_columns, t.k0_dirty_nodes) == (-2, n), (tick, t.k0_columns, t.k0_dirty_nodes, n)
                if tick == S.K0_TICK:
                    assert t.k0_columns >= 0, (tick, t.k0_columns)
            if form == "k0_skip_off" and tick >= 2:
                assert t.k0_columns >= 0, (tick, t.k0_columns)
            if form == "k0_full" and tick >= 2:
                assert t.k0_columns == -1, (tick, t.k0_columns)
            if form == "coop" and any(e.tick == tick for e in entries):
                assert t.k2_coop > 0, (tick, t.k2_coop)
        if form == "default":  # some K0-less tick re-pointed pods: the K0 of the 17th node applies them
            assert sum(x[3] for x in path[2:S.K0_TICK]) > 0, path
    finally:
        ck.close()
        record_property("path", str(path))
