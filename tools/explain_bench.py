#!/usr/bin/env python3
"""sr_explain_pods timing on a synthetic config (tools only; GPU).

A tick's plan (sr_plan, every candidate) names the failing pod of every
candidate that cannot drain.  One sr_explain_pods call then explains all of
those pods against the snapshot: timed host to host with and without the
per-node masks (median of --reps calls after two warm-up calls; the first
call's time, which builds the explain encoder's view of the pool, apart).  The
comparison is what the reference does at rescheduler.go:344-348, the oracle's
oracle_check_predicates over the same (pod, node) pairs on one thread; its
time includes one binding call per pair.  Every mask is checked against the
oracle's answer (mask == 0 iff yes).  One JSON line per config.

--plan times sr_explain_plan instead: after the tick's plan, host to host on
one box in one call, (a) one explain_plan_arrays call over the tick's status,
(b) the loop of explain_candidate_arrays over the same failing candidates,
which is what answers the question exactly without the batched entry point,
and (c) the sr_explain_pods call above, which answers it against the base
snapshot.  Each the median of --reps after two warm-up calls.  It reports the
failing candidates, how many stop at a pod k > 0, how many went each way
(`how`), and how many stop pods look feasible against the base snapshot but are
not in context; mask == 0 is checked against the oracle forked and filled the
same way, and (a) against (b) field for field.

--shortfall times sr_shortfall_pods on the same failing pods (with --plan:
sr_shortfall_plan on the same tick) beside its explain sibling, in one process:
counts only, with the per-node masks, and with node_short; the ratio of the
counts-only calls is the cost of asking "by how much" on top of "why".  `why`
is checked against the sibling array for array and the reductions against
numpy over node_mask / node_short.

--node-view times sr_node_view_plan on the tick's stuck candidates beside the one other route to the same
per-node numbers: sr_shortfall_plan with node_mask and node_short, folded over the candidates with numpy on the
host.  Both routes must give identical arrays; sr_shortfall_plan counts only is timed too, as the cost of the
same walk without the [n][n_spot] outputs.

--blockers times sr_blockers_plan on the tick's stuck candidates, with and without counts, beside (b) the only
other route to the same numbers -- the contract's loop on the host through the public calls, Fork, then per pod
sr_explain_pods of that pod alone and sr_snapshot_add_pod where it has a first node, Revert -- over a sample of
--sample stuck candidates (evenly spaced), scaled by stuck / sample, and (c) sr_explain_plan counts only, the
family's yardstick.  The sample's results must equal the call's; the way split and the distribution of blockers
per stuck candidate are reported, and the call is timed again asking for the batched candidates alone (the
device pass without the SINGLE candidates' per-pod calls).

--evacuate times sr_evacuate_plan on two workloads over the config's spot pool -- every spot node lost alone, and
ten pools (position j belongs to pool j % 10, the stand-in for an instance-type-in-a-zone label) -- each scenario
moving the pods of its lost nodes (DaemonSet and mirror pods left out), with and without counts, beside the only
other route to the same answer: sr_snapshot_create without the lost nodes, then sr_blockers_plan over the same
pods, over an evenly spaced sample of --sample scenarios scaled by scenarios / sample.  The sample's rows must
equal the call's; how many scenarios are JUDGED, NOT_PLAIN and FALLBACK is reported (--variant realistic: the
config with StatefulSet volumes, init containers and GPU pods).

  python tools/explain_bench.py [--configs 3] [--reps 9] [--no-oracle] [--out FILE] [--plan] [--shortfall]
                                [--node-view] [--blockers [--sample 40]] [--evacuate [--variant realistic]]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "k8s-spot-rescheduler_amd")]

import numpy as np  # noqa: E402

from oracle_lib import load_oracle  # noqa: E402
from sequence_ref import from_synth  # noqa: E402
from spotplanner import capi  # noqa: E402
from spotplanner.planner import PredicateChecker  # noqa: E402
from spotplanner.rescheduler import (blockers_plan_arrays, evacuate_plan_arrays, explain_arrays,  # noqa: E402
                                     explain_candidate_arrays, explain_plan_arrays, node_view_plan_arrays, plan_arrays, shortfall_arrays, shortfall_plan_arrays)
from spotplanner.synth import AFFINITY, REALISTIC, SynthCluster  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def median_of(fn, reps):
    for _ in range(2):
        fn()
    ms = [timed(fn)[0] for _ in range(reps)]
    return round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)


def plan_mode(args, ck, lib, config):
    inp = from_synth(SynthCluster(config))
    h = inp.product_snapshot()
    n_spot = len(inp.spot)
    off, cp = inp.cand_off, inp.cand_pods
    rel = off - off[0]  # node_of_pod is relative to cand_pod_off[0]
    try:
        plan = plan_arrays(ck, h, inp.ptr, off, cp)
        status, mapping = np.array(plan.status, np.int32), np.array(plan.node_of_pod, np.int32)
        failing = [c for c in range(len(status)) if status[c] >= 0]
        stops = np.array([cp[off[c] + status[c]] for c in failing], np.int32)

        def batched(mask=True):
            return explain_plan_arrays(ck, h, inp.ptr, off, cp, status, mapping, node_mask=mask)

        def loop(mask=True):
            return [explain_candidate_arrays(ck, h, inp.ptr, cp[off[c]:off[c + 1]], mapping[rel[c]:rel[c + 1]],
                                             int(status[c]), node_mask=mask) for c in failing]
        res, singles = batched(), loop()
        same = all(res.fallback[c] == one.fallback[0] and res.feasible[c] == one.feasible[0] and
                   res.first[c] == one.first[0] and np.array_equal(res.counts[c], one.counts[0]) and
                   np.array_equal(res.node_mask[c], one.node_mask[0]) for c, one in zip(failing, singles))
        base = explain_arrays(ck, h, inp.ptr, stops, node_mask=False)
        line = dict(config=config, mode="plan", n_cand=len(status), n_failing=len(failing), n_spot=n_spot,
                    failing_at_later_pod=int(np.sum(status > 0)),
                    how={name: int(np.sum(res.how == v)) for name, v in
                         (("none", capi.SR_EXPLAIN_NONE), ("batched", capi.SR_EXPLAIN_BATCHED),
                          ("single", capi.SR_EXPLAIN_SINGLE))},
                    fallback_stop_pods=int(res.fallback.sum()),
                    feasible_on_base_not_in_context=int(sum(
                        1 for i, c in enumerate(failing) if base.feasible[i] > 0 and res.feasible[c] == 0)),
                    batched_equals_loop=bool(same), reps=args.reps)
        print("# timing the batched call", file=sys.stderr, flush=True)
        for name, mask in (("with_node_mask", True), ("counts_only", False)):
            m = median_of(lambda: batched(mask), args.reps)
            line.update({"ms_explain_plan_%s_median" % name: m[0], "ms_explain_plan_%s_min" % name: m[1],
                         "ms_explain_plan_%s_max" % name: m[2]})
        print("# timing the per-candidate loop", file=sys.stderr, flush=True)
        m = median_of(loop, args.reps)
        line.update(ms_candidate_loop_median=m[0], ms_candidate_loop_min=m[1], ms_candidate_loop_max=m[2])
        m = median_of(lambda: explain_arrays(ck, h, inp.ptr, stops), args.reps)
        line.update(ms_explain_pods_base_median=m[0], ms_explain_pods_base_min=m[1], ms_explain_pods_base_max=m[2])
        if line["ms_explain_plan_with_node_mask_median"] > 0:
            line["ratio_loop_over_explain_plan"] = round(
                line["ms_candidate_loop_median"] / line["ms_explain_plan_with_node_mask_median"], 1)
    finally:
        lib.sr_snapshot_destroy(h)
    if not args.no_oracle and len(failing):
        print("# checking against the oracle", file=sys.stderr, flush=True)
        ora = load_oracle()
        osnap = inp.oracle_snapshot()
        ok = True
        for c in failing:
            if res.fallback[c]:
                continue
            assert ora.oracle_snapshot_fork(osnap.h) == 0
            for k in range(int(status[c])):
                ora.oracle_snapshot_add_pod(osnap.h, inp.ptr, int(cp[off[c] + k]), int(mapping[rel[c] + k]))
            pod = int(cp[off[c] + status[c]])
            fits = np.array([ora.oracle_check_predicates(osnap.h, inp.ptr, pod, j) for j in range(n_spot)], np.int32)
            ora.oracle_snapshot_revert(osnap.h)
            ok = ok and bool(np.array_equal(res.node_mask[c] == 0, fits == 1))
        osnap.close()
        line["matches_oracle_in_context"] = ok
    return line


def reductions_follow(why, short, rows):
    """near / only_nodes / only_min / only_at of `rows` recomputed with numpy from node_mask and node_short."""
    R = capi.SR_WHY_PODS | capi.SR_WHY_CPU | capi.SR_WHY_MEMORY | capi.SR_WHY_EPHEMERAL
    bits = (capi.SR_WHY_CPU, capi.SR_WHY_MEMORY, capi.SR_WHY_EPHEMERAL, capi.SR_WHY_PODS)
    for i in rows:
        m, s = why.node_mask[i].astype(np.int64), short.node_short[i]
        if why.fallback[i]:
            if short.near[i] != -1 or s.any():
                return False
            continue
        if short.near[i] != int(np.sum((m != 0) & ((m & ~R) == 0))):
            return False
        for d, bit in enumerate(bits):
            at = np.flatnonzero(m == bit)
            lo = int(s[at, d].min()) if len(at) else 0
            pos = int(at[np.argmax(s[at, d] == lo)]) if len(at) else -1
            if (short.only_nodes[i][d], short.only_min[i][d], short.only_at[i][d]) != (len(at), lo, pos):
                return False
            if ((s[:, d] != 0) != ((m & bit) != 0)).any():
                return False
    return True


def shortfall_mode(args, ck, lib, config):
    """--shortfall: sr_shortfall_pods (with --plan: sr_shortfall_plan) beside its explain sibling, in one process
    on the same queries: counts only, with the per-node masks, and with node_short as well."""
    inp = from_synth(SynthCluster(config))
    h = inp.product_snapshot()
    off, cp = inp.cand_off, inp.cand_pods
    try:
        plan = plan_arrays(ck, h, inp.ptr, off, cp)
        status, mapping = np.array(plan.status, np.int32), np.array(plan.node_of_pod, np.int32)
        failing = [c for c in range(len(status)) if status[c] >= 0]
        stops = np.array([cp[off[c] + status[c]] for c in failing], np.int32)
        if args.plan:
            def explain(mask):
                return explain_plan_arrays(ck, h, inp.ptr, off, cp, status, mapping, node_mask=mask)

            def shortfall(mask, node_short):
                return shortfall_plan_arrays(ck, h, inp.ptr, off, cp, status, mapping, node_short=node_short,
                                             node_mask=mask)
            rows = failing
        else:
            def explain(mask):
                return explain_arrays(ck, h, inp.ptr, stops, node_mask=mask)

            def shortfall(mask, node_short):
                return shortfall_arrays(ck, h, inp.ptr, stops, node_short=node_short, node_mask=mask)
            rows = range(len(stops))
        want = explain(True)
        why, short = shortfall(True, True)
        same = all(np.array_equal(getattr(why, f), getattr(want, f))
                   for f in ("feasible", "first", "counts", "fallback", "node_mask"))
        _, bare = shortfall(False, False)
        same_bare = all(np.array_equal(getattr(bare, f), getattr(short, f))
                        for f in ("near", "only_nodes", "only_min", "only_at"))
        judged = [i for i in rows if not why.fallback[i]]
        line = dict(config=config, mode="shortfall_plan" if args.plan else "shortfall", n_failing=len(failing),
                    n_spot=len(inp.spot), pairs=len(failing) * len(inp.spot), reps=args.reps,
                    why_equals_explain=bool(same), counts_only_equals_full=bool(same_bare),
                    reductions_follow_from_node_short=bool(reductions_follow(why, short, rows)),
                    queries_with_a_near_miss=int(sum(1 for i in judged if short.near[i] > 0)),
                    only_nodes={name: int(short.only_nodes[judged, d].sum()) for d, name in enumerate(capi.SHORT_NAMES)},
                    node_short_mib=round(len(rows) * len(inp.spot) * 32 / 2 ** 20, 1))
        del want, why, short, bare
        for name, fn in (("explain_counts_only", lambda: explain(False)),
                         ("explain_with_node_mask", lambda: explain(True)),
                         ("shortfall_counts_only", lambda: shortfall(False, False)),
                         ("shortfall_with_node_mask", lambda: shortfall(True, False)),
                         ("shortfall_with_node_short", lambda: shortfall(True, True))):
            print("# timing " + name, file=sys.stderr, flush=True)
            m = median_of(fn, args.reps)
            line.update({"ms_%s_median" % name: m[0], "ms_%s_min" % name: m[1], "ms_%s_max" % name: m[2]})
        if line["ms_explain_counts_only_median"] > 0:
            line["ratio_shortfall_over_explain_counts_only"] = round(
                line["ms_shortfall_counts_only_median"] / line["ms_explain_counts_only_median"], 2)
            line["ratio_shortfall_over_explain_with_node_mask"] = round(
                line["ms_shortfall_with_node_mask_median"] / line["ms_explain_with_node_mask_median"], 2)
    finally:
        lib.sr_snapshot_destroy(h)
    return line


def numpy_fold(why, short, status):
    """The per-node arrays of sr_node_view_plan from sr_shortfall_plan's node_mask / node_short, with numpy: the
    judged candidates (asked, not fallback) folded over axis 0; (shortfall, slot) compared lexicographically."""
    R = capi.SR_WHY_PODS | capi.SR_WHY_CPU | capi.SR_WHY_MEMORY | capi.SR_WHY_EPHEMERAL
    bits = (capi.SR_WHY_CPU, capi.SR_WHY_MEMORY, capi.SR_WHY_EPHEMERAL, capi.SR_WHY_PODS)
    q = np.flatnonzero((np.asarray(status) >= 0) & (why.fallback == 0))
    m = why.node_mask[q].astype(np.int64)          # [judged][n_spot]
    s = short.node_short[q]                         # [judged][n_spot][4]
    n_spot = m.shape[1]
    out = dict(judged=len(q), admits=(m == 0).sum(0), near=((m != 0) & ((m & ~R) == 0)).sum(0),
               refuses=np.stack([(m >> r & 1).sum(0) for r in range(capi.SR_WHY_COUNT)], 1),
               sole=np.stack([(m == 1 << r).sum(0) for r in range(capi.SR_WHY_COUNT)], 1),
               sole_min=np.zeros((n_spot, 4), np.int64), sole_at=np.full((n_spot, 4), -1, np.int32))
    big = np.iinfo(np.int64).max
    for d, bit in enumerate(bits):
        sole = m == bit
        if not len(q) or not sole.any():
            continue
        # a shortfall is at most INT64_MAX, which a sole query may hold: take the first row attaining the minimum
        # among the sole rows (the rows are in ascending slot order)
        v = np.where(sole, s[:, :, d], big)
        lo = v.min(0)
        first = np.argmax(sole & (v == lo), 0)
        has = sole.any(0)
        out["sole_min"][has, d] = lo[has]
        out["sole_at"][has, d] = q[first[has]]
    return out


def node_view_mode(args, ck, lib, config):
    inp = from_synth(SynthCluster(config))
    h = inp.product_snapshot()
    off, cp = inp.cand_off, inp.cand_pods
    try:
        plan = plan_arrays(ck, h, inp.ptr, off, cp)
        status, mapping = np.array(plan.status, np.int32), np.array(plan.node_of_pod, np.int32)
        failing = [c for c in range(len(status)) if status[c] >= 0]

        def view():
            return node_view_plan_arrays(ck, h, inp.ptr, off, cp, status, mapping)

        def route(fold=True):
            why, short = shortfall_plan_arrays(ck, h, inp.ptr, off, cp, status, mapping)
            return numpy_fold(why, short, status) if fold else None

        def counts_only():
            return shortfall_plan_arrays(ck, h, inp.ptr, off, cp, status, mapping, node_short=False, node_mask=False,
                                         why=False)
        res, want = view(), route()
        same = res.judged == want["judged"] and all(
            np.array_equal(getattr(res, f), want[f]) for f in ("admits", "near", "refuses", "sole", "sole_min", "sole_at"))
        n_spot = len(inp.spot)
        line = dict(config=config, mode="node_view_plan", n_cand=len(status), n_failing=len(failing), n_spot=n_spot,
                    judged=int(res.judged), pairs=len(failing) * n_spot, reps=args.reps,
                    both_routes_identical=bool(same),
                    how={name: int(np.sum(res.how == v)) for name, v in
                         (("none", capi.SR_EXPLAIN_NONE), ("batched", capi.SR_EXPLAIN_BATCHED),
                          ("single", capi.SR_EXPLAIN_SINGLE))},
                    nodes_admitting_none=int(np.sum(res.admits == 0)),
                    nodes_with_a_sole_reason=int(np.sum(res.sole.sum(1) > 0)),
                    sole={name: int(k) for name, k in zip(capi.WHY_NAMES, res.sole.sum(0)) if k},
                    node_mask_and_short_mib=round(len(status) * n_spot * 34 / 2 ** 20, 1),
                    node_view_download_kib=round(n_spot * 152 / 2 ** 10, 1))
        del want
        for name, fn in (("node_view_plan", view), ("shortfall_plan_counts_only", counts_only),
                         ("shortfall_plan_masks_and_short", lambda: route(False)),
                         ("shortfall_plan_masks_and_short_numpy_fold", route)):
            print("# timing " + name, file=sys.stderr, flush=True)
            m = median_of(fn, args.reps)
            line.update({"ms_%s_median" % name: m[0], "ms_%s_min" % name: m[1], "ms_%s_max" % name: m[2]})
        if line["ms_node_view_plan_median"] > 0:
            line["ratio_fold_route_over_node_view"] = round(
                line["ms_shortfall_plan_masks_and_short_numpy_fold_median"] / line["ms_node_view_plan_median"], 1)
    finally:
        lib.sr_snapshot_destroy(h)
    return line


def blockers_mode(args, ck, lib, config):
    inp = from_synth(SynthCluster(config))
    h = inp.product_snapshot()
    off, cp = inp.cand_off, inp.cand_pods
    try:
        plan = plan_arrays(ck, h, inp.ptr, off, cp)
        status, mapping = np.array(plan.status, np.int32), np.array(plan.node_of_pod, np.int32)
        stuck = [c for c in range(len(status)) if status[c] >= 0]
        step = max(1, len(stuck) // max(1, args.sample))
        sample = stuck[::step][:args.sample]

        def call(counts=True, ask=None):
            return blockers_plan_arrays(ck, h, inp.ptr, off, cp, status if ask is None else ask, counts=counts)

        def host_loop():
            out = {}
            for c in sample:
                assert lib.sr_snapshot_fork(h) == capi.SR_OK
                try:
                    row, rows = [], []
                    for p in cp[off[c]:off[c + 1]]:
                        one = explain_arrays(ck, h, inp.ptr, np.array([p], np.int32), node_mask=False)
                        row.append(int(one.first[0]))
                        rows.append(one.counts[0].copy() if one.first[0] < 0 else np.zeros(capi.SR_WHY_COUNT, np.int32))
                        if one.first[0] >= 0:
                            lib.sr_snapshot_add_pod(h, inp.ptr, int(p), int(one.first[0]))
                finally:
                    assert lib.sr_snapshot_revert(h) == capi.SR_OK
                out[c] = (row, rows)
            return out

        def counts_only():
            return explain_plan_arrays(ck, h, inp.ptr, off, cp, status, mapping, node_mask=False)
        res, loop = call(), host_loop()
        rel = off - off[0]
        same = all(list(res.node_of_pod[rel[c]:rel[c + 1]]) == row and
                   np.array_equal(res.counts[rel[c]:rel[c + 1]], np.array(rows).reshape(-1, capi.SR_WHY_COUNT))
                   for c, (row, rows) in loop.items())
        per = res.blockers[stuck]
        hist = {str(int(k)): int(v) for k, v in zip(*np.unique(per, return_counts=True))}
        line = dict(config=config, mode="blockers_plan", n_cand=len(status), n_stuck=len(stuck), n_spot=len(inp.spot),
                    pods_of_stuck=int(sum(off[c + 1] - off[c] for c in stuck)), reps=args.reps,
                    how={name: int(np.sum(res.how == v)) for name, v in
                         (("none", capi.SR_EXPLAIN_NONE), ("batched", capi.SR_EXPLAIN_BATCHED),
                          ("single", capi.SR_EXPLAIN_SINGLE))},
                    fallback=int(res.fallback.sum()), first_equals_status=bool(np.array_equal(res.first[stuck], status[stuck])),
                    blockers_per_stuck_candidate=hist, one_pod_away=int(np.sum(per == 1)),
                    median_blockers=float(np.median(per)) if len(per) else 0.0, max_blockers=int(per.max()) if len(per) else 0,
                    sample=len(sample), sample_equals_call=bool(same))
        only_batched = np.where(res.how == capi.SR_EXPLAIN_BATCHED, status, -1).astype(np.int32)
        line["pods_of_batched"] = int(sum(off[c + 1] - off[c] for c in stuck if res.how[c] == capi.SR_EXPLAIN_BATCHED))
        for name, fn in (("blockers_plan", call), ("blockers_plan_without_counts", lambda: call(False)),
                         ("blockers_plan_batched_candidates_only", lambda: call(True, only_batched)),
                         ("blockers_plan_batched_candidates_only_without_counts", lambda: call(False, only_batched)),
                         ("explain_plan_counts_only", counts_only), ("host_loop_sample", host_loop)):
            print("# timing " + name, file=sys.stderr, flush=True)
            m = median_of(fn, args.reps if name != "host_loop_sample" else min(args.reps, 3))
            line.update({"ms_%s_median" % name: m[0], "ms_%s_min" % name: m[1], "ms_%s_max" % name: m[2]})
        scale = len(stuck) / max(1, len(sample))
        line["ms_host_loop_scaled_to_all_stuck"] = round(line["ms_host_loop_sample_median"] * scale, 1)
        if line["ms_blockers_plan_median"] > 0:
            line["ratio_host_loop_over_blockers_plan"] = round(
                line["ms_host_loop_scaled_to_all_stuck"] / line["ms_blockers_plan_median"], 1)
    finally:
        lib.sr_snapshot_destroy(h)
    return line


def evacuate_mode(args, ck, lib, config):
    kw = {"realistic": REALISTIC, "affinity": AFFINITY}.get(args.variant, {})
    synth = SynthCluster(config, **kw)
    inp = from_synth(synth)
    h = inp.product_snapshot()
    n_spot = len(inp.spot)
    flags = synth.pod_flags()
    skip = capi.SR_POD_MIRROR | capi.SR_POD_DAEMONSET_CONTROLLER
    held = [[int(p) for p in inp.node_pod_idx[inp.node_pod_off[v]:inp.node_pod_off[v + 1]] if not flags[p] & skip]
            for v in inp.spot]

    def arrays(lost_sets):
        scen_off, pods, lost_off, lost_pos = [0], [], [0], []
        for lost in lost_sets:
            for j in lost:
                pods.extend(held[j])
            scen_off.append(len(pods))
            lost_pos.extend(lost)
            lost_off.append(len(lost_pos))
        return (np.array(scen_off, np.int32), np.array(pods, np.int32), np.array(lost_off, np.int32),
                np.array(lost_pos, np.int32))
    line = dict(config=config, variant=args.variant, mode="evacuate_plan", n_spot=n_spot, reps=args.reps,
                spot_pods_moved=int(sum(len(x) for x in held)))
    try:
        for name, lost_sets in (("n_minus_one", [[j] for j in range(n_spot)]),
                                ("ten_pools", [list(range(r, n_spot, 10)) for r in range(10)])):
            a = arrays(lost_sets)
            n = len(lost_sets)

            def call(counts=True):
                return evacuate_plan_arrays(ck, h, inp.ptr, *a, counts=counts)
            res = call()
            judged = [s for s in range(n) if res.how[s] == capi.SR_EVAC_JUDGED]
            step = max(1, len(judged) // max(1, args.sample))
            sample = judged[::step][:args.sample]

            def other_route():
                out = {}
                for s in sample:
                    keep = np.setdiff1d(np.arange(n_spot), lost_sets[s]).astype(np.int32)
                    spot = np.ascontiguousarray(inp.spot[keep], np.int32)
                    h2 = ctypes.c_void_p()
                    assert lib.sr_snapshot_create(inp.ptr, capi.ptr(spot, capi.P32), len(spot),
                                                  capi.ptr(inp.node_pod_off, capi.P32), capi.ptr(inp.node_pod_idx, capi.P32),
                                                  ctypes.byref(h2)) == capi.SR_OK
                    try:
                        pods = a[1][a[0][s]:a[0][s + 1]]
                        b = blockers_plan_arrays(ck, h2, inp.ptr, np.array([0, len(pods)], np.int32), pods,
                                                 np.zeros(1, np.int32))
                    finally:
                        lib.sr_snapshot_destroy(h2)
                    out[s] = (np.where(b.node_of_pod >= 0, keep[np.maximum(b.node_of_pod, 0)], -1), b.counts.copy(),
                              int(b.blockers[0]), int(b.fallback[0]))
                return out
            route = other_route()
            same = all(not fb and np.array_equal(res.node_of_pod[a[0][s]:a[0][s + 1]], row) and res.stranded[s] == k and
                       np.array_equal(res.counts[a[0][s]:a[0][s + 1]], cnt) for s, (row, cnt, k, fb) in route.items())
            d = dict(scenarios=n, pods=int(a[0][-1]), judged=len(judged),
                     not_plain=int(np.sum(res.how == capi.SR_EVAC_NOT_PLAIN)),
                     fallback=int(np.sum(res.how == capi.SR_EVAC_FALLBACK)),
                     scenarios_stranding=int(np.sum(res.stranded > 0)),
                     stranded_pods=int(res.stranded[res.stranded > 0].sum()),
                     worst=[int(s) for s in res.ranking()[:3]], sample=len(sample), sample_equals_call=bool(same))
            for label, fn in (("evacuate_plan", call), ("evacuate_plan_without_counts", lambda: call(False)),
                              ("other_route_sample", other_route)):
                print("# timing %s %s" % (name, label), file=sys.stderr, flush=True)
                m = median_of(fn, args.reps if label != "other_route_sample" else min(args.reps, 3))
                d.update({"ms_%s_median" % label: m[0], "ms_%s_min" % label: m[1], "ms_%s_max" % label: m[2]})
            d["ms_other_route_scaled_to_judged"] = round(d["ms_other_route_sample_median"] * len(judged) / max(1, len(sample)), 1)
            if d["ms_evacuate_plan_median"] > 0:
                d["ratio_other_route_over_evacuate_plan"] = round(d["ms_other_route_scaled_to_judged"] / d["ms_evacuate_plan_median"], 1)
            line[name] = d
            if not same:  # a number whose rows differ from the other route's is not published
                print(json.dumps(line), flush=True)
                raise SystemExit("evacuate: the other route's rows differ from the call's (%s)" % name)
    finally:
        lib.sr_snapshot_destroy(h)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="3")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--plan", action="store_true", help="time sr_explain_plan against the per-candidate loop")
    ap.add_argument("--shortfall", action="store_true",
                    help="time sr_shortfall_pods (with --plan: sr_shortfall_plan) beside its explain sibling")
    ap.add_argument("--node-view", action="store_true",
                    help="time sr_node_view_plan beside sr_shortfall_plan with node_mask / node_short and a numpy fold")
    ap.add_argument("--blockers", action="store_true",
                    help="time sr_blockers_plan beside the host loop of its contract and sr_explain_plan counts only")
    ap.add_argument("--sample", type=int, default=40,
                    help="--blockers: stuck candidates the host loop is timed over; --evacuate: scenarios of the other route")
    ap.add_argument("--evacuate", action="store_true",
                    help="time sr_evacuate_plan (every spot node lost alone; ten pools) beside sr_snapshot_create + sr_blockers_plan")
    ap.add_argument("--variant", default="baseline", choices=["baseline", "realistic", "affinity"],
                    help="--evacuate: the synthetic config's variant (bench.py's)")
    args = ap.parse_args()
    ck = PredicateChecker(0)
    lib = capi.load_planner()
    for config in [int(x) for x in args.configs.split(",")]:
        if args.evacuate or args.blockers or args.node_view or args.shortfall or args.plan:
            text = json.dumps(evacuate_mode(args, ck, lib, config) if args.evacuate
                              else blockers_mode(args, ck, lib, config) if args.blockers
                              else node_view_mode(args, ck, lib, config) if args.node_view
                              else shortfall_mode(args, ck, lib, config) if args.shortfall
                              else plan_mode(args, ck, lib, config))
            print(text, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(text + "\n")
            continue
        inp = from_synth(SynthCluster(config))
        h = inp.product_snapshot()
        try:
            plan = plan_arrays(ck, h, inp.ptr, inp.cand_off, inp.cand_pods)
            failing = [c for c in range(len(plan.status)) if plan.status[c] >= 0]
            pods = np.array([inp.cand_pods[inp.cand_off[c] + plan.status[c]] for c in failing], np.int32)
            n_spot = len(inp.spot)
            ms_first, res = timed(lambda: explain_arrays(ck, h, inp.ptr, pods))
            explain_arrays(ck, h, inp.ptr, pods, node_mask=False)
            with_mask = [timed(lambda: explain_arrays(ck, h, inp.ptr, pods))[0] for _ in range(args.reps)]
            without = [timed(lambda: explain_arrays(ck, h, inp.ptr, pods, node_mask=False))[0]
                       for _ in range(args.reps)]
            ms_plan = statistics.median(timed(lambda: plan_arrays(ck, h, inp.ptr, inp.cand_off, inp.cand_pods))[0]
                                        for _ in range(5))
        finally:
            lib.sr_snapshot_destroy(h)
        total = res.counts.sum(axis=0)
        line = dict(config=config, n_cand=len(plan.status), n_failing=len(failing), n_spot=n_spot,
                    pairs=len(failing) * n_spot, fallback_pods=int(res.fallback.sum()),
                    ms_first_call=round(ms_first, 3), reps=args.reps,
                    ms_with_node_mask_median=round(statistics.median(with_mask), 3),
                    ms_with_node_mask_min=round(min(with_mask), 3), ms_with_node_mask_max=round(max(with_mask), 3),
                    ms_counts_only_median=round(statistics.median(without), 3),
                    ms_counts_only_min=round(min(without), 3), ms_counts_only_max=round(max(without), 3),
                    ms_plan_every_candidate_median=round(ms_plan, 3),
                    reasons={name: int(k) for name, k in zip(capi.WHY_NAMES, total) if k})
        if not args.no_oracle and len(failing):
            ora = load_oracle()
            osnap = inp.oracle_snapshot()
            t0 = time.perf_counter()
            fits = np.array([[ora.oracle_check_predicates(osnap.h, inp.ptr, int(p), j) for j in range(n_spot)]
                             for p in pods], np.int32)
            line["ms_oracle_1thread"] = round((time.perf_counter() - t0) * 1e3, 1)
            osnap.close()
            judged = res.fallback == 0
            line["matches_oracle"] = bool(np.array_equal((res.node_mask[judged] == 0), fits[judged] == 1))
            line["ratio_oracle_over_explain_with_node_mask"] = round(
                line["ms_oracle_1thread"] / line["ms_with_node_mask_median"], 1)
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
    ck.close()


if __name__ == "__main__":
    main()
