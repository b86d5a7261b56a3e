#!/usr/bin/env python3
"""sr_plan_sequence timing on the synthetic configs (tools only; GPU).

Per config and budget (1, 8, 64, unlimited), on a fresh snapshot each time:
the host-to-host time of one sr_plan_sequence call (median of --reps calls,
the first of a budget on a planner that has already seen the input), its
rounds / rounds with K0 / rounds that kept the candidate side, and the round
times of the same pass replayed one round per call (max_drains = 1, first_cand
behind the previous drain, same snapshot: the drains are the same), with the
medians of each round's prepare (sr_timing.ms_pack_host / ms_upload) and, for
scale, of a winner-only sr_plan of the whole list on the final snapshot.  In the
same process the reference pass on the oracle, single thread, is timed and
compared (drains, statuses, mappings): the baseline of the speed-up.  One JSON
line per config and budget.

--pdb MODE times sr_plan_sequence_pdb instead (MODE none: sr_plan_sequence, as
above).  Every candidate gets a home group out of 8, three quarters of its pods
belong to it and the rest to none.  `loose`: allowances of 2**30, which never
bind -- the drains are sr_plan_sequence's, and each repetition also times a
plain sr_plan_sequence call right before the limited one (ms_plain_*: the price
of waiting for the ledger step's words instead of returning at K2's winner).
`tight`: every group allows n_cand * 4 // 150 evictions (40 on config 3, 400 on
config 4), which on the oracle refuses about half of the candidates that would
have drained (config 3: 100 drains, 89 refused candidates drainable where the
pass met them; config 4: 1,024 and 918); the baseline is the oracle's limited
pass (sequence_pdb_ref.py) on one thread.

  python tools/sequence_bench.py [--configs 3,4] [--budgets 1,8,64,0] [--reps 5] [--no-oracle] [--out FILE]
                                 [--pdb none|loose|tight]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "k8s-spot-rescheduler_amd")]

import numpy as np  # noqa: E402

from sequence_pdb_ref import reference_sequence_pdb  # noqa: E402
from sequence_ref import from_synth, reference_sequence  # noqa: E402
from spotplanner import capi  # noqa: E402
from spotplanner.planner import PredicateChecker  # noqa: E402
from spotplanner.rescheduler import PdbLimits, plan_arrays, plan_sequence_arrays  # noqa: E402
from spotplanner.synth import SynthCluster  # noqa: E402


PDB_GROUPS = 8


def pdb_limits(inp, mode):
    """The groups of --pdb MODE (see above); None for `none`."""
    if mode == "none":
        return None
    r = np.random.RandomState(1)
    n = len(inp.cand_off) - 1
    pod_group = np.repeat(r.randint(0, PDB_GROUPS, n), np.diff(inp.cand_off)).astype(np.int32)
    pod_group[r.random_sample(len(pod_group)) < 0.25] = -1
    allowed = 2 ** 30 if mode == "loose" else max(1, n * 4 // 150)
    return PdbLimits(np.full(PDB_GROUPS, allowed, np.int32), pod_group)


def one_call(ck, inp, budget, limits=None):
    h = inp.product_snapshot()
    try:
        t0 = time.perf_counter()
        r = plan_sequence_arrays(ck, h, inp.ptr, inp.cand_off, inp.cand_pods, budget, limits=limits)
        return (time.perf_counter() - t0) * 1e3, r
    finally:
        capi.load_planner().sr_snapshot_destroy(h)


def round_by_round(ck, inp, budget, limits=None):
    """The same pass, one round per call: per-round host-to-host times (ms) and the drains.  With limits each
    call goes on with what the call before left of the allowances."""
    h = inp.product_snapshot()
    times, pack, upload, drained, first = [], [], [], [], 0
    n = len(inp.cand_off) - 1
    try:
        while first < n and (budget is None or len(drained) < budget):
            t0 = time.perf_counter()
            r = plan_sequence_arrays(ck, h, inp.ptr, inp.cand_off, inp.cand_pods, 1, first, full=False,
                                     limits=limits)
            times.append((time.perf_counter() - t0) * 1e3)
            if limits is not None:
                limits = PdbLimits(r.remaining, limits.pod_group)
            t = ck.timing()  # the round's prepare: host phase (encode, wait for the previous K2), upload calls
            pack.append(t.ms_pack_host)
            upload.append(t.ms_upload)
            if len(r.drained) == 0:
                break
            drained.append(int(r.drained[0]))
            first = drained[-1] + 1
        # for scale: winner-only plans of the whole list on the snapshot as it now stands (no commit in between)
        plan = []
        for _ in range(9):
            t0 = time.perf_counter()
            plan_arrays(ck, h, inp.ptr, inp.cand_off, inp.cand_pods, full=False)
            plan.append((time.perf_counter() - t0) * 1e3)
    finally:
        capi.load_planner().sr_snapshot_destroy(h)
    return times, drained, statistics.median(pack), statistics.median(upload), statistics.median(plan[2:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="3")
    ap.add_argument("--budgets", default="1,8,64,0", help="0 = unlimited")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--pdb", default="none", choices=["none", "loose", "tight"])
    args = ap.parse_args()
    ck = PredicateChecker(0)
    for config in [int(x) for x in args.configs.split(",")]:
        inp = from_synth(SynthCluster(config))
        n = len(inp.cand_off) - 1
        limits = pdb_limits(inp, args.pdb)
        for b in [int(x) for x in args.budgets.split(",")]:
            budget = b if b > 0 else None
            one_call(ck, inp, budget, limits)  # the planner has seen the input (and, twice over, reuses its candidate side)
            one_call(ck, inp, budget, limits)
            runs, plain_ms = [], []
            for _ in range(args.reps):
                if args.pdb == "loose":  # interleaved: the plain call right before the limited one
                    plain_ms.append(one_call(ck, inp, budget)[0])
                runs.append(one_call(ck, inp, budget, limits))
            ms = [t for t, _ in runs]
            r = runs[-1][1]
            rt, rd, pack, upload, plan = round_by_round(ck, inp, budget, limits)
            assert rd == [int(x) for x in r.drained], "round-by-round replay drains differ"
            line = dict(pdb=args.pdb, config=config, n_cand=n, n_spot=len(inp.spot), budget=b, n_drained=len(r.drained), stop=r.stop,
                        rounds=r.rounds, rounds_k0=r.rounds_k0, rounds_reused=r.rounds_reused,
                        ms_total_median=round(statistics.median(ms), 4), ms_total_min=round(min(ms), 4),
                        ms_total_max=round(max(ms), 4), reps=args.reps,
                        ms_round_median=round(statistics.median(rt), 4), ms_round_worst=round(max(rt), 4),
                        ms_round_first=round(rt[0], 4), replay_rounds=len(rt),
                        ms_round_prepare_host_median=round(pack, 4), ms_round_upload_median=round(upload, 4),
                        ms_plan_whole_list_winner_only=round(plan, 4))
            if limits is not None:
                line["refused"] = int(np.sum(r.status == capi.SR_CAND_PDB))
            if plain_ms:
                prt = round_by_round(ck, inp, budget)[0]
                line.update(ms_plain_total_median=round(statistics.median(plain_ms), 4),
                            ms_plain_total_min=round(min(plain_ms), 4), ms_plain_total_max=round(max(plain_ms), 4),
                            ms_plain_round_median=round(statistics.median(prt), 4))
            if not args.no_oracle:
                osnap = inp.oracle_snapshot()
                t0 = time.perf_counter()
                if limits is None:
                    ref = reference_sequence(osnap, inp.ptr, inp.cand_off, inp.cand_pods, budget)
                else:
                    ref = reference_sequence_pdb(osnap, inp.ptr, inp.cand_off, inp.cand_pods, limits.allowed,
                                                 limits.pod_group, budget)
                line["ms_oracle_1thread"] = round((time.perf_counter() - t0) * 1e3, 3)
                osnap.close()
                same = (list(ref.drained) == list(r.drained) and ref.stop == r.stop and
                        np.array_equal(ref.status, r.status) and np.array_equal(ref.node_of_pod, r.node_of_pod))
                if limits is not None:
                    same = same and np.array_equal(ref.remaining, r.remaining)
                line["matches_oracle"] = bool(same)
                line["speedup_vs_oracle"] = round(line["ms_oracle_1thread"] / line["ms_total_median"], 2)
            text = json.dumps(line)
            print(text, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(text + "\n")
    ck.close()


if __name__ == "__main__":
    main()
