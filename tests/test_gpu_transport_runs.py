"""The two-rank transports under the load the single-rank planner is tested
with: many runs of one prepared workload, workloads that grow between ticks,
the non-default K2 dispatch forms, and shards with gaps between them.

With more than one rank K2 writes its outcomes elsewhere than on a single
rank: `res_stat` into the shared-memory segment and `res_map` into h_early
(sr_comm_init_shm, the bench's transport on one node: each rank's host walks
every rank's words, no collective, no K3), or nowhere (sr_comm_init_host: K3
after an allreduce(min) of d_min, here over gloo).  Two spawned workers plan
their shards through both transports; the parent compares what they gathered
with the oracle (rescheduler.go:228-287 evaluates the same candidates
serially and drains the first whose pods all fit).

A. consecutive runs of one prepared workload (test_consecutive_runs_match_oracle
   through the transports): 6 ticks x 40 sr_plan_run calls per config --
   winner-only, full and K2-timed runs interleaved -- each checked; under shm
   the 240 runs of a planner reuse each parity region of the segment 120 times.
B. a larger prepare right after a winner-only run: the run returns at the
   winner while K2 still plans the candidates after it, and the next prepare
   reallocates the arena, h_early and the output buffers (it must wait for K2
   first: sr_ctx::in_flight).  Also a shard larger than the segment's
   max_cand: refused, and a fresh planner and segment plan it.
C. the split launch, the cost-ordered list and cooperative blocks
   (test_gpu_k2_dispatch's thresholds) through both transports: both K2
   kernels of the split write the segment's words and d_min.
D. uneven shards: rank 0 plans global {0, 2, 4}, rank 1 {5, 7} or nothing;
   the reduced first_ok is the smallest drainable index among the planned ones.
E. sr_plan_first's prefix batches between the ticks of A on the same planner."""
import queue
import time

import numpy as np
import pytest

from test_gpu_distributed import _check_first, _free_port, _run_first

pytestmark = pytest.mark.gpu
WORLD = 2

A_CONFIGS = (3, 5)
A_TICKS, A_RUNS = 6, 40
A_FIRST_TICKS = (3, 4)                      # E: sr_plan_first before these ticks' prepare (config 3)
B_SEED = 48
B_ORDER = ("small", "all", "small", "larger", "all")
C_ENV = dict(SR_K2_SPLIT_MIN=64, SR_LIST_COST_MIN=0, SR_K2_WPB=4, SR_K2_COOP=32)
C_TICKS = 8
D_PLANNED = ((0, 2, 4), (5, 7))             # global indices per rank
# drainable global indices (the unplanned 1, 3, 6 always are: they must not count), rank 1 plans nothing
D_INPUTS = [((1, 2, 3, 5, 6, 7), False), ((1, 3, 5, 6, 7), False), ((1, 3, 6, 7), False), ((1, 3, 6), False),
            ((1, 3, 4, 5, 6), True)]
D_EXPECT = [2, 5, 7, -1, 4]


def _a_cluster(config):
    from spotplanner.synth import SynthCluster
    return SynthCluster(config, seed=47, n_on_demand=240, n_spot=600)


def _b_clusters():
    from spotplanner.synth import SynthCluster
    return (SynthCluster(3, seed=B_SEED, n_on_demand=300, n_spot=600),
            SynthCluster(3, seed=B_SEED, n_on_demand=400, n_spot=1200))


def _c_cluster():
    from spotplanner.synth import AFFINITY, SynthCluster
    return SynthCluster(3, seed=41, n_on_demand=300, n_spot=600, **AFFINITY)


def _candidates(sc):
    from spotplanner import capi
    from spotplanner.synth import build_candidates, new_node_map
    lib = capi.load_planner()
    nm = new_node_map(lib.sr_new_node_map, sc.ptr, sc.n_nodes, sc.n_pods, sc.od_label, sc.spot_label)
    cand_off, cand_pods = build_candidates(nm, sc.pod_flags())
    return nm, cand_off, cand_pods


def _prefix(cand_off, cand_pods, n):
    return cand_off[:n + 1], cand_pods[:int(cand_off[n])]


def _d_scenario(drainable):
    """3 spot nodes, 8 one-pod candidates: 100 mCPU (drainable) or more than any node holds."""
    from helpers import Scenario
    from spotplanner.model import Container, Node, Pod
    nodes = [Node("spot%d" % i, cpu_milli=4000) for i in range(3)]
    pods = [Pod("c%d" % g, namespace="default", containers=[Container(cpu_milli=100 if g in drainable else 10 ** 7)])
            for g in range(8)]
    return Scenario(nodes, [[], [], []], pods)


def _d_shard(sc, planned):
    loff = np.arange(len(planned) + 1, dtype=np.int32)
    lpods = np.asarray([sc.q0 + g for g in planned], np.int32)
    return loff, lpods, np.asarray(planned, np.int32)


def _plan_dict(p, loff, gidx, full=True):
    d = dict(first_ok=int(p.first_ok), first_fallback=int(p.first_fallback), winner=int(p.winner),
             wmap=[int(x) for x in p.winner_map] if len(p.winner_map) else None)
    if full:
        d["mine"] = {int(g): (int(s), [int(x) for x in p.node_of_pod[loff[k]:loff[k + 1]]])
                     for k, (g, s) in enumerate(zip(gidx, p.status))}
    return d


def _work(rank, world, port, transport):
    """Everything one rank plans; returns its results.  Any failed status raises: nothing more is started."""
    import ctypes
    import os

    import torch
    import torch.distributed as dist

    from spotplanner import capi
    from spotplanner.planner import PredicateChecker
    from spotplanner.rescheduler import plan_arrays
    from spotplanner.synth import shard
    from test_gpu_k2_dispatch import make_checker
    from test_gpu_ticks import _with_extra

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    bias = 1 << 63

    def allreduce_min(vals):  # uint64 words: order-preserving shift into int64
        t = torch.tensor([v - bias for v in vals], dtype=torch.int64)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return [int(x) + bias for x in t]

    def attach(ck, name, max_cand=4096):
        if transport == "shm":  # one segment per planner, the same name and session on both ranks
            ck.attach_shared_memory("/srruns-%d-%s" % (port, name), port * 7919, world, rank, max_cand)
        else:
            ck.attach_collective(world, rank, allreduce_min)

    lib = capi.load_planner()

    def snapshot(sc, nm, off, idx):
        h = ctypes.c_void_p()
        assert lib.sr_snapshot_create(sc.ptr, capi.ptr(nm.spot, capi.P32), len(nm.spot), capi.ptr(off, capi.P32),
                                      capi.ptr(idx, capi.P32), ctypes.byref(h)) == capi.SR_OK
        return h

    results = {"transport": transport}
    cks = {"a3": make_checker(SR_PREFIX_BATCH=2), "a5": PredicateChecker(0), "b": PredicateChecker(0),
           "b16": PredicateChecker(0), "c": make_checker(**C_ENV), "d": PredicateChecker(0)}
    for name, ck in cks.items():
        attach(ck, name, 16 if name == "b16" else 4096)
    dist.barrier()  # every rank attached before any plans (or rank 0's planner could unlink the name)

    # ---- A (and E): consecutive runs of one prepared workload, a pod more on a spot node every tick
    for config in A_CONFIGS:
        ck = cks["a%d" % config]
        sc = _a_cluster(config)
        nm, cand_off, cand_pods = _candidates(sc)
        loff, lpods, gidx = shard(cand_off, cand_pods, rank, world)
        n = len(loff) - 1
        c = capi.sr_candidates(n, capi.ptr(loff, capi.P32), capi.ptr(lpods, capi.P32), capi.ptr(gidx, capi.P32))
        wmap = np.full(int(np.max(np.diff(loff))), -1, np.int32)
        status = np.zeros(n, np.int32)
        nodes = np.zeros(int(loff[-1]), np.int32)
        rng = np.random.default_rng(config)  # the same changes on both ranks
        extra, ticks = [], []
        for tick in range(A_TICKS):
            if tick:
                extra.append((int(rng.choice(cand_pods)), int(rng.integers(len(nm.spot)))))
            off, idx = _with_extra(nm, sc.n_nodes, extra)
            h = snapshot(sc, nm, off, idx)
            if config == 3 and tick in A_FIRST_TICKS:  # the prefix batches take other workload slots
                results[("E", tick)] = _run_first(lib, ck, h, sc.ptr, loff, lpods, gidx)
            for _ in range(2 if tick == 0 else 1):
                assert lib.sr_plan_prepare(ck.handle, h, sc.ptr, ctypes.byref(c)) == capi.SR_OK, ck.last_error()
            tm = ck.timing()
            runs = []
            for r in range(A_RUNS):
                out = capi.sr_plan_out()
                out.winner_map = capi.ptr(wmap, capi.P32)
                full = r % 13 == 5
                if full:
                    out.status = capi.ptr(status, capi.P32)
                    out.node_of_pod = capi.ptr(nodes, capi.P32)
                timed = r % 11 == 7
                if timed:
                    ck.set_timing(2)
                assert lib.sr_plan_run(ck.handle, ctypes.byref(out)) == capi.SR_OK, ck.last_error()
                if timed:
                    assert ck.timing().n_runs == 1
                    ck.set_timing(0)
                rec = dict(first_ok=int(out.first_ok), first_fallback=int(out.first_fallback),
                           winner=int(out.winner), npods=int(out.winner_npods),
                           wmap=[int(x) for x in wmap[:out.winner_npods]] if out.winner_npods > 0 else None)
                if full:
                    rec["mine"] = {int(g): (int(status[k]), [int(x) for x in nodes[loff[k]:loff[k + 1]]])
                                   for k, g in enumerate(gidx)}
                runs.append(rec)
            ticks.append(dict(extra=list(extra), k0=int(tm.k0_columns), reused=int(tm.enc_reused), runs=runs))
            lib.sr_snapshot_destroy(h)
        results[("A", config)] = ticks

    # ---- B: winner-only runs, each followed at once by a prepare of another size
    ck = cks["b"]
    c1, c2 = _b_clusters()
    nm1, off1, pods1 = _candidates(c1)
    nm2, off2, pods2 = _candidates(c2)
    inputs = {"small": (c1, shard(*_prefix(off1, pods1, 40), rank, world)),
              "all": (c1, shard(off1, pods1, rank, world)),
              "larger": (c2, shard(off2, pods2, rank, world))}
    snaps = {id(c1): snapshot(c1, nm1, nm1.node_pod_off, nm1.node_pod_idx),
             id(c2): snapshot(c2, nm2, nm2.node_pod_off, nm2.node_pod_idx)}
    b_ticks = []
    for name in B_ORDER:  # no barrier, no other work between a run's return and the next prepare
        sc, (loff, lpods, gidx) = inputs[name]
        q = plan_arrays(ck, snaps[id(sc)], sc.ptr, loff, lpods, cand_global=gidx, full=False)
        b_ticks.append((q.first_ok, q.first_fallback, q.winner, [int(x) for x in q.winner_map]))
    sc, (loff, lpods, gidx) = inputs["all"]
    p = plan_arrays(ck, snaps[id(sc)], sc.ptr, loff, lpods, cand_global=gidx)
    results[("B",)] = dict(ticks=[(int(a), int(b), int(c_), m) for a, b, c_, m in b_ticks],
                           full=_plan_dict(p, loff, gidx))
    # a shard of 17 candidates through a 16-entry segment, then the same through a fresh planner and segment
    loff, lpods, gidx = shard(*_prefix(off1, pods1, 34), rank, world)
    assert len(gidx) == 17
    c = capi.sr_candidates(17, capi.ptr(loff, capi.P32), capi.ptr(lpods, capi.P32), capi.ptr(gidx, capi.P32))
    wmap = np.full(int(np.max(np.diff(loff))), -1, np.int32)
    o = capi.sr_plan_out()
    o.winner_map = capi.ptr(wmap, capi.P32)
    st = lib.sr_plan(cks["b16"].handle, snaps[id(c1)], c1.ptr, ctypes.byref(c), ctypes.byref(o))
    refused = dict(status=int(st), error=cks["b16"].last_error() if st != capi.SR_OK else "")
    cks["fresh"] = PredicateChecker(0)
    attach(cks["fresh"], "fresh")
    dist.barrier()
    p = plan_arrays(cks["fresh"], snaps[id(c1)], c1.ptr, loff, lpods, cand_global=gidx)
    results[("B", "refused")] = dict(refused=refused, fresh=_plan_dict(p, loff, gidx))
    for h in snaps.values():
        lib.sr_snapshot_destroy(h)

    # ---- C: split launch, cost order, cooperative blocks
    ck = cks["c"]
    sc = _c_cluster()
    nm, cand_off, cand_pods = _candidates(sc)
    loff, lpods, gidx = shard(cand_off, cand_pods, rank, world)
    rng = np.random.default_rng(41)
    extra, c_ticks = [], []
    for tick in range(C_TICKS):
        if tick == 5:
            extra.clear()
        if tick:
            for _ in range(int(rng.integers(1, 4))):
                extra.append((int(rng.choice(cand_pods)), int(rng.integers(len(nm.spot)))))
        off, idx = _with_extra(nm, sc.n_nodes, extra)
        h = snapshot(sc, nm, off, idx)
        q = plan_arrays(ck, h, sc.ptr, loff, lpods, cand_global=gidx, full=False)
        tq = ck.timing()
        p = plan_arrays(ck, h, sc.ptr, loff, lpods, cand_global=gidx)
        tp = ck.timing()
        lib.sr_snapshot_destroy(h)
        c_ticks.append(dict(extra=list(extra), q=_plan_dict(q, loff, gidx, full=False), p=_plan_dict(p, loff, gidx),
                            forms=[(int(t.k2_launches), int(t.k2_list_by_cost), int(t.k2_coop)) for t in (tq, tp)]))
    results[("C",)] = c_ticks

    # ---- D: shards with a gap between them, and a rank that plans nothing
    ck = cks["d"]
    for i, (drainable, rank1_empty) in enumerate(D_INPUTS):
        sc = _d_scenario(drainable)
        planned = D_PLANNED[rank] if not (rank == 1 and rank1_empty) else ()
        loff, lpods, gidx = _d_shard(sc, planned)
        h = sc.product_snapshot()
        q = plan_arrays(ck, h, sc.ptr, loff, lpods, cand_global=gidx, full=False)
        p = plan_arrays(ck, h, sc.ptr, loff, lpods, cand_global=gidx)
        lib.sr_snapshot_destroy(h)
        results[("D", i)] = dict(q=_plan_dict(q, loff, gidx, full=False), p=_plan_dict(p, loff, gidx))

    dist.barrier()  # no rank closes (rank 0: unlinks) a segment another still plans through
    for ck in cks.values():
        ck.close()
    gathered = [None] * world
    dist.all_gather_object(gathered, results)
    dist.destroy_process_group()
    return gathered


def _worker(rank, world, port, out, transport):
    import os
    import sys
    import traceback
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(repo, "k8s-spot-rescheduler_amd"), os.path.join(repo, "tests")]
    try:
        gathered = _work(rank, world, port, transport)
        if rank == 0:
            out.put(("ok", gathered))
    except BaseException:  # noqa: BLE001 -- the parent fails at once with this text; nothing more runs here
        out.put(("error", "rank %d:\n%s" % (rank, traceback.format_exc())))
        out.close()
        out.join_thread()
        os._exit(1)  # (no teardown that could wait for the other rank)


@pytest.fixture(scope="module", params=["host_fn", "shm"])
def runs(request):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, q, request.param)) for r in range(WORLD)]
    t0 = time.monotonic()
    try:
        for p in procs:
            p.start()
        msg, dead = None, []
        while msg is None:
            try:
                msg = q.get(timeout=2 if dead else 0.5)
            except queue.Empty:
                # (a worker that raised has flushed its traceback before it exits: one more look after a death)
                assert not dead, "a worker died without a message: exit codes %s" % dead
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert time.monotonic() - t0 < 240, "no result from the workers within 240 s"
        assert msg[0] == "ok", msg[1]
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0, p.exitcode
        return msg[1]
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
            if p.is_alive():
                p.kill()
                p.join(timeout=10)


def _oracle_with_extra(sc, nm, cand_off, cand_pods, extra):
    from oracle_lib import OracleSnapshot, oracle_plan
    from test_gpu_ticks import _with_extra
    off, idx = _with_extra(nm, sc.n_nodes, extra)
    return oracle_plan(OracleSnapshot(sc.ptr, nm.spot, off, idx), sc.ptr, cand_off, cand_pods, mode=1, threads=8)


def _seg(o, cand_off, c):
    return [int(x) for x in o["node_of_pod"][int(cand_off[c]):int(cand_off[c + 1])]]


def _check_reduced(per_rank, o, cand_off, where):
    """first_ok / first_fallback / winner on every rank, and the mapping from the owner alone."""
    want = (int(o["first_ok"]), int(o["first_fallback"]), int(o["winner"]))
    for r in per_rank:
        assert (r["first_ok"], r["first_fallback"], r["winner"]) == want, where
    owners = [k for k, r in enumerate(per_rank) if r["wmap"]]
    if want[0] >= 0:
        assert owners == [want[0] % WORLD], (where, owners)
        assert per_rank[owners[0]]["wmap"] == _seg(o, cand_off, want[0]), where
    else:
        assert owners == [], where


def _check_merged(per_rank, o, cand_off, where, fallback_ok=False):
    """Every candidate's status and mapping, merged over the ranks."""
    from spotplanner import capi
    merged = {}
    for r in per_rank:
        merged.update(r["mine"])
    n = len(cand_off) - 1
    assert sorted(merged) == list(range(n)), where
    for c in range(n):
        s, m = merged[c]
        if fallback_ok and s == capi.SR_CAND_FALLBACK:
            continue
        assert s == int(o["status"][c]), (where, c)
        assert m == _seg(o, cand_off, c), (where, c)


@pytest.mark.parametrize("config", A_CONFIGS)
def test_consecutive_runs_match_oracle_on_two_ranks(runs, config):
    """A: every one of the 240 runs per rank returns the oracle's first_ok,
    first_fallback and winner; exactly the rank first_ok % 2 returns the
    mapping, the oracle's; the full runs' merged statuses and mappings are the
    oracle's (candidates of C5 outside the encoded set may take the reference
    path, as in test_consecutive_runs_match_oracle).  The candidate side is
    reused from the third tick and at least 3 ticks per rank launch no K0."""
    sc = _a_cluster(config)
    nm, cand_off, cand_pods = _candidates(sc)
    ticks = [res[("A", config)] for res in runs]
    assert all(len(t) == A_TICKS for t in ticks)
    n_full = 0
    for tick in range(A_TICKS):
        assert ticks[0][tick]["extra"] == ticks[1][tick]["extra"] and len(ticks[0][tick]["extra"]) == tick
        o = _oracle_with_extra(sc, nm, cand_off, cand_pods, ticks[0][tick]["extra"])
        for r in range(A_RUNS):
            per_rank = [t[tick]["runs"][r] for t in ticks]
            _check_reduced(per_rank, o, cand_off, (tick, r))
            for rank, rec in enumerate(per_rank):
                assert rec["npods"] == (len(_seg(o, cand_off, o["first_ok"]))
                                        if o["first_ok"] >= 0 and o["first_ok"] % WORLD == rank else 0), (tick, r)
            assert ("mine" in per_rank[0]) == ("mine" in per_rank[1]) == (r % 13 == 5)
            if r % 13 == 5:
                _check_merged(per_rank, o, cand_off, (tick, r), fallback_ok=config == 5)
                n_full += 1
        if tick >= 2:
            assert [t[tick]["reused"] for t in ticks] == [1] * WORLD, tick
    assert n_full == 3 * A_TICKS
    # K0-less ticks (K2 alone resets and sets the run's d_min words for the allreduce, or writes the
    # segment's words): at least 3 of the 6 on every rank, as test_consecutive_runs_match_oracle asks of one rank
    for rank, t in enumerate(ticks):
        k0 = [tk["k0"] for tk in t]
        print("rank %d k0_columns per tick: %s" % (rank, k0))
        assert sum(k == -2 for k in k0) >= 3, (rank, k0)


@pytest.mark.parametrize("tick", A_FIRST_TICKS)
def test_plan_first_between_ticks_of_one_planner(runs, tick):
    """E: sr_plan_first's prefix batches (batch size 2) on A's config-3 planner
    between two ticks equal the reference loop, and the tick prepared right
    after still reuses the candidate side."""
    from oracle_lib import OracleSnapshot, oracle_plan
    from test_gpu_ticks import _with_extra
    sc = _a_cluster(3)
    nm, cand_off, cand_pods = _candidates(sc)
    extra = runs[0][("A", 3)][tick]["extra"]
    off, idx = _with_extra(nm, sc.n_nodes, extra)
    osnap = OracleSnapshot(sc.ptr, nm.spot, off, idx)
    ref_all = oracle_plan(osnap, sc.ptr, cand_off, cand_pods, mode=1, threads=8)
    ref_early = oracle_plan(osnap, sc.ptr, cand_off, cand_pods, mode=0)
    print("prefix batches per rank:", [res[("E", tick)]["batches"] for res in runs], "first_ok", ref_all["first_ok"])
    _check_first(runs, ("E", tick), ref_all, ref_early, cand_off)
    assert all(res[("E", tick)]["batches"] >= 1 for res in runs)
    assert [res[("A", 3)][tick]["reused"] for res in runs] == [1] * WORLD


def test_larger_prepare_right_after_a_winner_only_run(runs):
    """B: small -> all -> small -> larger cluster -> all, each a winner-only
    sr_plan immediately followed by the next one's prepare, then a full run.
    In the all-candidate ticks the winner lies in the first tenth of the
    candidates (asserted from the oracle alone), so K2 has most of its list
    outstanding when the run returns."""
    from oracle_lib import OracleSnapshot, oracle_plan
    c1, c2 = _b_clusters()
    refs = {}
    for name, sc, lim in (("small", c1, 40), ("all", c1, None), ("larger", c2, None)):
        nm, cand_off, cand_pods = _candidates(sc)
        if lim:
            cand_off, cand_pods = _prefix(cand_off, cand_pods, lim)
        o = oracle_plan(OracleSnapshot(sc.ptr, nm.spot, nm.node_pod_off, nm.node_pod_idx), sc.ptr, cand_off,
                        cand_pods, mode=1, threads=8)
        refs[name] = (o, cand_off)
        if lim is None:
            assert 0 <= o["first_ok"] < (len(cand_off) - 1) // 10, (name, o["first_ok"])
    assert len(refs["larger"][1]) > len(refs["all"][1]) > len(refs["small"][1])
    for k, name in enumerate(B_ORDER):
        o, cand_off = refs[name]
        per_rank = [dict(zip(("first_ok", "first_fallback", "winner", "wmap"), res[("B",)]["ticks"][k]))
                    for res in runs]
        _check_reduced(per_rank, o, cand_off, (k, name))
    o, cand_off = refs["all"]
    full = [res[("B",)]["full"] for res in runs]
    _check_reduced(full, o, cand_off, "full")
    _check_merged(full, o, cand_off, "full")


def test_shard_beyond_the_segment_is_refused_and_a_fresh_planner_plans_it(runs):
    """B: 17 candidates per rank through a segment made for 16 are refused
    before anything is planned (SR_ERR_CAPACITY, as include/sr_planner.h
    documents for sr_comm_init_shm's max_cand) on both ranks alike; the same
    shards through a fresh planner and segment give the oracle's plan.  The
    gloo transport has no such bound and plans them."""
    from oracle_lib import OracleSnapshot, oracle_plan
    from spotplanner import capi
    c1, _ = _b_clusters()
    nm, cand_off, cand_pods = _candidates(c1)
    cand_off, cand_pods = _prefix(cand_off, cand_pods, 34)
    o = oracle_plan(OracleSnapshot(c1.ptr, nm.spot, nm.node_pod_off, nm.node_pod_idx), c1.ptr, cand_off, cand_pods,
                    mode=1, threads=8)
    for res in runs:
        refused = res[("B", "refused")]["refused"]
        print(res["transport"], refused)
        if res["transport"] == "shm":
            assert refused["status"] == capi.SR_ERR_CAPACITY, refused
            assert "max_cand" in refused["error"], refused
        else:
            assert refused["status"] == capi.SR_OK, refused
    fresh = [res[("B", "refused")]["fresh"] for res in runs]
    _check_reduced(fresh, o, cand_off, "fresh")
    _check_merged(fresh, o, cand_off, "fresh")


def test_dispatch_forms_through_the_transports(runs):
    """C: eight ticks of the affinity cluster through planners with the split
    launch, the cost-ordered list and cooperative blocks at test size: every
    tick's merged plan and reduced values are the oracle's, the winner-only
    run equals the full run, and each rank reached every form."""
    sc = _c_cluster()
    nm, cand_off, cand_pods = _candidates(sc)
    ticks = [res[("C",)] for res in runs]
    assert all(len(t) == C_TICKS for t in ticks)
    for tick in range(C_TICKS):
        assert ticks[0][tick]["extra"] == ticks[1][tick]["extra"]
        o = _oracle_with_extra(sc, nm, cand_off, cand_pods, ticks[0][tick]["extra"])
        full = [t[tick]["p"] for t in ticks]
        _check_reduced(full, o, cand_off, tick)
        _check_merged(full, o, cand_off, tick)
        for t in ticks:
            q, p = t[tick]["q"], t[tick]["p"]
            assert (q["first_ok"], q["first_fallback"], q["winner"], q["wmap"]) == \
                (p["first_ok"], p["first_fallback"], p["winner"], p["wmap"]), tick
    for rank, t in enumerate(ticks):
        forms = [f for tk in t for f in tk["forms"]]
        print("rank %d (k2_launches, k2_list_by_cost, k2_coop) per run: %s" % (rank, forms))
        assert all(launches == 2 for launches, _, _ in forms), (rank, forms)
        assert sum(by_cost > 0 for _, by_cost, _ in forms) >= 8, (rank, forms)
        assert sum(coop > 0 for _, _, coop in forms) >= 6, (rank, forms)


@pytest.mark.parametrize("which", range(len(D_INPUTS)))
def test_uneven_shards_reduce_to_the_smallest_planned_drainable_index(runs, which):
    """D: rank 0 plans global {0, 2, 4}, rank 1 {5, 7} (or nothing): both ranks
    report the smallest drainable index among the planned ones -- 2, 5, 7,
    none, and 4 with the empty rank -- winner-only and in full, whatever
    indices lie unplanned in between (1 and 3 are drainable and must not
    count; a walk that stopped at the unplanned 1 reported none); only the
    owner returns the mapping."""
    from oracle_lib import oracle_plan
    drainable, rank1_empty = D_INPUTS[which]
    planned = sorted(D_PLANNED[0] + (() if rank1_empty else D_PLANNED[1]))
    want = min([g for g in planned if g in drainable], default=-1)
    assert want == D_EXPECT[which]
    sc = _d_scenario(drainable)
    loff, lpods, gidx = _d_shard(sc, planned)
    o = oracle_plan(sc.oracle_snapshot(), sc.ptr, loff, lpods, mode=1, cand_global=gidx)
    assert (o["first_ok"], o["first_fallback"], o["winner"]) == (want, -1, want)
    owner = None if want < 0 else (0 if want in D_PLANNED[0] else 1)
    for mode in ("q", "p"):
        per_rank = [res[("D", which)][mode] for res in runs]
        for rank, r in enumerate(per_rank):
            assert (r["first_ok"], r["first_fallback"], r["winner"]) == (want, -1, want), (mode, rank, r)
            if rank == owner:
                assert r["wmap"] == [int(x) for x in o["winner_map"]] == [0], (mode, rank, r)
            else:
                assert r["wmap"] is None, (mode, rank, r)
    merged = {}
    for res in runs:
        merged.update(res[("D", which)]["p"]["mine"])
    assert sorted(merged) == planned
    for k, g in enumerate(planned):
        assert merged[g] == (int(o["status"][k]), [int(o["node_of_pod"][k])]), g
