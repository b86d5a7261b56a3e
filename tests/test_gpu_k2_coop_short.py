"""The winner's mapping from the wave's registers (SR_K2_MAP_REGS).

On a single rank a winner-only run returns once the host has walked K2's
per-candidate words up to the first drainable candidate and read that
candidate's mapping from `res_map`.  K2 stores those words from what the wave
still holds when it finishes -- the node-order kernel's per-lane registers
(pod 64 * g + lane in group g), the pod-order path's LDS mapping -- instead of
fencing its `out_node` stores and reading them back.

Every case runs consecutive ticks of one candidate input (one to three filler
pods more per tick on random spot nodes: K0-less ticks after the first, but
for one tick with 20 nodes changed at once, which launches K0 again), each
tick planned winner-only and in full, and
compares every status, every pod's node, first_ok / first_fallback / winner
and the winner-only mapping with the oracle: the comparison of
test_gpu_k2_dispatch._ticks (compare_plans plus a winner-only run).

The winner is candidate 1 (candidate 0 is stuck, as at the bench's shape:
the host walks two words), with 1, 64, 65 and 256 pods -- one lane, a full
group, one pod into the second group, all four groups -- on a 600-node pool
(10-word rows) whose first 512 nodes mostly refuse its pods, so the mapping
mixes head nodes and nodes beyond the head.  The same through the general
kernel's node-order path (SR_K2_NODE_KERNEL=0), through its pod-order path
(300 pods: more than node order takes; SR_K2_MODE=1), and with the switch off."""
import ctypes
import zlib

import numpy as np
import pytest

from helpers import Scenario
from oracle_lib import OracleSnapshot, oracle_plan
from spotplanner import capi
from spotplanner.model import Container, Node, Pod
from spotplanner.rescheduler import plan_arrays
from test_gpu_k2_dispatch import make_checker
from test_gpu_parity import compare_plans
from test_gpu_ticks import _with_extra

pytestmark = pytest.mark.gpu

N_NODES, HEAD, N_TICKS, BURST_TICK = 600, 512, 8, 5


def winner_scenario(n_win):
    """Candidate 0 stuck at its third pod, candidate 1 the winner with n_win
    pods, then four small drainable candidates (their waves finish before the
    winner's and are first drainable so far for a while)."""
    nodes = []
    for i in range(N_NODES):
        if i < HEAD:
            cpu = 320 if i % 50 == 7 else 90  # ten head nodes take two or three of the winner's pods
        else:
            cpu = 400 + 50 * (i % 7)
        nodes.append(Node("n%d" % i, cpu))
    stuck = [Pod("s%d" % k, containers=[Container(10 if k != 2 else 10 ** 6)]) for k in range(5)]
    win = [Pod("w%d" % k, containers=[Container(100 + 10 * (k % 6))]) for k in range(n_win)]
    rest = [[Pod("r%d_%d" % (c, k), containers=[Container(20 + 5 * k)]) for k in range(3 + c)] for c in range(4)]
    cands = [stuck, win] + rest
    flat = [p for c in cands for p in c]
    filler = Pod("filler", containers=[Container(60)])  # on a node the winner uses, it moves the pods behind it
    # pod stamps: without them the encoder never reuses the candidate side (no K0-less tick); distinct per winner
    # size, as no other input of the process may share them
    stamps = [(1 << 63) | (zlib.crc32(b"winner-map-%d" % n_win) << 24) | (i + 1) for i in range(len(flat) + 1)]
    sc = Scenario(nodes, [[] for _ in nodes], flat + [filler], stamps=stamps)
    cand_off = np.cumsum([0] + [len(c) for c in cands]).astype(np.int32)
    cand_pods = np.arange(sc.q0, sc.q0 + len(flat), dtype=np.int32)
    return sc, cand_off, cand_pods, sc.q0 + len(flat)


def tick_inputs(sc, filler, n_ticks, seed):
    """Per tick the spot nodes' pod lists: one to three filler pods more than
    the tick before, every other one on a node with room for the winner's pods;
    tick BURST_TICK gets 20 more on distinct nodes."""
    rng = np.random.default_rng(seed)
    roomy = [i for i in range(N_NODES) if i >= HEAD or i % 50 == 7]
    extra, out = [], []
    for tick in range(n_ticks):
        if tick:
            for _ in range(int(rng.integers(1, 4))):
                pos = int(rng.choice(roomy)) if len(extra) % 2 == 0 else int(rng.integers(N_NODES))
                extra.append((filler, pos))
        if tick == BURST_TICK:  # more changed nodes than a K0-less run carries (16): this tick launches K0
            extra.extend((filler, int(i)) for i in rng.choice(N_NODES, 20, replace=False))
        out.append(_with_extra(sc, N_NODES, extra))
    return out


CASES = {
    "np1": (1, {}), "np64": (64, {}), "np65": (65, {}), "np256": (256, {}),
    "np65_general_kernel": (65, dict(SR_K2_NODE_KERNEL=0)),
    "np300_pod_order": (300, {}),                 # beyond node order: the general kernel's pod-order path (LDS mapping)
    "np65_pod_order_mode": (65, dict(SR_K2_MODE=1)),
    "np65_switch_off": (65, dict(SR_K2_MAP_REGS=0)),  # the fence and the read-back of out_node
    "np256_switch_off": (256, dict(SR_K2_MAP_REGS=0)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_winner_mapping(case):
    n_win, env = CASES[case]
    sc, cand_off, cand_pods, filler = winner_scenario(n_win)
    lib = capi.load_planner()
    ck = make_checker(**env)
    k0_less = k0_runs = 0
    try:
        for tick, (off, idx) in enumerate(tick_inputs(sc, filler, N_TICKS, n_win)):
            o = oracle_plan(OracleSnapshot(sc.ptr, sc.spot, off, idx), sc.ptr, cand_off, cand_pods, mode=1)
            h = ctypes.c_void_p()
            assert lib.sr_snapshot_create(sc.ptr, capi.ptr(sc.spot, capi.P32), len(sc.spot), capi.ptr(off, capi.P32),
                                          capi.ptr(idx, capi.P32), ctypes.byref(h)) == capi.SR_OK
            try:
                q = plan_arrays(ck, h, sc.ptr, cand_off, cand_pods, full=False)  # winner only: returns at the winner
                tq = ck.timing()
                p = plan_arrays(ck, h, sc.ptr, cand_off, cand_pods)
            finally:
                lib.sr_snapshot_destroy(h)
            k0_less += tq.k0_columns == -2
            k0_runs += tq.k0_columns != -2
            compare_plans(o, p, cand_off)
            assert np.array_equal(p.status, o["status"]), tick
            assert (q.first_ok, q.first_fallback, q.winner) == (p.first_ok, p.first_fallback, p.winner), tick
            assert (q.first_ok, q.winner) == (o["first_ok"], o["winner"]) == (1, 1), tick
            want = o["node_of_pod"][cand_off[1]:cand_off[2]]
            assert len(q.winner_map) == n_win and np.array_equal(q.winner_map, want), tick
            assert np.array_equal(p.winner_map, want), tick
            # the mapping is not trivial: head nodes and nodes beyond the head
            if n_win >= 64:
                assert np.any(want < HEAD) and np.any(want >= HEAD), tick
        if "pod_order" in case:  # K2 corrects changed nodes on node-order launches only: every tick launches K0
            assert (k0_less, k0_runs) == (0, N_TICKS), (k0_less, k0_runs)
        else:
            assert k0_less >= 2 and k0_runs >= 2, (k0_less, k0_runs)
    finally:
        ck.close()
