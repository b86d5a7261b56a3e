"""K2's changed-node table and wave header on K0-less ticks.

A K0-less tick's K2 corrects the tables for the spot nodes changed since they
were written: every wave holds the changed nodes (position, free values,
record) in its registers, one table entry per lane, and takes the F-head
bits, the far words, the pointer moves and the window records of those nodes
from there; its other operands come from the wave's header.  These cases make
the changed nodes decide the plan, tick after tick, and compare every tick --
planned winner-only and in full -- with the oracle exactly: every status,
every pod's node, first_ok / first_fallback / winner and the winner-only
mapping.

The pool: tight nodes (no pod of the main candidate fits), `BIG` nodes that
take one big pod each, backup nodes that take one small pod each, and window 2
(nodes 128..191) without any room, which no candidate ever visits; only the
pool's last two nodes take a huge pod.  The main candidate (candidate 1;
candidate 0 is stuck) is two zero-request pods, eight big pods, two host-port
pods, a pod with an ephemeral request, small pods and two huge pods, so first
fit walks the BIG nodes in order, then the backups, then the last nodes.  Node
0 takes three pods: with a filler on it the patch's pod count lets the two
zero-request pods in and refuses the next pod for the pod limit alone.  A BIG
node with a cpu filler still has room for a host-port pod, which sets its port
bit on the changed node's record.  The script adds
filler pods tick by tick (cpu and ephemeral fillers: a bit turns
off) on spot positions 0, 5 (two in one word),
63 | 64 (a window boundary), 511 | 512 (the last head node, the first far
node), the pool's last node, a node of the unvisited window and nodes in
between: 1, 2, 15 and 16 changed nodes since the tables were written run
K0-less, the 17th -- a cpu filler like the others, one more node than the
table's 16 entries -- launches K0; the last two ticks take fillers away again
(a bit turns on).  Every tick's plan must differ from the tick before.

A host-port filler cannot ride a K0-less tick of a candidate with host-port
pods: a node's base UsedPorts are static conflicts in the atom rows (its
record's port word starts at zero), so the tick that adds one rewrites the
tables whatever the number of changed nodes (the one-pod case has no host-port
pod and no such row: there the tick is K0-less, which the case asserts).  It has a tick of its own after the 17-node tick, and the K0-less ticks
after it plan on that state.  The patch's port word is therefore always zero.

The 6,000-node cases also plan their first tick with SR_S_HEAD_ONLY=0: K0
writes fewer bytes in the case's own planner, so its S rows are head-only."""
import ctypes
import zlib

import numpy as np
import pytest

from helpers import Scenario
from oracle_lib import OracleSnapshot, oracle_plan
from spotplanner import capi
from spotplanner.model import Container, ContainerPort, Node, Pod
from spotplanner.rescheduler import plan_arrays
from test_gpu_k2_dispatch import make_checker
from test_gpu_parity import compare_plans
from test_gpu_ticks import _with_extra

pytestmark = pytest.mark.gpu

HEAD = 512
N_BIG = 8
BIGS = [0, 5, 63, 64, 70, 71, 300, 511, 512, 520] + list(range(521, 529))  # (522..528: spares no filler lands on)
UNVISITED = 150  # window 2: no room at all
GiB = 1 << 30


def pool_nodes(n_nodes):
    nodes = []
    for i in range(n_nodes):
        if i >= n_nodes - 2:
            cpu = 400  # the two nodes that take a huge pod (350); with a cpu filler none
        elif i in BIGS:
            cpu = 170  # one big pod (150); with a cpu filler (60) none
        elif i >= 72 and not 128 <= i < 192 and i % 3 != 0 and (i < 600 or i >= n_nodes - 400):
            cpu = 140  # a backup: one small pod (100); with a cpu filler none
        else:
            cpu = 90
        nodes.append(Node("n%d" % i, cpu, pods=3 if i == 0 else 100, ephemeral=100 * GiB))
    return nodes


def main_pods(n_win, init):
    """The main candidate's pods.  `init`: the big pods ask for their 150 through an init container (the fit
    request; AddPod accounts the 100 of the container): extension records."""
    def big(k):
        if init:
            return Pod("b%d" % k, containers=[Container(100)], init_containers=[Container(150)])
        return Pod("b%d" % k, containers=[Container(150)])
    if n_win == 1:
        return [big(0)]
    pods = [Pod("zero%d" % k, containers=[Container(0)]) for k in range(2)] + [big(k) for k in range(N_BIG)]
    pods += [Pod("port%d" % k, containers=[Container(100, ports=[ContainerPort(8080)])]) for k in range(2)]
    pods.append(Pod("eph", containers=[Container(100, ephemeral=60 * GiB)]))
    pods += [Pod("s%d" % k, containers=[Container(100)]) for k in range(n_win - len(pods) - 2)]
    # the last pods: with a filler on the pool's last node the second one finds its only node taken, and the
    # candidate is stuck there (its row is not empty: no pod enters the empty class, the tick stays K0-less)
    return pods + [Pod("huge%d" % k, containers=[Container(350)]) for k in range(2)]


def scenario(n_nodes, n_win, init, tag):
    nodes = pool_nodes(n_nodes)
    stuck = [Pod("x%d" % k, containers=[Container(10 if k != 2 else 10 ** 6)]) for k in range(5)]
    rest = [[Pod("r%d_%d" % (c, k), containers=[Container(20 + 5 * k)]) for k in range(3 + c)] for c in range(4)]
    cands = [stuck, main_pods(n_win, init)] + rest
    flat = [p for c in cands for p in c]
    fillers = [Pod("f_cpu", containers=[Container(60)]),
               Pod("f_eph", containers=[Container(1, ephemeral=50 * GiB)]),
               Pod("f_port", containers=[Container(1, ports=[ContainerPort(8080)])])]
    # pod stamps: without them the encoder never reuses the candidate side (no K0-less tick); distinct per case
    stamps = [(1 << 63) | (zlib.crc32(tag.encode()) << 24) | (i + 1) for i in range(len(flat) + len(fillers))]
    sc = Scenario(nodes, [[] for _ in nodes], flat + fillers, stamps=stamps)
    cand_off = np.cumsum([0] + [len(c) for c in cands]).astype(np.int32)
    cand_pods = np.arange(sc.q0, sc.q0 + len(flat), dtype=np.int32)
    f0 = sc.q0 + len(flat)
    return sc, cand_off, cand_pods, dict(cpu=f0, eph=f0 + 1, port=f0 + 2)


def script(n_nodes, ports):
    """Per tick the fillers (kind, spot position) present, and the nodes changed since the tables were
    written (None: the tick launches K0).  `ports`: some candidate pod has a host port, so the port filler
    changes an atom row and its tick launches K0; without one no row knows the port and the tick is K0-less."""
    last = n_nodes - 1
    t2 = [("cpu", 0)]
    t3 = t2 + [("cpu", 5)]
    # 13 more nodes (73, 74, 76 are the first backups)
    t4 = t3 + [("cpu", 63), ("cpu", 64), ("cpu", 511), ("cpu", 512), ("cpu", last), ("cpu", UNVISITED), ("cpu", 70),
               ("eph", 74), ("cpu", 76), ("cpu", 77), ("cpu", 79), ("cpu", 300), ("cpu", 80)]
    t5 = t4 + [("cpu", 71)]
    t6 = t5 + [("cpu", 520)]  # the 17th changed node, a cpu filler like the others: one more than the table holds
    t7 = t6 + [("port", 73), ("cpu", 521)]  # the port filler on a tick of its own: K0 again, for the atoms (above)
    t8 = [f for f in t7 if f[1] not in (5, 63, 64)]
    t9 = [f for f in t8 if f[1] not in (0, 511, 512, last)]
    after = (None, 3, 7) if ports else (2, 5, 9)
    return [([], None), ([], None), (t2, 1), (t3, 2), (t4, 15), (t5, 16), (t6, None), (t7, after[0]), (t8, after[1]),
            (t9, after[2])]


CASES = {
    # candidates of 1, 64, 65 and 256 pods on the node-order kernel (one lane, one group, two groups, four)
    "np1": (600, 1, False, {}),
    "np64": (600, 64, False, {}),
    "np65": (600, 65, False, {}),
    "np256": (600, 256, False, {}),
    # the general kernel's node-order path
    "np65_general_kernel": (600, 65, False, dict(SR_K2_NODE_KERNEL=0)),
    # an init container: the launch takes the instance with extension records
    "np65_init_container": (600, 65, True, {}),
    # cooperative blocks (as test_gpu_k2_dispatch.test_cooperative_blocks sets them up)
    "np65_coop": (600, 65, False, dict(SR_LIST_COST_MIN=0, SR_K2_WPB=4, SR_K2_COOP=4096)),
    # 94-word rows, head-only S rows: the class programs and the helpers' scans read the table
    "np65_wide": (6000, 65, False, {}),
    "np65_wide_coop": (6000, 65, False, dict(SR_LIST_COST_MIN=0, SR_K2_WPB=4, SR_K2_COOP=4096)),
}


def run_ticks(ck, sc, cand_off, cand_pods, inputs, n_nodes, winner_runs=1):
    """Every tick winner-only (`winner_runs` times) and in full against the oracle; returns per tick
    (oracle plan, timing of the full run)."""
    lib = capi.load_planner()
    out = []
    for tick, (off, idx) in enumerate(inputs):
        o = oracle_plan(OracleSnapshot(sc.ptr, sc.spot, off, idx), sc.ptr, cand_off, cand_pods, mode=1)
        h = ctypes.c_void_p()
        assert lib.sr_snapshot_create(sc.ptr, capi.ptr(sc.spot, capi.P32), len(sc.spot), capi.ptr(off, capi.P32),
                                      capi.ptr(idx, capi.P32), ctypes.byref(h)) == capi.SR_OK
        try:
            qs = [plan_arrays(ck, h, sc.ptr, cand_off, cand_pods, full=False) for _ in range(winner_runs)]
            tq = ck.timing()
            p = plan_arrays(ck, h, sc.ptr, cand_off, cand_pods)
            t = ck.timing()
        finally:
            lib.sr_snapshot_destroy(h)
        print("tick %d: k0_columns %d / %d, k0_dirty_nodes %d, enc_reused %d, k2_coop %d, first_ok %d" % (
            tick, tq.k0_columns, t.k0_columns, t.k0_dirty_nodes, t.enc_reused, t.k2_coop, o["first_ok"]))
        compare_plans(o, p, cand_off)
        assert np.array_equal(p.status, o["status"]), tick
        assert np.array_equal(p.node_of_pod, o["node_of_pod"]), tick
        assert (p.first_ok, p.first_fallback, p.winner) == (o["first_ok"], o["first_fallback"], o["winner"]), tick
        want = o["node_of_pod"][cand_off[o["first_ok"]]:cand_off[o["first_ok"] + 1]] if o["first_ok"] >= 0 else None
        for q in qs:
            assert (q.first_ok, q.first_fallback, q.winner) == (o["first_ok"], o["first_fallback"], o["winner"]), tick
            if want is not None:
                assert np.array_equal(q.winner_map, want), tick
        if want is not None:
            assert np.array_equal(p.winner_map, want), tick
        out.append((o, tq, t))
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_changed_nodes_decide_the_plan(case):
    n_nodes, n_win, init, env = CASES[case]
    sc, cand_off, cand_pods, filler = scenario(n_nodes, n_win, init, "changed-nodes-" + case)
    ticks = script(n_nodes, ports=n_win > 1)
    inputs = [_with_extra(sc, n_nodes, [(filler[k], pos) for k, pos in fl]) for fl, _ in ticks]
    ck = make_checker(**env)
    try:
        res = run_ticks(ck, sc, cand_off, cand_pods, inputs, n_nodes)
    finally:
        ck.close()
    main = slice(int(cand_off[1]), int(cand_off[2]))
    for tick, ((fl, changed), (o, tq, t)) in enumerate(zip(ticks, res)):
        if tick >= 2:  # the changed nodes decide: some pod of the main candidate moves
            prev = res[tick - 1][0]
            assert not np.array_equal(o["node_of_pod"][main], prev["node_of_pod"][main]), tick
        if tick < 2:
            continue
        if changed is None:  # the 17th changed node, then the port filler: K0 runs
            assert tq.k0_columns >= 0, (tick, tq.k0_columns)
            if tick == 6:  # exactly 17 nodes, none of them for its ports
                assert len({pos for _, pos in fl}) == 17 and {k for k, _ in fl} <= {"cpu", "eph"}, fl
        else:  # K0-less, winner-only and in full, with exactly the script's changed nodes
            assert (tq.k0_columns, t.k0_columns, t.k0_dirty_nodes) == (-2, -2, changed), (
                tick, tq.k0_columns, t.k0_columns, t.k0_dirty_nodes)
        if "coop" in case:
            assert t.k2_coop > 0, (tick, t.k2_coop)
    if n_nodes > 64 * 64:  # rows wider than 64 words: K0 wrote only the heads of the S rows, fewer bytes than full rows
        full = make_checker(SR_S_HEAD_ONLY=0, **env)
        try:
            r0 = run_ticks(full, sc, cand_off, cand_pods, inputs[:1], n_nodes)
        finally:
            full.close()
        assert res[0][2].k0_columns == r0[0][2].k0_columns == -1, (res[0][2].k0_columns, r0[0][2].k0_columns)
        assert 0 < res[0][2].bytes_tables < r0[0][2].bytes_tables, (res[0][2].bytes_tables, r0[0][2].bytes_tables)
    if n_win >= 64:  # the main candidate's plan uses head nodes and nodes beyond the head
        m = res[0][0]["node_of_pod"][main]
        assert np.any((m >= 0) & (m < HEAD)) and np.any(m >= HEAD)


def test_finish_many_small_drainable_candidates():
    """k2_finish: a stuck candidate 0, then 200 small drainable candidates whose waves finish in any order.
    Every drainable wave enters the first-drainable minimum and stores through the header's pointers; the
    winner must be candidate 1 with the oracle's mapping in each of 20 consecutive winner-only runs and in the full run of
    every tick (a cpu filler more on node 0 or 1 per tick: the winner's pods move)."""
    n_nodes = 600
    nodes = [Node("n%d" % i, 170 if i < 3 else 90) for i in range(n_nodes)]
    stuck = [Pod("x%d" % k, containers=[Container(10 if k != 1 else 10 ** 6)]) for k in range(3)]
    small = [[Pod("c%d_%d" % (c, k), containers=[Container(80)]) for k in range(2)] for c in range(200)]
    cands = [stuck] + small
    flat = [p for c in cands for p in c]
    fill = Pod("f_cpu", containers=[Container(60)])
    stamps = [(1 << 63) | (zlib.crc32(b"changed-nodes-finish") << 24) | (i + 1) for i in range(len(flat) + 1)]
    sc = Scenario(nodes, [[] for _ in nodes], flat + [fill], stamps=stamps)
    cand_off = np.cumsum([0] + [len(c) for c in cands]).astype(np.int32)
    cand_pods = np.arange(sc.q0, sc.q0 + len(flat), dtype=np.int32)
    f = sc.q0 + len(flat)
    ticks = [[], [], [(f, 0)], [(f, 0), (f, 0)], [(f, 0), (f, 0), (f, 1)], []]
    inputs = [_with_extra(sc, n_nodes, fl) for fl in ticks]
    ck = make_checker()
    try:
        res = run_ticks(ck, sc, cand_off, cand_pods, inputs, n_nodes, winner_runs=20)
    finally:
        ck.close()
    for tick, (o, tq, t) in enumerate(res):
        assert (o["first_ok"], o["winner"]) == (1, 1), tick
        if tick >= 2:
            assert (tq.k0_columns, t.k0_columns) == (-2, -2), (tick, tq.k0_columns, t.k0_columns)
            prev = res[tick - 1][0]
            assert not np.array_equal(o["node_of_pod"][3:5], prev["node_of_pod"][3:5]), tick
