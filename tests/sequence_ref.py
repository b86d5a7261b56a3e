"""The reference pass of sr_plan_sequence on the CPU oracle, and the inputs the
sequence tests share.

The pass is the loop of rescheduler.go:228-287 with the `break` at :286
replaced by "keep the forked state and go on", up to a budget: Fork,
canDrainNode, Revert for every candidate in order; a drainable candidate's pods
are then added to the snapshot at their planned nodes (what the Go snapshot
holds after canDrainNode returns nil) and the pass goes on from that state.
"""
from __future__ import annotations

import ctypes
import zlib
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional

import numpy as np

from helpers import Scenario
from oracle_lib import OracleSnapshot, load_oracle, oracle_plan
from randcluster import rand_scenario
from scenario_gen import init_and_gpu_scenario, rand_spread_replicas, rand_spread_scenario, rand_volume_scenario
from spotplanner import capi
from spotplanner.model import Container, Node, PersistentVolume, PersistentVolumeClaim, Pod, Volume, VolumeWorld
from spotplanner.synth import AFFINITY, REALISTIC, SynthCluster, build_candidates, new_node_map

OK, FB, EMPTY, SKIPPED = capi.SR_CAND_OK, capi.SR_CAND_FALLBACK, capi.SR_CAND_EMPTY, capi.SR_CAND_SKIPPED


@dataclass
class RefSequence:
    drained: np.ndarray
    stop: int
    stop_cand: int
    status: np.ndarray
    node_of_pod: np.ndarray


def reference_sequence(osnap: OracleSnapshot, cluster_ptr, cand_off, cand_pods, max_drains: Optional[int] = None,
                       first_cand: int = 0) -> RefSequence:
    """The pass on `osnap`, which keeps every drained candidate's pods."""
    lib = load_oracle()
    cand_off = np.ascontiguousarray(cand_off, np.int32)
    cand_pods = np.ascontiguousarray(cand_pods, np.int32)
    n = len(cand_off) - 1
    base = int(cand_off[0]) if n > 0 else 0
    status = np.full(n, SKIPPED, np.int32)
    node = np.full(int(cand_off[-1]) - base if n > 0 else 0, -1, np.int32)
    drained, stop, stop_cand = [], capi.SR_SEQ_END, -1
    for c in range(first_cand, n):
        b, e = int(cand_off[c]), int(cand_off[c + 1])
        if e == b:
            status[c] = EMPTY
            continue
        pods = np.ascontiguousarray(cand_pods[b:e])
        omap = np.full(e - b, -1, np.int32)
        assert lib.oracle_snapshot_fork(osnap.h) == 0
        r = lib.oracle_can_drain_node(osnap.h, cluster_ptr, capi.ptr(pods, capi.P32), e - b, capi.ptr(omap, capi.P32))
        assert lib.oracle_snapshot_revert(osnap.h) == 0
        if r == -2:
            status[c] = FB
            stop, stop_cand = capi.SR_SEQ_FALLBACK, c
            break
        node[b - base:e - base] = omap
        if r >= 0:
            status[c] = r
            continue
        status[c] = OK
        for k in range(e - b):
            lib.oracle_snapshot_add_pod(osnap.h, cluster_ptr, int(pods[k]), int(omap[k]))
        drained.append(c)
        if max_drains is not None and len(drained) == max_drains:
            stop = capi.SR_SEQ_BUDGET
            break
    return RefSequence(np.array(drained, np.int32), stop, stop_cand, status, node)


@dataclass
class SeqInput:
    """One cluster: what both snapshots are built from and the candidate list."""
    ptr: object
    spot: np.ndarray
    node_pod_off: np.ndarray
    node_pod_idx: np.ndarray
    cand_off: np.ndarray
    cand_pods: np.ndarray
    keep: object = None  # the encoding's owner
    _ref: Dict = field(default_factory=dict)

    def oracle_snapshot(self) -> OracleSnapshot:
        return OracleSnapshot(self.ptr, self.spot, self.node_pod_off, self.node_pod_idx)

    def product_snapshot(self):
        h = ctypes.c_void_p()
        st = capi.load_planner().sr_snapshot_create(self.ptr, capi.ptr(self.spot, capi.P32), len(self.spot),
                                                    capi.ptr(self.node_pod_off, capi.P32),
                                                    capi.ptr(self.node_pod_idx, capi.P32), ctypes.byref(h))
        assert st == capi.SR_OK
        return h

    def base_plan(self):
        """Every candidate from the base snapshot (computed once)."""
        if "base" not in self._ref:
            self._ref["base"] = oracle_plan(self.oracle_snapshot(), self.ptr, self.cand_off, self.cand_pods, mode=1,
                                            threads=8)
        return self._ref["base"]

    def reference(self, max_drains=None, first_cand=0, after=None):
        """The reference pass from the base snapshot (computed once per argument set, never changed); `after`: a
        pass (max_drains, first_cand) run on the same snapshot before it.  Returns (RefSequence, node states)."""
        key = (max_drains, first_cand, after)
        if key not in self._ref:
            osnap = self.oracle_snapshot()
            if after is not None:
                reference_sequence(osnap, self.ptr, self.cand_off, self.cand_pods, *after)
            r = reference_sequence(osnap, self.ptr, self.cand_off, self.cand_pods, max_drains, first_cand)
            self._ref[key] = (r, [osnap.node_state(i) for i in range(len(self.spot))])
            osnap.close()
        return self._ref[key]


def from_scenario(nodes, spot_pods, cands, volumes=None, stamped: Optional[str] = None) -> SeqInput:
    """`stamped`: the input's name; its pods then carry pod stamps (sr_cluster.pod_stamp), without which the
    encoder never reuses the candidate side between rounds.  A stamp names one pod object for the process's
    lifetime and every input has a string dictionary of its own, hence stamps no other input shares."""
    flat = [p for c in cands for p in c]
    stamps = None
    if stamped is not None:
        n = sum(len(ps) for ps in spot_pods) + len(flat)
        stamps = [(1 << 63) | (zlib.crc32(stamped.encode()) << 24) | (i + 1) for i in range(n)]
    sc = Scenario(nodes, spot_pods, flat, volumes=volumes, stamps=stamps)
    cand_off = np.cumsum([0] + [len(c) for c in cands]).astype(np.int32)
    cand_pods = np.arange(sc.q0, sc.q0 + len(flat), dtype=np.int32)
    return SeqInput(sc.ptr, sc.spot, sc.node_pod_off, sc.node_pod_idx, cand_off, cand_pods, keep=sc)


def from_synth(sc: SynthCluster) -> SeqInput:
    lib = capi.load_planner()
    nm = new_node_map(lib.sr_new_node_map, sc.ptr, sc.n_nodes, sc.n_pods, sc.od_label, sc.spot_label)
    cand_off, cand_pods = build_candidates(nm, sc.pod_flags())
    return SeqInput(sc.ptr, nm.spot, nm.node_pod_off, nm.node_pod_idx, np.ascontiguousarray(cand_off, np.int32),
                    np.ascontiguousarray(cand_pods, np.int32), keep=(sc, nm))


SMALL = dict(n_spot=6, n_cand=12, max_pods=6)

BUILDERS: Dict[str, Callable[[], SeqInput]] = {}
for _s in (1, 2, 3, 4, 5, 11, 12, 14):
    BUILDERS["plain-%d" % _s] = lambda s=_s: from_scenario(*rand_scenario(s, features=False, **SMALL))
for _s in (1, 11, 14, 30, 33):
    BUILDERS["features-%d" % _s] = lambda s=_s: from_scenario(*rand_scenario(s))
BUILDERS["anti-30"] = lambda: from_scenario(*rand_scenario(30, anti=0.3))
for _s in (11, 33):
    BUILDERS["interpod-%d" % _s] = lambda s=_s: from_scenario(*rand_scenario(s, anti=0.3, aff=0.2, shared_keys=True,
                                                                              valid_selectors=True))
BUILDERS["c5"] = lambda: from_synth(SynthCluster(5, seed=5, n_on_demand=100, n_spot=200))
BUILDERS["c3-affinity"] = lambda: from_synth(SynthCluster(3, seed=41, n_on_demand=300, n_spot=80, **AFFINITY))
BUILDERS["c3-tight"] = lambda: from_synth(SynthCluster(3, seed=41, n_on_demand=300, n_spot=40))
FALLBACK_STOPS = {0: 5, 13: 6, 25: 6, 31: 10}  # seed -> the candidate the pass stops at, after two drains
for _s in FALLBACK_STOPS:
    BUILDERS["fallback-%d" % _s] = lambda s=_s: from_scenario(*rand_scenario(s, fallback=True, **SMALL))

# Volume, spread and extension-record state that moves between rounds.  The facts test_sequence_reference.py
# asserts: name -> (drains, stop, stop candidate, divergence()).  A FALLBACK stop is "static" when the candidate is
# FALLBACK from the base snapshot too, "dynamic" (DYNAMIC_STOPS) when only the snapshot the earlier drains leave
# makes it one.
END, FALLBACK = capi.SR_SEQ_END, capi.SR_SEQ_FALLBACK
RECORDED = {
    "vol-5": (5, END, -1, (2, 3, 2, 8)),
    "vol-11": (7, END, -1, (0, 5, 0, 7)),
    "vol-22": (4, END, -1, (4, 3, 2, 9)),
    "vol-26": (7, END, -1, (1, 5, 0, 6)),
    "vol-17": (6, FALLBACK, 7, (1, 3, 0, 4)),
    "vol-10": (3, FALLBACK, 8, (1, 2, 0, 5)),
    "spread-8": (6, END, -1, (6, 5, 0, 11)),
    "spread-10": (6, END, -1, (4, 5, 1, 10)),
    "spread-22": (9, END, -1, (1, 6, 0, 7)),
    "spread-0": (5, FALLBACK, 10, (1, 1, 0, 3)),
    "spread-2": (5, FALLBACK, 5, (0, 3, 0, 3)),
    "replicas-0": (3, END, -1, (0, 2, 0, 2)),
    "initgpu-1": (3, END, -1, (1, 1, 0, 2)),
    "realistic-40": (22, END, -1, (0, 16, 0, 231)),
    "realistic-80": (24, END, -1, (0, 18, 1, 231)),
    "realistic-120": (28, END, -1, (1, 25, 6, 230)),
}
for _n in RECORDED:
    _kind, _s = _n.split("-")
    _s = int(_s)
    if _kind == "vol":
        BUILDERS[_n] = lambda s=_s, n=_n: from_scenario(*rand_volume_scenario(s), stamped=n)
    elif _kind == "spread":
        BUILDERS[_n] = lambda s=_s, n=_n: from_scenario(*rand_spread_scenario(s), stamped=n)
    elif _kind == "replicas":
        BUILDERS[_n] = lambda s=_s, n=_n: from_scenario(*rand_spread_replicas(s), stamped=n)
    elif _kind == "initgpu":
        BUILDERS[_n] = lambda s=_s, n=_n: from_scenario(*init_and_gpu_scenario(s), stamped=n)
    else:
        BUILDERS[_n] = lambda s=_s: from_synth(SynthCluster(3, seed=41, n_on_demand=300, n_spot=s, **REALISTIC))


def volflip(which: str) -> SeqInput:
    """Candidates 3 and 5 bring the same attachable volume V: from the base snapshot no spot node holds it and
    all seven candidates are planned; once candidate 3 has drained (round 4, the encoder reusing the candidate
    side since round 3), a spot node holds V and candidate 5 belongs to the reference path."""
    nodes = [Node("s%d" % i, cpu_milli=4000) for i in range(4)]
    world = VolumeWorld()
    if which == "ebs":
        world = VolumeWorld(pvcs=[PersistentVolumeClaim("q", volume_name="pv-q")],
                            pvs=[PersistentVolume("pv-q", kind="aws-ebs", volume_id="vol-1")])

    def vol():
        if which == "ebs":
            return Volume(name="q", claim="q")
        return Volume(name="pd", gce_pd="pd7", read_only=which == "gce_ro")

    def pod(name, *vols, cpu=100):
        return Pod(name, containers=[Container(cpu_milli=cpu)], volumes=list(vols))

    cands = [[pod("p0")], [pod("p1", cpu=3900)], [pod("p2")], [pod("v3", vol())], [pod("p4")],
             [pod("v5", vol()), pod("q5")], [pod("p6")]]
    return from_scenario(nodes, [[] for _ in nodes], cands, volumes=world, stamped="volflip-" + which)


VOLFLIP = ["volflip-gce_ro", "volflip-gce_rw", "volflip-ebs"]
for _n in VOLFLIP:
    BUILDERS[_n] = lambda w=_n.split("-")[1]: volflip(w)
    RECORDED[_n] = (5, FALLBACK, 5, None)  # the divergence is not part of these inputs' contract
DYNAMIC_STOPS = ["spread-2"] + VOLFLIP
# The round whose prepare is the first to classify the stop candidate FALLBACK (round k + 1 sees k drains).  The
# encoder saves an input on its first encode, builds the reuse index on the second and reuses from the third:
# a planner that starts cold can have reused a round before the flip only when this is 4 or more.
FLIP_ROUND = {"spread-2": 2, "volflip-gce_ro": 5, "volflip-gce_rw": 5, "volflip-ebs": 5}

_inputs: Dict[str, SeqInput] = {}


def get_input(name: str) -> SeqInput:
    """The named input, built once per process."""
    if name not in _inputs:
        _inputs[name] = BUILDERS[name]()
    return _inputs[name]


def divergence(inp: SeqInput, ref: RefSequence):
    """How the pass differs from the base plan: (candidates drainable from the
    base snapshot that fail in the pass, drained candidates whose mapping
    changed, candidates failing at another pod, judged candidates that differ
    in status or mapping)."""
    base = inp.base_plan()
    off = inp.cand_off - inp.cand_off[0]
    fail_now = maps = fail_idx = differ = 0
    for c in range(len(inp.cand_off) - 1):
        s, b = int(ref.status[c]), int(base["status"][c])
        if s in (SKIPPED, FB, EMPTY):
            continue
        same_map = np.array_equal(ref.node_of_pod[off[c]:off[c + 1]], base["node_of_pod"][off[c]:off[c + 1]])
        fail_now += b == OK and s >= 0
        maps += s == OK and not same_map
        fail_idx += s >= 0 and b >= 0 and s != b
        differ += s != b or not same_map
    return fail_now, maps, fail_idx, differ
