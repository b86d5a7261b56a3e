"""Mirror of the reference's planning functions (rescheduler.go, package main).

findSpotNodeForPod (rescheduler.go:338-353), canDrainNode (:357-370),
validateArgs (:407-417), podID (:402-404), and plan_arrays: the planning
segment of run() (:228-287) evaluated for every candidate at once on the GPU.
plan_sequence_arrays / drainSequence go beyond the reference, which drains one
node per tick: several consistent drains planned in one tick (sr_plan_sequence).
explainPods / explainCandidate batch the per-node log line of :348: which filter
groups refuse a pod on each spot node (sr_explain_pods); explainPlan does it for
every stuck candidate of a plan at once, each stop pod judged after the
candidate's own earlier pods (sr_explain_plan).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import capi
from .model import EncodedDrain, NilControllerPanic, Node, Pod, PodDisruptionBudget, encode_cluster, pod_id
from .planner import ClusterSnapshot, FallbackRequired, PlannerError, PredicateChecker
from .synth import pods_for_deletion

podID = pod_id


class GoError(Exception):
    """A Go `error` value: str(err) is its Error() text."""


def validateArgs(OnDemandNodeLabel: str, SpotNodeLabel: str) -> Optional[GoError]:
    """rescheduler.go:407-417."""
    if len(OnDemandNodeLabel.split("=")) > 2:
        return GoError("the on demand node label is not correctly formatted: expected '<label_name>' or "
                       "'<label_name>=<label_value>', but got %s" % OnDemandNodeLabel)
    if len(SpotNodeLabel.split("=")) > 2:
        return GoError("the spot node label is not correctly formatted: expected '<label_name>' or "
                       "'<label_name>=<label_value>', but got %s" % SpotNodeLabel)
    return None


@dataclass
class BlockingPod:
    """drain.BlockingPod: the pod that stops a node from being drained and why (capi.SR_BLOCK_*)."""
    Pod: Pod
    Reason: int


def _block_error(pod: Pod, reason: int) -> GoError:
    """The error texts of drain.GetPodsForDeletionOnNodeDrain [upstream CA @03f60a4c3818]."""
    if reason == capi.SR_BLOCK_NOT_REPLICATED:
        return GoError("%s/%s is not replicated" % (pod.namespace, pod.name))
    if reason == capi.SR_BLOCK_UNMOVABLE_KUBE_SYSTEM:
        return GoError("non-daemonset, non-mirrored, non-pdb-assigned kube-system pod present: %s" % pod.name)
    if reason == capi.SR_BLOCK_LOCAL_STORAGE:
        return GoError("pod with local storage present: %s" % pod.name)
    if reason == capi.SR_BLOCK_NOT_SAFE_TO_EVICT:
        return GoError("pod annotated as not safe to evict present: %s" % pod.name)
    return GoError("error matching pods to pdbs")


def podsForDeletion(podList: Sequence[Pod], pdbs: Sequence[PodDisruptionBudget], deleteNonReplicatedPods: bool = False):
    """The pods run() moves off one on-demand node (rescheduler.go:231-256):
    GetPodsForDeletionOnNodeDrain(nodeInfo.Pods, pdbs, *deleteNonReplicatedPods,
    false, false, nil, 0, now), then the DaemonSet-owner filter.  Returns
    (podsForDeletion, blockingPod, err); evaluated by the planner library
    (sr_pods_for_deletion).  A nil OwnerReference.Controller reached by the
    filter raises NilControllerPanic, as the reference panics."""
    pods = list(podList)
    enc = encode_cluster([Node("node", 0)], pods, pod_node=[0] * len(pods))
    drain = EncodedDrain(pods, list(pdbs))
    lib = capi.load_planner()
    off, idx, bp, br, st = pods_for_deletion(lib.sr_pods_for_deletion, enc.ptr, drain.ptr, np.zeros(1, np.int32),
                                             np.array([0, len(pods)], np.int32), np.arange(len(pods), dtype=np.int32),
                                             deleteNonReplicatedPods)
    if st == capi.SR_ERR_NIL_CONTROLLER:
        raise NilControllerPanic("nil OwnerReference.Controller (rescheduler.go:244)")
    if st != capi.SR_OK:
        raise PlannerError("sr_pods_for_deletion: status %d" % st)
    if bp[0] >= 0:
        blocking = pods[int(bp[0])]
        return [], BlockingPod(blocking, int(br[0])), _block_error(blocking, int(br[0]))
    return [pods[int(i)] for i in idx], None, None


def updateSpotNodeMetrics(spotNodeInfos, pdbs: Sequence[PodDisruptionBudget], deleteNonReplicatedPods: bool = False):
    """updateSpotNodeMetrics (rescheduler.go:388-399): per spot node, the number of
    pods GetPodsForDeletionOnNodeDrain returns (the pods the rescheduler
    understands), {node name: count}; nodes whose call errors are skipped, as the
    reference logs and continues.  The Prometheus gauge itself stays in the Go
    shim (metrics.UpdateNodePodsCount(SpotNodeLabel, name, count))."""
    infos = list(spotNodeInfos)
    pods, pod_node = [], []
    for i, ni in enumerate(infos):
        pods.extend(ni.Pods)
        pod_node.extend([i] * len(ni.Pods))
    enc = encode_cluster([ni.Node for ni in infos], pods, pod_node=pod_node)
    drain = EncodedDrain(pods, list(pdbs))
    off = np.zeros(len(infos) + 1, np.int32)
    off[1:] = np.cumsum([len(ni.Pods) for ni in infos])
    out_off, _, bp, _, st = pods_for_deletion(capi.load_planner().sr_pods_for_deletion, enc.ptr, drain.ptr,
                                              np.arange(len(infos), dtype=np.int32), off,
                                              np.arange(len(pods), dtype=np.int32), deleteNonReplicatedPods,
                                              owner_filter=False)
    if st != capi.SR_OK:
        raise PlannerError("sr_pods_for_deletion: status %d" % st)
    return {ni.Node.name: int(out_off[i + 1] - out_off[i]) for i, ni in enumerate(infos) if bp[i] < 0}


def _node_names(nodes) -> List[str]:
    return [ni.Node.name for ni in nodes]


def _check_order(snapshot: ClusterSnapshot, nodes):
    snapshot.materialize()
    if _node_names(nodes) != snapshot.node_names():
        raise PlannerError("NodeInfoArray order must be the snapshot's node order")


def findSpotNodeForPod(predicateChecker: PredicateChecker, spotSnapshot: ClusterSnapshot, nodes,
                       pod: Pod) -> str:
    """First spot node in NodeInfoArray order whose predicates pass, else ""."""
    if len(nodes) == 0:
        return ""
    pod.node_name = ""  # :341 — pretend the pod is not scheduled
    _check_order(spotSnapshot, nodes)
    enc = spotSnapshot.encode_pods([pod])
    idx = np.zeros(1, np.int32)
    out = np.full(1, -1, np.int32)
    fb = np.zeros(1, np.uint8)
    lib = predicateChecker.lib
    st = lib.sr_find_spot_nodes(predicateChecker.handle, spotSnapshot.handle, enc.ptr, capi.ptr(idx, capi.P32), 1,
                                capi.ptr(out, capi.P32), capi.ptr(fb, capi.PU8))
    if st != capi.SR_OK:
        raise PlannerError("sr_find_spot_nodes: %d %s" % (st, predicateChecker.last_error()))
    if fb[0]:
        raise FallbackRequired(pod_id(pod))
    return nodes[int(out[0])].Node.name if out[0] >= 0 else ""


def canDrainNode(predicateChecker: PredicateChecker, spotSnapshot: ClusterSnapshot, nodes,
                 pods: Sequence[Pod]) -> Optional[GoError]:
    """Places pods one by one (first fit) and adds each to the snapshot; returns
    the reference's error for the first pod that fits nowhere, else None."""
    if len(pods) == 0:
        return None
    _check_order(spotSnapshot, nodes)
    enc = spotSnapshot.encode_pods(list(pods))
    idx = np.arange(len(pods), dtype=np.int32)
    mapping = np.full(len(pods), -1, np.int32)
    fail = ctypes.c_int32(-1)
    fb = ctypes.c_uint8(0)
    lib = predicateChecker.lib
    st = lib.sr_can_drain_node(predicateChecker.handle, spotSnapshot.handle, enc.ptr, capi.ptr(idx, capi.P32),
                               len(pods), capi.ptr(mapping, capi.P32), ctypes.byref(fail), ctypes.byref(fb))
    if st != capi.SR_OK:
        raise PlannerError("sr_can_drain_node: %d %s" % (st, predicateChecker.last_error()))
    if fb.value:
        raise FallbackRequired(", ".join(pod_id(p) for p in pods))
    if len(nodes) > 0:
        # :341 runs for every pod findSpotNodeForPod evaluates: up to and
        # including the first pod that fits nowhere (canDrainNode returns there)
        evaluated = pods if fail.value < 0 else pods[:fail.value + 1]
        for p in evaluated:
            p.node_name = ""
    canDrainNode.last_mapping = [nodes[int(k)].Node.name if k >= 0 else "" for k in mapping]
    if fail.value >= 0:
        return GoError("pod %s can't be rescheduled on any existing spot node" % pod_id(pods[fail.value]))
    return None


canDrainNode.last_mapping = []


@dataclass
class PlanResult:
    winner: int            # index of the candidate run() drains, -1 none / unresolved
    first_ok: int
    first_fallback: int
    status: np.ndarray     # per candidate: SR_CAND_* or failing pod index
    node_of_pod: np.ndarray  # flat, spot position per candidate pod (-1 not placed)
    winner_map: np.ndarray
    checks: int
    fallback_pods: int


def plan_arrays(predicateChecker: PredicateChecker, snapshot_handle, cluster_ptr, cand_off: np.ndarray,
                cand_pods: np.ndarray, cand_global: Optional[np.ndarray] = None, full: bool = True) -> PlanResult:
    """sr_plan over caller-built arrays (the batched drop-in of rescheduler.go:228-287)."""
    lib = predicateChecker.lib
    n = len(cand_off) - 1
    c = capi.sr_candidates(n, capi.ptr(cand_off, capi.P32), capi.ptr(cand_pods, capi.P32),
                           capi.ptr(cand_global, capi.P32) if cand_global is not None else None)
    maxp = int(np.max(np.diff(cand_off))) if n > 0 else 0
    status = np.zeros(max(n, 1), np.int32)
    nodes = np.zeros(max(int(cand_off[-1]) if n > 0 else 0, 1), np.int32)
    wmap = np.full(max(maxp, 1), -1, np.int32)
    o = capi.sr_plan_out()
    o.status = capi.ptr(status, capi.P32) if full else None
    o.node_of_pod = capi.ptr(nodes, capi.P32) if full else None
    o.winner_map = capi.ptr(wmap, capi.P32)
    st = lib.sr_plan(predicateChecker.handle, snapshot_handle, cluster_ptr, ctypes.byref(c), ctypes.byref(o))
    if st != capi.SR_OK:
        raise PlannerError("sr_plan: %d %s" % (st, predicateChecker.last_error()))
    return PlanResult(o.winner, o.first_ok, o.first_fallback, status[:n], nodes[: int(cand_off[-1]) if n else 0],
                      wmap[: o.winner_npods], int(o.checks), int(o.fallback_pods))


@dataclass
class SequenceResult:
    drained: np.ndarray      # candidates to drain, in drain order (ascending)
    stop: int                # capi.SR_SEQ_END / SR_SEQ_BUDGET / SR_SEQ_FALLBACK
    stop_cand: int           # the fallback candidate the pass stopped at, else -1
    status: np.ndarray       # per candidate: SR_CAND_* or failing pod index, as judged in the pass
    node_of_pod: np.ndarray  # flat, spot position per candidate pod (-1 not placed / not judged)
    rounds: int              # device rounds; of which launched K0 / kept the candidate side
    rounds_k0: int
    rounds_reused: int
    remaining: Optional[np.ndarray] = None  # with limits: evictions each group still allows after the pass


@dataclass
class PdbLimits:
    """Disruption groups for sr_plan_sequence_pdb: `allowed[g]` evictions group g still allows (the PDB status'
    allowed disruptions), `pod_group[q]` the group of candidate pod q (parallel to cand_pods; -1: none).  A pod
    selected by several PDBs gets a group of its own with allowed = 0."""
    allowed: np.ndarray
    pod_group: np.ndarray


def plan_sequence_arrays(predicateChecker: PredicateChecker, snapshot_handle, cluster_ptr, cand_off: np.ndarray,
                         cand_pods: np.ndarray, max_drains: Optional[int] = None, first_cand: int = 0,
                         full: bool = True, limits: Optional[PdbLimits] = None) -> SequenceResult:
    """sr_plan_sequence over caller-built arrays: the loop of rescheduler.go:228-287 with
    the `break` at :286 replaced by "keep the forked state and go on", up to max_drains
    (None: no budget).  The snapshot is modified: afterwards it holds every drained
    candidate's pods on their planned nodes.  With `limits` the pass is sr_plan_sequence_pdb's: a
    candidate whose pods would exceed a group's allowance gets SR_CAND_PDB and is not planned."""
    lib = predicateChecker.lib
    n = len(cand_off) - 1
    budget = 2 ** 31 - 1 if max_drains is None else int(max_drains)  # None: no budget (the pass ends with SR_SEQ_END)
    c = capi.sr_candidates(n, capi.ptr(cand_off, capi.P32), capi.ptr(cand_pods, capi.P32), None)
    n_pods = int(cand_off[-1] - cand_off[0]) if n > 0 else 0
    drained = np.full(max(min(max(budget, 1), max(n, 1)), 1), -1, np.int32)
    status = np.full(max(n, 1), capi.SR_CAND_SKIPPED, np.int32)
    nodes = np.full(max(n_pods, 1), -1, np.int32)
    o = capi.sr_sequence_out()
    o.max_drains = budget
    o.first_cand = int(first_cand)
    o.drained = capi.ptr(drained, capi.P32)
    o.status = capi.ptr(status, capi.P32) if full else None
    o.node_of_pod = capi.ptr(nodes, capi.P32) if full else None
    remaining = None
    if limits is None:
        name = "sr_plan_sequence"
        st = lib.sr_plan_sequence(predicateChecker.handle, snapshot_handle, cluster_ptr, ctypes.byref(c),
                                  ctypes.byref(o))
    else:
        name = "sr_plan_sequence_pdb"
        allowed = np.ascontiguousarray(limits.allowed, np.int32)
        pod_group = np.ascontiguousarray(limits.pod_group, np.int32)
        if len(pod_group) != n_pods:
            raise ValueError("limits.pod_group has %d entries for %d candidate pods" % (len(pod_group), n_pods))
        remaining = np.full(max(len(allowed), 1), -1, np.int32)
        lim = capi.sr_pdb_limits(len(allowed), capi.ptr(allowed, capi.P32), capi.ptr(pod_group, capi.P32),
                                 capi.ptr(remaining, capi.P32))
        st = lib.sr_plan_sequence_pdb(predicateChecker.handle, snapshot_handle, cluster_ptr, ctypes.byref(c),
                                      ctypes.byref(lim), ctypes.byref(o))
        remaining = remaining[:len(allowed)]
    if st != capi.SR_OK:
        err = PlannerError("%s: %d %s" % (name, st, predicateChecker.last_error()))
        err.status = st
        err.drained = drained[: o.n_drained].copy()  # what the snapshot already holds
        raise err
    return SequenceResult(drained[: o.n_drained].copy(), o.stop, o.stop_cand, status[:n], nodes[:n_pods],
                          o.rounds, o.rounds_k0, o.rounds_reused, remaining)


def drainSequence(predicateChecker: PredicateChecker, spotSnapshot: ClusterSnapshot, nodes,
                  candidates: Sequence[Sequence[Pod]], max_drains: Optional[int] = None, first_cand: int = 0,
                  limits: Optional[PdbLimits] = None):
    """Several consistent drains in one tick, in the style of canDrainNode: `candidates`
    are the podsForDeletion lists of the on-demand nodes in NodeInfoArray order.  Returns
    (SequenceResult, plans) with plans = [(candidate index, [spot node name per pod])] in
    drain order; the snapshot keeps the drained candidates' pods.  On SR_SEQ_FALLBACK the
    caller judges candidate `stop_cand` with the reference path and calls again with
    first_cand = stop_cand + 1 (and, with `limits`, allowed = the result's `remaining`, less
    stop_cand's pods if it drained that candidate; pod_group follows the flattened candidates)."""
    _check_order(spotSnapshot, nodes)
    flat = [p for c in candidates for p in c]
    enc = spotSnapshot.encode_pods(flat)
    cand_off = np.zeros(len(candidates) + 1, np.int32)
    cand_off[1:] = np.cumsum([len(c) for c in candidates])
    cand_pods = np.arange(len(flat), dtype=np.int32)
    r = plan_sequence_arrays(predicateChecker, spotSnapshot.handle, enc.ptr, cand_off, cand_pods, max_drains,
                             first_cand, limits=limits)
    plans = []
    for c in r.drained:
        seg = r.node_of_pod[cand_off[c]:cand_off[c + 1]]
        for p in candidates[int(c)]:
            p.node_name = ""  # :341
        plans.append((int(c), [nodes[int(k)].Node.name for k in seg]))
    return r, plans


@dataclass
class ExplainResult:
    """sr_explain_out for n pods: why each pod is refused on the spot nodes (capi.SR_WHY_* bits)."""
    feasible: np.ndarray             # [n] spot nodes with mask 0; -1 for a fallback pod
    first: np.ndarray                # [n] first spot position with mask 0 (findSpotNodeForPod), -1 none
    counts: np.ndarray               # [n][SR_WHY_COUNT] nodes refusing for each reason
    fallback: np.ndarray             # [n] 1: outside the encoded predicate set, nothing evaluated
    node_mask: Optional[np.ndarray]  # [n][n_spot] the mask of every node (None: not asked for)
    n_spot: int = 0
    how: Optional[np.ndarray] = None  # explain_plan_arrays: [n] capi.SR_EXPLAIN_* the way each candidate went

    def reasons(self, i: int = 0) -> dict:
        """{reason name: nodes refusing for it} of pod i, reasons no node gives left out."""
        return {name: int(k) for name, k in zip(capi.WHY_NAMES, self.counts[i]) if k}

    def summary(self, i: int = 0) -> str:
        """The scheduler's line: "0/3 nodes are available: 2 CPU, 1 TAINT." """
        n_spot = self.n_spot
        why = ", ".join("%d %s" % (k, name) for name, k in self.reasons(i).items())
        return "%d/%d nodes are available%s." % (max(int(self.feasible[i]), 0), n_spot, ": " + why if why else "")


def _explain_out(n: int, n_spot: int, node_mask: bool):
    feasible = np.full(max(n, 1), -1, np.int32)
    first = np.full(max(n, 1), -1, np.int32)
    counts = np.zeros((max(n, 1), capi.SR_WHY_COUNT), np.int32)
    fallback = np.zeros(max(n, 1), np.uint8)
    masks = np.zeros((max(n, 1), max(n_spot, 1)), np.uint16) if node_mask else None
    # the struct keeps the pointers it is given, and they their arrays (capi._KeepsArrays)
    o = capi.sr_explain_out(capi.ptr(feasible, capi.P32), capi.ptr(first, capi.P32), capi.ptr(counts, capi.P32),
                            capi.ptr(masks, capi.PU16) if node_mask else None, capi.ptr(fallback, capi.PU8))
    res = ExplainResult(feasible[:n], first[:n], counts[:n], fallback[:n], masks[:n, :n_spot] if node_mask else None,
                        n_spot)
    return o, res


def explain_arrays(predicateChecker: PredicateChecker, snapshot_handle, cluster_ptr, pods: np.ndarray,
                   node_mask: bool = True) -> ExplainResult:
    """sr_explain_pods over caller-built arrays: every pod judged against the snapshot as it is."""
    lib = predicateChecker.lib
    pods = np.ascontiguousarray(pods, np.int32)
    o, res = _explain_out(len(pods), lib.sr_snapshot_num_nodes(snapshot_handle), node_mask)
    st = lib.sr_explain_pods(predicateChecker.handle, snapshot_handle, cluster_ptr, capi.ptr(pods, capi.P32), len(pods),
                             ctypes.byref(o))
    if st != capi.SR_OK:
        raise PlannerError("sr_explain_pods: %d %s" % (st, predicateChecker.last_error()))
    return res


def explain_candidate_arrays(predicateChecker: PredicateChecker, snapshot_handle, cluster_ptr, pods: np.ndarray,
                             node_of_pod: np.ndarray, at_pod: int, node_mask: bool = True) -> ExplainResult:
    """sr_explain_candidate: pods[at_pod] explained with pods[:at_pod] added at node_of_pod (the plan's mapping);
    the snapshot is restored."""
    lib = predicateChecker.lib
    pods = np.ascontiguousarray(pods, np.int32)
    node_of_pod = np.ascontiguousarray(node_of_pod, np.int32)
    o, res = _explain_out(1, lib.sr_snapshot_num_nodes(snapshot_handle), node_mask)
    st = lib.sr_explain_candidate(predicateChecker.handle, snapshot_handle, cluster_ptr, capi.ptr(pods, capi.P32),
                                  len(pods), capi.ptr(node_of_pod, capi.P32), int(at_pod), ctypes.byref(o))
    if st != capi.SR_OK:
        err = PlannerError("sr_explain_candidate: %d %s" % (st, predicateChecker.last_error()))
        err.status = st
        raise err
    return res


def explainPods(predicateChecker: PredicateChecker, spotSnapshot: ClusterSnapshot, nodes, pods: Sequence[Pod],
                node_mask: bool = True) -> ExplainResult:
    """What the reference logs per spot node at rescheduler.go:348, for every pod at once."""
    _check_order(spotSnapshot, nodes)
    enc = spotSnapshot.encode_pods(list(pods))
    return explain_arrays(predicateChecker, spotSnapshot.handle, enc.ptr, np.arange(len(pods), dtype=np.int32),
                          node_mask)


def explainCandidate(predicateChecker: PredicateChecker, spotSnapshot: ClusterSnapshot, nodes, pods: Sequence[Pod],
                     mapping: Sequence[str], at_pod: int, node_mask: bool = True) -> ExplainResult:
    """Why canDrainNode stopped at pods[at_pod]: `mapping` is the spot node name of every earlier pod
    (canDrainNode.last_mapping)."""
    _check_order(spotSnapshot, nodes)
    enc = spotSnapshot.encode_pods(list(pods))
    pos = {name: i for i, name in enumerate(_node_names(nodes))}
    node_of_pod = np.array([pos.get(mapping[k], -1) if k < at_pod else -1 for k in range(len(pods))], np.int32)
    return explain_candidate_arrays(predicateChecker, spotSnapshot.handle, enc.ptr,
                                    np.arange(len(pods), dtype=np.int32), node_of_pod, at_pod, node_mask)


def explain_plan_arrays(predicateChecker: PredicateChecker, snapshot_handle, cluster_ptr, cand_off: np.ndarray,
                        cand_pods: np.ndarray, at_pod: np.ndarray, node_of_pod: np.ndarray,
                        node_mask: bool = True) -> ExplainResult:
    """sr_explain_plan: candidate c's pod at_pod[c] (negative: not asked; plan.status as it is) explained with its
    earlier pods at node_of_pod (plan.node_of_pod; None is allowed when no asked candidate has an earlier pod);
    results by candidate, `how` says which way each went."""
    lib = predicateChecker.lib
    cand_off = np.ascontiguousarray(cand_off, np.int32)
    cand_pods = np.ascontiguousarray(cand_pods, np.int32)
    at_pod = np.ascontiguousarray(at_pod, np.int32)
    if node_of_pod is not None:
        node_of_pod = np.ascontiguousarray(node_of_pod, np.int32)
    n = len(cand_off) - 1
    if len(at_pod) != n:
        raise ValueError("at_pod needs one entry per candidate")
    c = capi.sr_candidates(n, capi.ptr(cand_off, capi.P32), capi.ptr(cand_pods, capi.P32), None)
    o, res = _explain_out(n, lib.sr_snapshot_num_nodes(snapshot_handle), node_mask)
    how = np.zeros(max(n, 1), np.uint8)
    st = lib.sr_explain_plan(predicateChecker.handle, snapshot_handle, cluster_ptr, ctypes.byref(c),
                             capi.ptr(at_pod, capi.P32),
                             capi.ptr(node_of_pod, capi.P32) if node_of_pod is not None else None, ctypes.byref(o),
                             capi.ptr(how, capi.PU8))
    if st != capi.SR_OK:
        err = PlannerError("sr_explain_plan: %d %s" % (st, predicateChecker.last_error()))
        err.status = st
        raise err
    res.how = how[:n]
    return res


def explainPlan(predicateChecker: PredicateChecker, spotSnapshot: ClusterSnapshot, nodes,
                candidates: Sequence[Sequence[Pod]], plan, node_mask: bool = True) -> ExplainResult:
    """Why every stuck candidate of `plan` (plan_arrays' result for `candidates`) stopped, in one call."""
    _check_order(spotSnapshot, nodes)
    flat = [p for c in candidates for p in c]
    enc = spotSnapshot.encode_pods(flat)
    cand_off = np.zeros(len(candidates) + 1, np.int32)
    cand_off[1:] = np.cumsum([len(c) for c in candidates])
    return explain_plan_arrays(predicateChecker, spotSnapshot.handle, enc.ptr, cand_off,
                               np.arange(len(flat), dtype=np.int32), plan.status, plan.node_of_pod, node_mask)


@dataclass
class ShortfallResult:
    """sr_shortfall_out for n pods: what each pod NodeResourcesFit refuses is short of (capi.SR_SHORT_* dimensions)."""
    near: np.ndarray                  # [n] nodes only NodeResourcesFit's four checks refuse; -1 for a fallback pod
    only_nodes: np.ndarray            # [n][SR_SHORT_COUNT] nodes whose mask is exactly that dimension's bit
    only_min: np.ndarray              # [n][SR_SHORT_COUNT] smallest shortfall among them, 0 when none
    only_at: np.ndarray               # [n][SR_SHORT_COUNT] lowest spot position attaining it, -1 when none
    node_short: Optional[np.ndarray]  # [n][n_spot][SR_SHORT_COUNT] every node's shortfalls (None: not asked for)

    def closest(self, i: int = 0) -> dict:
        """{dimension name: (shortfall, spot position)} of pod i over the nodes short of that dimension alone."""
        return {name: (int(self.only_min[i][d]), int(self.only_at[i][d]))
                for d, name in enumerate(capi.SHORT_NAMES) if self.only_at[i][d] >= 0}


def _shortfall_out(n: int, n_spot: int, node_short: bool):
    m = max(n, 1)
    near = np.full(m, -1, np.int32)
    only_nodes = np.zeros((m, capi.SR_SHORT_COUNT), np.int32)
    only_min = np.zeros((m, capi.SR_SHORT_COUNT), np.int64)
    only_at = np.full((m, capi.SR_SHORT_COUNT), -1, np.int32)
    short = np.zeros((m, max(n_spot, 1), capi.SR_SHORT_COUNT), np.int64) if node_short else None
    o = capi.sr_shortfall_out(capi.ptr(near, capi.P32), capi.ptr(only_nodes, capi.P32), capi.ptr(only_min, capi.P64),
                              capi.ptr(only_at, capi.P32), capi.ptr(short, capi.P64) if node_short else None)
    res = ShortfallResult(near[:n], only_nodes[:n], only_min[:n], only_at[:n],
                          short[:n, :n_spot] if node_short else None)
    return o, res


def shortfall_arrays(predicateChecker: PredicateChecker, snapshot_handle, cluster_ptr, pods: np.ndarray,
                     node_short: bool = True, node_mask: bool = True, why: bool = True):
    """sr_shortfall_pods over caller-built arrays: (ExplainResult or None when `why` is False, ShortfallResult)."""
    lib = predicateChecker.lib
    pods = np.ascontiguousarray(pods, np.int32)
    n_spot = lib.sr_snapshot_num_nodes(snapshot_handle)
    o, res = _explain_out(len(pods), n_spot, node_mask) if why else (None, None)
    so, short = _shortfall_out(len(pods), n_spot, node_short)
    st = lib.sr_shortfall_pods(predicateChecker.handle, snapshot_handle, cluster_ptr, capi.ptr(pods, capi.P32),
                               len(pods), ctypes.byref(o) if why else None, ctypes.byref(so))
    if st != capi.SR_OK:
        err = PlannerError("sr_shortfall_pods: %d %s" % (st, predicateChecker.last_error()))
        err.status = st
        raise err
    return res, short


def shortfall_plan_arrays(predicateChecker: PredicateChecker, snapshot_handle, cluster_ptr, cand_off: np.ndarray,
                          cand_pods: np.ndarray, at_pod: np.ndarray, node_of_pod: np.ndarray,
                          node_short: bool = True, node_mask: bool = True, why: bool = True):
    """sr_shortfall_plan, arguments as explain_plan_arrays: (ExplainResult with `how`, ShortfallResult); without
    `why` the first is an ExplainResult that carries `how` alone."""
    lib = predicateChecker.lib
    cand_off = np.ascontiguousarray(cand_off, np.int32)
    cand_pods = np.ascontiguousarray(cand_pods, np.int32)
    at_pod = np.ascontiguousarray(at_pod, np.int32)
    if node_of_pod is not None:
        node_of_pod = np.ascontiguousarray(node_of_pod, np.int32)
    n = len(cand_off) - 1
    if len(at_pod) != n:
        raise ValueError("at_pod needs one entry per candidate")
    n_spot = lib.sr_snapshot_num_nodes(snapshot_handle)
    c = capi.sr_candidates(n, capi.ptr(cand_off, capi.P32), capi.ptr(cand_pods, capi.P32), None)
    o, res = _explain_out(n, n_spot, node_mask) if why else (None, ExplainResult(None, None, None, None, None, n_spot))
    so, short = _shortfall_out(n, n_spot, node_short)
    how = np.zeros(max(n, 1), np.uint8)
    st = lib.sr_shortfall_plan(predicateChecker.handle, snapshot_handle, cluster_ptr, ctypes.byref(c),
                               capi.ptr(at_pod, capi.P32),
                               capi.ptr(node_of_pod, capi.P32) if node_of_pod is not None else None,
                               ctypes.byref(o) if why else None, ctypes.byref(so), capi.ptr(how, capi.PU8))
    if st != capi.SR_OK:
        err = PlannerError("sr_shortfall_plan: %d %s" % (st, predicateChecker.last_error()))
        err.status = st
        raise err
    res.how = how[:n]
    return res, short


def shortfallPods(predicateChecker: PredicateChecker, spotSnapshot: ClusterSnapshot, nodes, pods: Sequence[Pod],
                  node_short: bool = True, node_mask: bool = True):
    """explainPods with "by how much": (ExplainResult, ShortfallResult) from one device pass."""
    _check_order(spotSnapshot, nodes)
    enc = spotSnapshot.encode_pods(list(pods))
    return shortfall_arrays(predicateChecker, spotSnapshot.handle, enc.ptr, np.arange(len(pods), dtype=np.int32),
                            node_short, node_mask)


def shortfallPlan(predicateChecker: PredicateChecker, spotSnapshot: ClusterSnapshot, nodes,
                  candidates: Sequence[Sequence[Pod]], plan, node_short: bool = True, node_mask: bool = True):
    """explainPlan with "by how much" for every stuck candidate of `plan`: (ExplainResult, ShortfallResult)."""
    _check_order(spotSnapshot, nodes)
    flat = [p for c in candidates for p in c]
    enc = spotSnapshot.encode_pods(flat)
    cand_off = np.zeros(len(candidates) + 1, np.int32)
    cand_off[1:] = np.cumsum([len(c) for c in candidates])
    return shortfall_plan_arrays(predicateChecker, spotSnapshot.handle, enc.ptr, cand_off,
                                 np.arange(len(flat), dtype=np.int32), plan.status, plan.node_of_pod, node_short,
                                 node_mask)


@dataclass
class NodeViewResult:
    """sr_node_view_out: what each spot node refuses, over the judged queries (asked, inside the encoded set)."""
    judged: int            # queries evaluated
    admits: np.ndarray     # [n_spot] judged queries whose mask on the node is 0
    near: np.ndarray       # [n_spot] ... for which the node is a near miss
    refuses: np.ndarray    # [n_spot][SR_WHY_COUNT] ... whose mask on the node holds the bit
    sole: np.ndarray       # [n_spot][SR_WHY_COUNT] ... whose mask on the node is exactly that bit
    sole_min: np.ndarray   # [n_spot][SR_SHORT_COUNT] smallest shortfall among the sole-d queries, 0 when none
    sole_at: np.ndarray    # [n_spot][SR_SHORT_COUNT] lowest query slot attaining it, -1 when none
    fallback: np.ndarray   # [n] 1: outside the encoded predicate set, counted nowhere
    how: Optional[np.ndarray] = None  # node_view_plan_arrays: [n] capi.SR_EXPLAIN_* the way each candidate went

    def sole_reasons(self, node: int) -> dict:
        """{reason name: queries only that reason keeps off the node}, reasons with none left out: the single
        thing that, put right, frees that many queries there."""
        return {name: int(k) for name, k in zip(capi.WHY_NAMES, self.sole[node]) if k}

    def closest(self, node: int) -> dict:
        """{dimension name: (shortfall, query slot)} of the node over the queries short of that dimension alone."""
        return {name: (int(self.sole_min[node][d]), int(self.sole_at[node][d]))
                for d, name in enumerate(capi.SHORT_NAMES) if self.sole_at[node][d] >= 0}


def _node_view_out(n: int, n_spot: int):
    m, s = max(n, 1), max(n_spot, 1)
    judged = np.zeros(1, np.int32)
    admits = np.zeros(s, np.int32)
    near = np.zeros(s, np.int32)
    refuses = np.zeros((s, capi.SR_WHY_COUNT), np.int32)
    sole = np.zeros((s, capi.SR_WHY_COUNT), np.int32)
    sole_min = np.zeros((s, capi.SR_SHORT_COUNT), np.int64)
    sole_at = np.full((s, capi.SR_SHORT_COUNT), -1, np.int32)
    fallback = np.zeros(m, np.uint8)
    o = capi.sr_node_view_out(capi.ptr(judged, capi.P32), capi.ptr(admits, capi.P32), capi.ptr(near, capi.P32),
                              capi.ptr(refuses, capi.P32), capi.ptr(sole, capi.P32), capi.ptr(sole_min, capi.P64),
                              capi.ptr(sole_at, capi.P32), capi.ptr(fallback, capi.PU8))

    def result():
        return NodeViewResult(int(judged[0]), admits[:n_spot], near[:n_spot], refuses[:n_spot], sole[:n_spot],
                              sole_min[:n_spot], sole_at[:n_spot], fallback[:n])
    return o, result


def node_view_arrays(predicateChecker: PredicateChecker, snapshot_handle, cluster_ptr,
                     pods: np.ndarray) -> NodeViewResult:
    """sr_node_view_pods over caller-built arrays: every pod judged against the snapshot as it is, reduced per
    spot node on the device; a query's slot is its index in `pods`."""
    lib = predicateChecker.lib
    pods = np.ascontiguousarray(pods, np.int32)
    o, result = _node_view_out(len(pods), lib.sr_snapshot_num_nodes(snapshot_handle))
    st = lib.sr_node_view_pods(predicateChecker.handle, snapshot_handle, cluster_ptr, capi.ptr(pods, capi.P32),
                               len(pods), ctypes.byref(o))
    if st != capi.SR_OK:
        err = PlannerError("sr_node_view_pods: %d %s" % (st, predicateChecker.last_error()))
        err.status = st
        raise err
    return result()


def node_view_plan_arrays(predicateChecker: PredicateChecker, snapshot_handle, cluster_ptr, cand_off: np.ndarray,
                          cand_pods: np.ndarray, at_pod: np.ndarray, node_of_pod: np.ndarray) -> NodeViewResult:
    """sr_node_view_plan, arguments as explain_plan_arrays: every asked candidate's stop pod in the context of its
    earlier pods, reduced per spot node; a query's slot is its candidate."""
    lib = predicateChecker.lib
    cand_off = np.ascontiguousarray(cand_off, np.int32)
    cand_pods = np.ascontiguousarray(cand_pods, np.int32)
    at_pod = np.ascontiguousarray(at_pod, np.int32)
    if node_of_pod is not None:
        node_of_pod = np.ascontiguousarray(node_of_pod, np.int32)
    n = len(cand_off) - 1
    if len(at_pod) != n:
        raise ValueError("at_pod needs one entry per candidate")
    c = capi.sr_candidates(n, capi.ptr(cand_off, capi.P32), capi.ptr(cand_pods, capi.P32), None)
    o, result = _node_view_out(n, lib.sr_snapshot_num_nodes(snapshot_handle))
    how = np.zeros(max(n, 1), np.uint8)
    st = lib.sr_node_view_plan(predicateChecker.handle, snapshot_handle, cluster_ptr, ctypes.byref(c),
                               capi.ptr(at_pod, capi.P32),
                               capi.ptr(node_of_pod, capi.P32) if node_of_pod is not None else None, ctypes.byref(o),
                               capi.ptr(how, capi.PU8))
    if st != capi.SR_OK:
        err = PlannerError("sr_node_view_plan: %d %s" % (st, predicateChecker.last_error()))
        err.status = st
        raise err
    res = result()
    res.how = how[:n]
    return res


def nodeViewPods(predicateChecker: PredicateChecker, spotSnapshot: ClusterSnapshot, nodes,
                 pods: Sequence[Pod]) -> NodeViewResult:
    """explainPods from the nodes' side: what each spot node refuses among `pods`."""
    _check_order(spotSnapshot, nodes)
    enc = spotSnapshot.encode_pods(list(pods))
    return node_view_arrays(predicateChecker, spotSnapshot.handle, enc.ptr, np.arange(len(pods), dtype=np.int32))


def nodeViewPlan(predicateChecker: PredicateChecker, spotSnapshot: ClusterSnapshot, nodes,
                 candidates: Sequence[Sequence[Pod]], plan) -> NodeViewResult:
    """explainPlan from the nodes' side: what each spot node refuses among the stuck candidates of `plan`."""
    _check_order(spotSnapshot, nodes)
    flat = [p for c in candidates for p in c]
    enc = spotSnapshot.encode_pods(flat)
    cand_off = np.zeros(len(candidates) + 1, np.int32)
    cand_off[1:] = np.cumsum([len(c) for c in candidates])
    return node_view_plan_arrays(predicateChecker, spotSnapshot.handle, enc.ptr, cand_off,
                                 np.arange(len(flat), dtype=np.int32), plan.status, plan.node_of_pod)


@dataclass
class BlockersResult:
    """sr_blockers_out for n candidates: every pod that keeps a stuck candidate from draining."""
    blockers: np.ndarray      # [n] pods of the candidate that fit nowhere; -1: not asked, or fallback
    first: np.ndarray         # [n] index of the first blocker in the candidate's list, -1: none
    node_of_pod: np.ndarray   # [pods of the list] spot position; -1: blocker, or pod of a candidate not judged
    counts: Optional[np.ndarray]  # [pods of the list][SR_WHY_COUNT] a blocker's refusing nodes per reason, or None
    fallback: np.ndarray      # [n] 1: a pod of the candidate lies outside the encoded set
    how: np.ndarray           # [n] capi.SR_EXPLAIN_* the way each candidate went
    cand_off: np.ndarray      # [n + 1] the candidates' pods in node_of_pod / counts (relative to the first)

    def blocker_pods(self, c: int) -> List[int]:
        """The indices, in candidate c's list, of its pods that fit nowhere."""
        if self.blockers[c] < 0:
            return []
        row = self.node_of_pod[self.cand_off[c]:self.cand_off[c + 1]]
        return [int(k) for k in np.nonzero(row < 0)[0]]

    def ranking(self) -> List[int]:
        """The judged candidates with at least one blocker, fewest blockers first (ties in candidate order):
        where an operator's effort goes furthest."""
        stuck = [c for c in range(len(self.blockers)) if self.blockers[c] > 0]
        return sorted(stuck, key=lambda c: (int(self.blockers[c]), c))


def blockers_plan_arrays(predicateChecker: PredicateChecker, snapshot_handle, cluster_ptr, cand_off: np.ndarray,
                         cand_pods: np.ndarray, ask: np.ndarray, counts: bool = True) -> BlockersResult:
    """sr_blockers_plan: canDrainNode's loop without its early return for every candidate with ask[c] >= 0
    (plan.status as it is asks for the stuck ones)."""
    lib = predicateChecker.lib
    cand_off = np.ascontiguousarray(cand_off, np.int32)
    cand_pods = np.ascontiguousarray(cand_pods, np.int32)
    ask = np.ascontiguousarray(ask, np.int32)
    n = len(cand_off) - 1
    if len(ask) != n:
        raise ValueError("ask needs one entry per candidate")
    total = int(cand_off[n] - cand_off[0]) if n > 0 else 0
    c = capi.sr_candidates(n, capi.ptr(cand_off, capi.P32), capi.ptr(cand_pods, capi.P32), None)
    blockers = np.full(max(n, 1), -1, np.int32)
    first = np.full(max(n, 1), -1, np.int32)
    node_of_pod = np.full(max(total, 1), -1, np.int32)
    cnt = np.zeros((max(total, 1), capi.SR_WHY_COUNT), np.int32) if counts else None
    fallback = np.zeros(max(n, 1), np.uint8)
    how = np.zeros(max(n, 1), np.uint8)
    o = capi.sr_blockers_out(capi.ptr(blockers, capi.P32), capi.ptr(first, capi.P32), capi.ptr(node_of_pod, capi.P32),
                             capi.ptr(cnt, capi.P32) if counts else None, capi.ptr(fallback, capi.PU8))
    st = lib.sr_blockers_plan(predicateChecker.handle, snapshot_handle, cluster_ptr, ctypes.byref(c),
                              capi.ptr(ask, capi.P32), ctypes.byref(o), capi.ptr(how, capi.PU8))
    if st != capi.SR_OK:
        err = PlannerError("sr_blockers_plan: %d %s" % (st, predicateChecker.last_error()))
        err.status = st
        raise err
    return BlockersResult(blockers[:n], first[:n], node_of_pod[:total], cnt[:total] if counts else None, fallback[:n],
                          how[:n], cand_off - cand_off[0] if n > 0 else np.zeros(1, np.int32))


def blockersPlan(predicateChecker: PredicateChecker, spotSnapshot: ClusterSnapshot, nodes,
                 candidates: Sequence[Sequence[Pod]], plan, counts: bool = True) -> BlockersResult:
    """Every blocker of every stuck candidate of `plan` (plan_arrays' result for `candidates`), in one call."""
    _check_order(spotSnapshot, nodes)
    flat = [p for c in candidates for p in c]
    enc = spotSnapshot.encode_pods(flat)
    cand_off = np.zeros(len(candidates) + 1, np.int32)
    cand_off[1:] = np.cumsum([len(c) for c in candidates])
    return blockers_plan_arrays(predicateChecker, spotSnapshot.handle, enc.ptr, cand_off,
                                np.arange(len(flat), dtype=np.int32), plan.status, counts)


@dataclass
class EvacuateResult:
    """sr_evacuate_out for n scenarios: what losing each scenario's spot nodes strands."""
    stranded: np.ndarray      # [n] pods of the scenario that fit on no surviving node; -1: not judged
    first: np.ndarray         # [n] index of the first stranded pod in the scenario's list, -1: none / not judged
    node_of_pod: np.ndarray   # [pods of the list] position in the original spot list; -1: stranded, or not judged
    counts: Optional[np.ndarray]  # [pods of the list][SR_WHY_COUNT] a stranded pod's refusing surviving nodes, or None
    how: np.ndarray           # [n] capi.SR_EVAC_JUDGED / SR_EVAC_FALLBACK / SR_EVAC_NOT_PLAIN
    scen_off: np.ndarray      # [n + 1] the scenarios' pods in node_of_pod / counts (relative to the first)

    def stranded_pods(self, s: int) -> List[int]:
        """The indices, in scenario s's list, of its pods that fit nowhere."""
        if self.stranded[s] < 0:
            return []
        row = self.node_of_pod[self.scen_off[s]:self.scen_off[s + 1]]
        return [int(k) for k in np.nonzero(row < 0)[0]]

    def ranking(self) -> List[int]:
        """The judged scenarios that strand at least one pod, most stranded pods first (ties in scenario
        order): the reclaims that hurt most."""
        hit = [s for s in range(len(self.stranded)) if self.stranded[s] > 0]
        return sorted(hit, key=lambda s: (-int(self.stranded[s]), s))

    def not_answered(self) -> List[int]:
        """The scenarios the call reports nothing for (NOT_PLAIN or FALLBACK): the caller answers them by
        building the reduced snapshot and calling blockers_plan_arrays on it."""
        return [s for s in range(len(self.how)) if self.how[s] != capi.SR_EVAC_JUDGED]


def evacuate_plan_arrays(predicateChecker: PredicateChecker, snapshot_handle, cluster_ptr, scen_off: np.ndarray,
                         scen_pods: np.ndarray, lost_off: np.ndarray, lost_pos: np.ndarray,
                         counts: bool = True) -> EvacuateResult:
    """sr_evacuate_plan: scenario s loses the spot positions lost_pos[lost_off[s]:lost_off[s + 1]] and re-places
    the pods scen_pods[scen_off[s]:scen_off[s + 1]], in order, on the surviving nodes."""
    lib = predicateChecker.lib
    scen_off = np.ascontiguousarray(scen_off, np.int32)
    scen_pods = np.ascontiguousarray(scen_pods, np.int32)
    lost_off = np.ascontiguousarray(lost_off, np.int32)
    lost_pos = np.ascontiguousarray(lost_pos, np.int32)
    n = len(scen_off) - 1
    if len(lost_off) != n + 1:
        raise ValueError("lost_off needs one entry per scenario and one more")
    total = int(scen_off[n] - scen_off[0]) if n > 0 else 0
    c = capi.sr_candidates(n, capi.ptr(scen_off, capi.P32), capi.ptr(scen_pods, capi.P32), None)
    stranded = np.full(max(n, 1), -1, np.int32)
    first = np.full(max(n, 1), -1, np.int32)
    node_of_pod = np.full(max(total, 1), -1, np.int32)
    cnt = np.zeros((max(total, 1), capi.SR_WHY_COUNT), np.int32) if counts else None
    how = np.zeros(max(n, 1), np.uint8)
    o = capi.sr_evacuate_out(capi.ptr(stranded, capi.P32), capi.ptr(first, capi.P32), capi.ptr(node_of_pod, capi.P32),
                             capi.ptr(cnt, capi.P32) if counts else None, capi.ptr(how, capi.PU8))
    st = lib.sr_evacuate_plan(predicateChecker.handle, snapshot_handle, cluster_ptr, ctypes.byref(c),
                              capi.ptr(lost_off, capi.P32), capi.ptr(lost_pos, capi.P32), ctypes.byref(o))
    if st != capi.SR_OK:
        err = PlannerError("sr_evacuate_plan: %d %s" % (st, predicateChecker.last_error()))
        err.status = st
        raise err
    return EvacuateResult(stranded[:n], first[:n], node_of_pod[:total], cnt[:total] if counts else None, how[:n],
                          scen_off - scen_off[0] if n > 0 else np.zeros(1, np.int32))


def evacuation_scenarios(nodes, pool_key: Optional[str] = None):
    """The reclaims worth asking about, as (names, lost sets of spot positions): every spot node lost alone
    ("node:<name>"), then, with `pool_key`, every set of nodes sharing a value of that node label
    ("pool:<value>", in order of first appearance; a node without the label is in no pool)."""
    names, lost = [], []
    for i, info in enumerate(nodes):
        names.append("node:" + info.Node.name)
        lost.append([i])
    if pool_key is not None:
        pools = {}
        for i, info in enumerate(nodes):
            v = (info.Node.labels or {}).get(pool_key)
            if v is not None:
                pools.setdefault(v, []).append(i)
        for v, members in pools.items():
            names.append("pool:" + v)
            lost.append(members)
    return names, lost


def evacuatePlan(predicateChecker: PredicateChecker, spotSnapshot: ClusterSnapshot, nodes,
                 lost: Sequence[Sequence[int]], moved: Optional[Sequence[Sequence[Pod]]] = None,
                 counts: bool = True) -> EvacuateResult:
    """What each reclaim strands: scenario s loses the spot positions lost[s] of `nodes` (evacuation_scenarios
    builds the usual ones) and re-places moved[s] -- by default every pod of the lost nodes, in NodeInfoArray
    order -- on the nodes that survive."""
    _check_order(spotSnapshot, nodes)
    if moved is None:
        moved = [[p for i in sorted(set(s)) for p in nodes[i].Pods] for s in lost]
    if len(moved) != len(lost):
        raise ValueError("moved needs one pod list per scenario")
    flat = [p for m in moved for p in m]
    enc = spotSnapshot.encode_pods(flat)
    scen_off = np.zeros(len(lost) + 1, np.int32)
    scen_off[1:] = np.cumsum([len(m) for m in moved])
    lost_off = np.zeros(len(lost) + 1, np.int32)
    lost_off[1:] = np.cumsum([len(s) for s in lost])
    lost_pos = np.array([int(i) for s in lost for i in s], np.int32)
    return evacuate_plan_arrays(predicateChecker, spotSnapshot.handle, enc.ptr, scen_off,
                                np.arange(len(flat), dtype=np.int32), lost_off, lost_pos, counts)
