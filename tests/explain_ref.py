"""Reference for sr_explain_pods on random clusters, from the CPU oracle alone.

The oracle answers yes / no per (pod, node); it names no reason.  Three things
can still be said about the bits without a second implementation of the
filters:

  feasible   mask == 0 iff oracle_check_predicates says yes;
  resources  PODS / CPU / MEMORY / EPHEMERAL are fitsRequest's arithmetic
             [upstream k8s v1.19.2 noderesources/fit.go] on the oracle's own node
             state (oracle_snapshot_node_state) and the cluster arrays;
  twins      a twin of the pod stripped to zero requests and ONE group of
             fields (and, unless that group is the tolerations, tolerating
             everything) passes every other filter except the pod count, so on a node
             whose pod count admits a pod the oracle's no for the twin is that
             group's refusal: tolerations -> UNSCHEDULABLE | TAINT, selector and
             required affinity -> NODE_AFFINITY, host ports -> PORTS.  Valid on
             inputs without inter-pod terms, spread constraints and volumes
             (randcluster.rand_scenario with anti = aff = 0).
"""
from __future__ import annotations

import numpy as np

from helpers import Scenario
from oracle_lib import load_oracle
from spotplanner import capi
from spotplanner.model import Container, ContainerPort, Pod, Toleration

PODS, CPU, MEMORY, EPHEMERAL = capi.SR_WHY_PODS, capi.SR_WHY_CPU, capi.SR_WHY_MEMORY, capi.SR_WHY_EPHEMERAL
RESOURCE_BITS = PODS | CPU | MEMORY | EPHEMERAL
TWIN_GROUPS = (("tolerations", capi.SR_WHY_UNSCHEDULABLE | capi.SR_WHY_TAINT),
               ("affinity", capi.SR_WHY_NODE_AFFINITY),
               ("ports", capi.SR_WHY_PORTS))


def twin(pod: Pod, group: str, name: str) -> Pod:
    """`pod` with zero requests and only the fields of one filter group."""
    t = Pod(name, namespace=pod.namespace, containers=[Container()], owner_references=list(pod.owner_references))
    if group == "tolerations":  # without tolerations: refused wherever a taint or Spec.Unschedulable stands
        t.tolerations = list(pod.tolerations)
        return t
    t.tolerations = [Toleration("", "Exists")]  # the other groups' twins tolerate every taint and the cordon
    if group == "affinity":
        t.node_selector = dict(pod.node_selector)
        t.required_node_affinity = pod.required_node_affinity
    else:
        t.containers = [Container(ports=[ContainerPort(p.host_port, p.container_port, p.protocol, p.host_ip)
                                         for p in pod.host_ports()])]
    return t


class Reference:
    """One random scenario: its candidate pods (flattened) and their three twins
    each as query pods of one cluster; the oracle's answers computed once."""

    def __init__(self, nodes, spot_pods, pods):
        self.nodes, self.pods = nodes, list(pods)
        self.n, self.n_spot = len(self.pods), len(nodes)
        query = list(self.pods)
        for g, _ in TWIN_GROUPS:
            query += [twin(p, g, "%s-%s" % (p.name, g)) for p in self.pods]
        self.sc = Scenario(nodes, spot_pods, query)
        lib = load_oracle()
        self.osnap = self.sc.oracle_snapshot()
        self.fallback = np.array([lib.oracle_pod_needs_fallback(self.osnap.h, self.sc.ptr, self.sc.qidx(i))
                                  for i in range(self.n)], np.uint8)
        self.fits = np.array([[lib.oracle_check_predicates(self.osnap.h, self.sc.ptr, self.sc.qidx(i), j)
                               for j in range(self.n_spot)] for i in range(len(query))], np.int32)
        A = self.sc.enc.a
        state = [self.osnap.node_state(j) for j in range(self.n_spot)]
        self.requested = np.array([s[0] for s in state], np.int64)      # [n_spot][3]
        self.num_pods = np.array([s[1] for s in state], np.int64)
        self.alloc = np.stack([A["alloc_cpu"], A["alloc_mem"], A["alloc_eph"]], 1)[: self.n_spot]
        self.alloc_pods = A["alloc_pods"][: self.n_spot]
        q0 = self.sc.q0
        self.req = np.stack([A["req_cpu"], A["req_mem"], A["req_eph"]], 1)[q0: q0 + self.n]
        so = A["pod_scalar_off"]
        self.lists_scalar = np.array([so[q0 + i + 1] > so[q0 + i] for i in range(self.n)])

    def pod_indices(self):
        return np.array([self.sc.qidx(i) for i in range(self.n)], np.int32)

    def resource_mask(self, i, j) -> int:
        """fitsRequest for pod i on node j: the pod count first; an all-zero request
        listing no scalar returns there; else allocatable < request + requested per resource."""
        m = PODS if self.num_pods[j] + 1 > self.alloc_pods[j] else 0
        if not self.req[i].any() and not self.lists_scalar[i]:
            return m
        for d, bit in enumerate((CPU, MEMORY, EPHEMERAL)):
            if self.alloc[j][d] < self.req[i][d] + self.requested[j][d]:
                m |= bit
        return m

    def pods_refuses(self, j) -> bool:
        return bool(self.num_pods[j] + 1 > self.alloc_pods[j])

    def twin_refuses(self, g, i, j) -> bool:
        """The oracle's no for twin g of pod i on node j (a node whose pod count admits a pod)."""
        return self.fits[self.n * (1 + g) + i][j] == 0

    def pods_refusing_share(self) -> float:
        return float(np.mean([self.pods_refuses(j) for j in range(self.n_spot)]))

    def twin_bits_seen(self) -> int:
        """The groups some twin is refused for on a node whose pod count admits a pod."""
        seen = 0
        for g, (_, bits) in enumerate(TWIN_GROUPS):
            if any(self.twin_refuses(g, i, j) for i in range(self.n) for j in range(self.n_spot)
                   if not self.pods_refuses(j)):
                seen |= bits
        return seen

    def check(self, res):
        """Asserts an ExplainResult (with node_mask) of pod_indices() against the reference."""
        for i in range(self.n):
            if self.fallback[i]:
                assert res.fallback[i] == 1 and res.feasible[i] == -1 and res.first[i] == -1, i
                assert not res.counts[i].any() and not res.node_mask[i].any(), i
                continue
            assert res.fallback[i] == 0, i
            row = res.node_mask[i]
            for j in range(self.n_spot):
                m = int(row[j])
                assert (m == 0) == (self.fits[i][j] == 1), (self.pods[i].name, j, hex(m))
                assert m & RESOURCE_BITS == self.resource_mask(i, j), (self.pods[i].name, j, hex(m))
                if self.pods_refuses(j):
                    continue
                for g, (_, bits) in enumerate(TWIN_GROUPS):
                    assert bool(m & bits) == self.twin_refuses(g, i, j), (self.pods[i].name, j, hex(m), g)
            assert res.feasible[i] == int(np.sum(row == 0)), i
            zero = np.flatnonzero(row == 0)
            assert res.first[i] == (int(zero[0]) if len(zero) else -1), i
            for r in range(capi.SR_WHY_COUNT):
                assert res.counts[i][r] == int(np.sum((row >> r) & 1)), (i, r)
