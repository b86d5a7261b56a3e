"""Hand-written refusal masks for sr_explain_pods: for one pod, the SR_WHY_*
bits of every spot node, derived by hand from the filter rules quoted in
tests/known_answer.py.  Every case of known_answer.cases() is here (`masks`
per node; 0 where the case's answer is yes), plus cases of their own on pools
of at most 8 nodes for what the known answers do not separate: every reason on
its own (SCALAR, SPREAD, VOLUMES, and UNSCHEDULABLE apart from TAINT), nodes
refused by two and three filter groups at once, fitsRequest's zero-request
shortcut, a zero request in one resource on an over-committed node, a request
above every node's free value, a required node affinity with an empty term
list and a pod failing VolumeBinding's PreFilter.

tests/test_explain_reference.py checks on the CPU that no mask disagrees with
the oracle on feasibility; tests/test_gpu_explain.py checks the masks, counts,
feasible and first of every case on the GPU."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

from known_answer import N, P, cases as known_cases, used
from spotplanner.model import (Container, ContainerPort, GiB, LabelSelector, MiB, NodeSelectorRequirement,
                               NodeSelectorTerm, Pod, PodAffinityTerm, Taint, TopologySpreadConstraint, Volume,
                               VolumeWorld)

UNSCHEDULABLE, TAINT, NODE_AFFINITY, PODS, CPU, MEMORY, EPHEMERAL, SCALAR, PORTS, INTER_POD, SPREAD, VOLUMES = (
    1 << r for r in range(12))


@dataclass
class ExplainCase:
    name: str
    pod: Pod
    nodes: list
    base: list
    masks: List[int]
    world: Optional[VolumeWorld] = None


# ---- the known answers.  The cases of one filter alone refuse with that
# filter's bit wherever the answer is no; NodeResourcesFit's cases name the
# resource, written out node by node.
_GROUP_BIT = {"_taints": TAINT, "_unschedulable": UNSCHEDULABLE, "_affinity": NODE_AFFINITY, "_ports": PORTS,
              "_interpod": INTER_POD}
_RESOURCE_MASKS = {
    "memory_exact_fit": [0, MEMORY],
    "ephemeral_exact_fit": [0, EPHEMERAL, EPHEMERAL],
    "cpu_exact_fit": [0, CPU],
    "pod_count": [PODS, 0, PODS],
    "zero_request_skips_resources": [0],
    "nonzero_request_on_overcommitted_node": [MEMORY, 0],
    "init_container_max": [CPU, 0, MEMORY],           # cpu 800 on 1000 - 201; memory 1Gi on 2Gi - (1Gi + 1)
    "pod_overhead": [CPU, 0, MEMORY],                 # cpu 600 on 1000 - 401; memory 100Mi on 1Gi - (924Mi + 1)
    "sum_of_containers": [CPU, 0],
    "scalar_request_needs_the_resource": [0, SCALAR, SCALAR, 0],
    "scalar_zero_request_listed": [0, 0],
    "hugepages_exact_fit": [0, SCALAR],
    "scalar_init_container_max": [SCALAR, 0],
    "scalar_overhead": [SCALAR, 0],
    "scalar_and_cpu_both_checked": [CPU, 0],          # the gpu fits on both; cpu 900 on 1000 - 200
    "node_accounting_skips_init_containers": [0],
}


def _known():
    import known_answer
    group_of = {}
    for g in ("_resources", "_scalar", "_taints", "_unschedulable", "_affinity", "_ports", "_interpod"):
        for c in getattr(known_answer, g)():
            group_of[c.name] = g
    out = []
    for c in known_cases():
        if c.name in _RESOURCE_MASKS:
            masks = _RESOURCE_MASKS[c.name]
        else:
            masks = [0 if f else _GROUP_BIT[group_of[c.name]] for f in c.fits]
        assert len(masks) == len(c.nodes), c.name
        out.append(ExplainCase(c.name, c.pod, c.nodes, c.base, masks))
    return out


# ---- cases of their own
def _hp(name, port):
    return Pod(name, containers=[Container(cpu_milli=10, ports=[ContainerPort(port)])])


def _own():
    k = Taint("k", "v", "NoSchedule")
    yield ExplainCase(
        "x_unschedulable_apart_from_taint", P(),
        [N("a", unschedulable=True), N("b", taints=[k]), N("c", unschedulable=True, taints=[k]), N("d")],
        [[], [], [], []], [UNSCHEDULABLE, TAINT, UNSCHEDULABLE | TAINT, 0])
    E = 10 * GiB
    yield ExplainCase(
        "x_each_resource_alone", P(cpu=500, mem=1 * GiB, eph=1 * GiB),
        [N("a", cpu=1000, eph=E), N("b", mem=2 * GiB, eph=E), N("c", eph=E), N("d", pods=1, eph=E), N("e", eph=E)],
        [[used(cpu=501)], [used(mem=1 * GiB + 1)], [used(eph=9 * GiB + 1)], [used()], [used(cpu=3500)]],
        [CPU, MEMORY, EPHEMERAL, PODS, 0])
    yield ExplainCase(
        "x_pods_with_cpu", P(cpu=500, mem=64 * MiB),
        [N("a", cpu=1000, pods=1), N("b", cpu=1000, mem=1 * GiB, pods=2), N("c", cpu=1000, pods=1), N("d", cpu=1000)],
        [[used(cpu=600)], [used(cpu=600), used(mem=1 * GiB, name="m")], [used(cpu=100)], [used(cpu=500)]],
        [PODS | CPU, PODS | CPU | MEMORY, PODS, 0])
    p = Pod("p", containers=[Container(cpu_milli=100, ports=[ContainerPort(80)])], node_selector={"zone": "a"})
    yield ExplainCase(
        "x_taint_with_affinity_with_ports", p,
        [N("a", labels={"zone": "b"}, taints=[k]), N("b", labels={"zone": "a"}), N("c", labels={"zone": "a"}),
         N("d", labels={"zone": "a"}, taints=[k]), N("e", labels={"zone": "b"}), N("f", taints=[k])],
        [[_hp("x", 80)], [_hp("y", 80)], [_hp("z", 8080)], [], [], [_hp("u", 80)]],
        [TAINT | NODE_AFFINITY | PORTS, PORTS, 0, TAINT, NODE_AFFINITY, TAINT | NODE_AFFINITY | PORTS])
    yield ExplainCase(
        "x_zero_request_shortcut", P(cpu=0),
        [N("a", cpu=1000, mem=1 * GiB), N("b", cpu=1000, mem=1 * GiB, pods=1)],
        [[used(cpu=5000, mem=4 * GiB)], [used(cpu=5000, mem=4 * GiB)]], [0, PODS])
    yield ExplainCase(
        "x_zero_cpu_request_on_overcommitted_node", P(cpu=0, mem=1 * MiB),
        [N("a", cpu=1000), N("b", cpu=1000), N("c", cpu=1000, mem=1 * GiB)],
        [[used(cpu=1500)], [used(cpu=1000)], [used(cpu=1001, mem=1 * GiB)]], [CPU, 0, CPU | MEMORY])
    yield ExplainCase(
        "x_request_above_every_node", P(cpu=9000),
        [N("a", cpu=4000), N("b", cpu=8000, taints=[k]), N("c", cpu=8000, mem=1 * GiB)],
        [[], [], [used(mem=2 * GiB)]], [CPU, CPU | TAINT, CPU | MEMORY])
    yield ExplainCase(
        "x_affinity_with_empty_term_list", P(required_node_affinity=[]),
        [N("a"), N("b", taints=[k]), N("c", cpu=1000)], [[], [], [used(cpu=950)]],
        [NODE_AFFINITY, NODE_AFFINITY | TAINT, NODE_AFFINITY | CPU])
    yield ExplainCase(
        "x_prefilter_fail", Pod("p", containers=[Container(cpu_milli=100)], volumes=[Volume(claim="no-such-claim")]),
        [N("a"), N("b", taints=[k]), N("c", pods=0)], [[], [], []], [VOLUMES, VOLUMES | TAINT, VOLUMES | PODS],
        VolumeWorld())
    G = "nvidia.com/gpu"
    gpu = Pod("p", containers=[Container(cpu_milli=900, scalar={G: 2})])
    yield ExplainCase(
        "x_scalar_alone_and_with_cpu", gpu,
        [N("a", cpu=1000, scalar={G: 1}), N("b", cpu=1000, scalar={G: 2}), N("c", cpu=1000),
         N("d", cpu=1000, scalar={G: 4})],
        [[], [used(cpu=200)], [used(cpu=200)], [Pod("u", containers=[Container(cpu_milli=10, scalar={G: 2})])]],
        [SCALAR, CPU, SCALAR | CPU, 0])
    web = LabelSelector({"app": "web"})

    def w(name):
        return Pod(name, labels={"app": "web"}, containers=[Container(cpu_milli=10)])
    sp = Pod("p", labels={"app": "web"}, containers=[Container(cpu_milli=10)],
             topology_spread=[TopologySpreadConstraint(1, "zone", label_selector=web)])
    # zone a counts 2, zone b counts 0: 2 + 1 - 0 > maxSkew on a's nodes; a node without the key is refused
    yield ExplainCase(
        "x_spread_alone", sp,
        [N("a", labels={"zone": "a"}), N("b", labels={"zone": "b"}), N("c", labels={"zone": "a"}), N("d"),
         N("e", labels={"zone": "b"}, taints=[k])],
        [[w("w1"), w("w2")], [], [], [], []], [SPREAD, 0, SPREAD, SPREAD, TAINT])
    iscsi = Pod("p", containers=[Container(cpu_milli=10, ports=[ContainerPort(80)])], volumes=[Volume(iscsi_iqn="iqn-1")])

    def disk(name, vol):
        return Pod(name, containers=[Container(cpu_milli=10)], volumes=[Volume(iscsi_iqn=vol)])
    # VolumeRestrictions: two read-write mounts of one ISCSI volume conflict; apart from the host port of the same pod
    yield ExplainCase(
        "x_volumes_alone_and_with_ports", iscsi, [N("a"), N("b"), N("c"), N("d")],
        [[disk("x", "iqn-1")], [_hp("y", 80)], [disk("z", "iqn-1"), _hp("u", 80)], [disk("v", "iqn-2")]],
        [VOLUMES, PORTS, VOLUMES | PORTS, 0], VolumeWorld())
    Z = "zone"
    anti = Pod("p", namespace="default", labels={"app": "web"}, containers=[Container(cpu_milli=10)],
               pod_anti_affinity=[PodAffinityTerm(Z, LabelSelector({"app": "db"}))],
               required_node_affinity=[NodeSelectorTerm([NodeSelectorRequirement(Z, "In", ["a", "b"])])])

    def db(name):
        return Pod(name, namespace="default", labels={"app": "db"}, containers=[Container(cpu_milli=10)])
    yield ExplainCase(
        "x_inter_pod_with_affinity", anti,
        [N("a", labels={Z: "a"}), N("b", labels={Z: "a"}), N("c", labels={Z: "b"}), N("d", labels={Z: "c"}), N("e")],
        [[db("d1")], [], [], [db("d2")], []], [INTER_POD, INTER_POD, 0, INTER_POD | NODE_AFFINITY, NODE_AFFINITY])


def cases() -> List[ExplainCase]:
    out = _known() + list(_own())
    names = [c.name for c in out]
    assert len(names) == len(set(names))
    return out


def scenario(case: ExplainCase):
    from helpers import Scenario
    return Scenario(case.nodes, case.base, [case.pod], volumes=case.world)
