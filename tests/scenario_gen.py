"""Random scenario generators shared by the test modules of their predicates
(test_volumes.py, test_topology_spread.py, test_scalar_resources.py) and the
sequence inputs (sequence_ref.py): importable without any module's fixtures or
parametrised tests.  Each returns (spot nodes, their pods, candidates[, volume
world]) for helpers.Scenario; the seeds are deterministic."""
import random

from randcluster import rand_scenario
from spotplanner.model import (Container, GiB, LabelSelector, LabelSelectorRequirement, Node, NodeSelectorRequirement,
                               NodeSelectorTerm, PersistentVolume, PersistentVolumeClaim, Pod,
                               TopologySpreadConstraint, Volume, VolumeWorld)

TZ, TR = "topology.kubernetes.io/zone", "topology.kubernetes.io/region"
Z = TZ
H = "kubernetes.io/hostname"
EBS_CSI = "ebs.csi.aws.com"
G = "nvidia.com/gpu"
WEB = LabelSelector(match_labels={"app": "web"})


def term(*reqs, fields=()):
    return NodeSelectorTerm(list(reqs), list(fields))


def req(k, op, *vals):
    return NodeSelectorRequirement(k, op, list(vals))


def spread(pod, *cs):
    pod.topology_spread = list(cs)
    return pod


def zc(skew=1, sel=WEB, key=Z, when="DoNotSchedule"):
    return TopologySpreadConstraint(skew, key, when, sel)


def rand_volume_scenario(seed):
    """Random clusters whose pods carry claims (CSI / EBS / GCE PD PVs with zone
    labels and node affinity), inline ISCSI / GCE PD / EBS disks, under CSINode
    and Allocatable limits; some claims unbound or waiting for a consumer."""
    r = random.Random(seed)
    nodes, spot_pods, cands = rand_scenario(9500 + seed, n_spot=6 + seed % 14, n_cand=10, max_pods=3 + seed % 6,
                                            features=seed % 3 == 0)
    zones = ["z1", "z2", "z3"]
    for i, n in enumerate(nodes):
        if r.random() < 0.8:
            n.labels[TZ] = r.choice(zones)
        if r.random() < 0.5:
            n.labels[TR] = "r1"
        if r.random() < 0.3:
            n.scalar["attachable-volumes-aws-ebs"] = r.choice([0, 1, 2, 3])
    pvcs, pvs, vid = [], [], [0]

    def new_claim(ns):
        vid[0] += 1
        name = "c%d" % vid[0]
        x = r.random()
        if x < 0.05:
            pvcs.append(PersistentVolumeClaim(name, namespace=ns))
        elif x < 0.1:
            pvcs.append(PersistentVolumeClaim(name, namespace=ns, binding_mode="WaitForFirstConsumer"))
        else:
            kind = r.choice(["csi", "csi", "aws-ebs", "gce-pd", "nfs"])
            labels = {TZ: r.choice(zones + ["z1__z2"])} if r.random() < 0.5 else {}
            terms = None
            if r.random() < 0.3:
                terms = [term(req(TZ, "In", *r.sample(zones, r.choice([1, 2]))))]
                if r.random() < 0.3:
                    terms.append(term(req(TR, "Exists")))
            pvs.append(PersistentVolume("pv" + name, kind=kind, volume_id="v%d" % vid[0], labels=labels,
                                        node_affinity=terms))
            pvcs.append(PersistentVolumeClaim(name, namespace=ns, volume_name="pv" + name))
        return Volume(name=name, claim=name)

    iqns = ["iq1", "iq2", "iq3"]
    for ps in spot_pods + cands:
        for p in ps:
            if r.random() < 0.35:
                p.volumes.append(new_claim(p.namespace))
            if r.random() < 0.15:
                p.volumes.append(Volume(name="isc", iscsi_iqn=r.choice(iqns), read_only=r.random() < 0.5))
            if r.random() < 0.05:
                p.volumes.append(Volume(name="pd", gce_pd="pd%d" % r.randrange(1000), read_only=r.random() < 0.5))
    csi = {n.name: {EBS_CSI: r.choice([1, 2, 4])} for n in nodes if r.random() < 0.6}
    return nodes, spot_pods, cands, VolumeWorld(pvcs=pvcs, pvs=pvs, csi_limits=csi)


def rand_spread_scenario(seed):
    """Random zone / rack clusters with web / api pods in two namespaces,
    some terminating, and spread constraints on a share of the candidate
    pods (several per pod, shared keys, selectors of every operator, nil)."""
    r = random.Random(5150 + seed)
    nodes, spot_pods, cands = rand_scenario(6600 + seed, n_spot=6 + seed % 25, n_cand=12, max_pods=5,
                                            features=False)
    zones = ["z%d" % i for i in range(1 + seed % 4)]
    for i, n in enumerate(nodes):
        n.labels = dict(n.labels)
        n.labels[H] = n.name
        if r.random() < 0.85:
            n.labels[Z] = r.choice(zones + [""] if seed % 5 == 0 else zones)
        if r.random() < 0.5:
            n.labels["example.com/rack"] = "r%d" % r.randrange(3)
    apps = ["web", "api", "db"]
    for ps in spot_pods:
        for p in ps:
            p.namespace = r.choice(["default", "default", "other"])
            p.labels = {"app": r.choice(apps)} if r.random() < 0.9 else {}
            if r.random() < 0.1:
                p.deletion_age_s = 3.0

    def rand_sel():
        x = r.random()
        if x < 0.1:
            return None
        if x < 0.6:
            return LabelSelector(match_labels={"app": r.choice(apps)})
        op = r.choice(["In", "NotIn", "Exists", "DoesNotExist"])
        vals = r.sample(apps, r.randint(1, 2)) if op in ("In", "NotIn") else []
        return LabelSelector(match_expressions=[LabelSelectorRequirement("app", op, vals)])

    for c in cands:
        for p in c:
            p.namespace = "default" if r.random() < 0.8 else "other"
            p.labels = {"app": r.choice(apps)}
            if r.random() < 0.5:
                p.topology_spread = [zc(skew=r.choice([1, 1, 2]), sel=rand_sel(),
                                        key=r.choice([Z, Z, H, "example.com/rack"]))
                                     for _ in range(r.choice([1, 1, 2]))]
                if r.random() < 0.2:
                    p.node_selector = {Z: r.choice(zones)}
    return nodes, spot_pods, cands


def rand_spread_replicas(seed):
    """Large candidates of Deployment replicas spread over zones (65-230 pods
    per candidate: 2-4 pod groups of the domain path), with a hostname
    constraint on some, over pools whose nodes already run replicas."""
    r = random.Random(8080 + seed)
    zones = ["z%d" % i for i in range(2 + seed % 4)]
    n_spot = 30 + seed % 40
    nodes = [Node("s%d" % i, cpu_milli=64000, memory=256 * 2 ** 30, pods=110,
                  labels={Z: r.choice(zones), H: "s%d" % i}) for i in range(n_spot)]
    apps = ["web", "api"]
    spot_pods = [[Pod("b%d_%d" % (i, j), namespace="default", containers=[Container(cpu_milli=r.choice([100, 250]))],
                      labels={"app": r.choice(apps)}) for j in range(r.randrange(4))] for i in range(n_spot)]
    cands = []
    for ci in range(3):
        n = 65 + r.randrange(166)
        app = r.choice(apps)
        cs = [zc(skew=r.choice([1, 2, 3]), sel=LabelSelector(match_labels={"app": app}))]
        if r.random() < 0.3:
            cs.append(zc(skew=r.choice([2, 4]), sel=LabelSelector(match_labels={"app": app}), key=H))
        cands.append([spread(Pod("c%d_%d" % (ci, j), namespace="default",
                                 containers=[Container(cpu_milli=r.choice([50, 100, 250, 500]))],
                                 labels={"app": app}), *cs) for j in range(n)])
    return nodes, spot_pods, cands


def init_and_gpu_scenario(seed):
    """Random clusters where most pods carry init containers (fit request !=
    AddPod accounting) and most candidates list one GPU name in several pods
    (a running scalar state per touched node), some hugepages too."""
    nodes, spot_pods, cands = rand_scenario(9100 + seed, n_spot=6 + seed % 20, n_cand=12, max_pods=4 + seed % 12,
                                            features=seed % 2 == 0)
    r = random.Random(seed)
    for n in nodes:
        if r.random() < 0.8:
            n.scalar = {G: r.choice([0, 1, 2, 4, 8]), "hugepages-2Mi": r.choice([0, 8 << 20])}
    for c in cands:
        gpu_cand = r.random() < 0.7
        for p in c:
            if r.random() < 0.5:
                p.init_containers = [Container(cpu_milli=r.choice([200, 1500, 3000]),
                                               memory=r.choice([0, 1 * GiB, 6 * GiB]),
                                               scalar={G: r.choice([1, 2])} if gpu_cand and r.random() < 0.3 else {})]
            if gpu_cand and r.random() < 0.6:
                p.containers[0].scalar = {G: r.choice([0, 1, 1, 2])}
                if r.random() < 0.2:
                    p.containers[0].scalar["hugepages-2Mi"] = r.choice([2 << 20, 4 << 20])
                if p.containers[0].cpu_milli == 0:
                    p.containers[0].cpu_milli = 10
    return nodes, spot_pods, cands
