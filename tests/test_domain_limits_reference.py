"""What test_gpu_domain_limits.py rests on, asserted on the CPU oracle: the
hand-derived plans of domain_limits.py, and the preconditions that make each
case decisive -- every deciding pod has another open node that a dropped
refusal, a dropped requirement or a wrong minimum would choose, every limit
case is at the limit and one over it (values, keys, terms and constraints are
counted here), and no case that claims a high domain id is decided below id 31.
A change to a generator that empties one of those cases fails here, without a
GPU."""
import numpy as np
import pytest

import domain_limits as D
from domain_cases import H
from oracle_lib import load_oracle, oracle_plan
from randcluster import aff_interacts, anti_interacts_off_node
from sequence_ref import FB, OK
from spotplanner import capi

IDS = ["%s-%s" % pc for pc in D.CALLS]


def check_hand_answers(o, cands, cand_off, changed=None):
    """The plan `o` against every candidate's written-out answer."""
    for c, cd in enumerate(cands):
        want, fail = cd.want, cd.fail
        if changed and cd.name in changed:
            want, fail = changed[cd.name]
        if want is None:
            continue
        assert int(o["status"][c]) == (OK if fail < 0 else fail), (cd.name, cd.why, o["status"][c])
        got = [int(x) for x in o["node_of_pod"][cand_off[c]:cand_off[c + 1]]]
        assert got == want, (cd.name, cd.why, [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w][:6])


@pytest.mark.parametrize("pool,call", D.CALLS, ids=IDS)
def test_oracle_gives_the_hand_answers(pool, call):
    P = D.get_pool(pool)
    cand_off, _ = P.arrays(call)
    o = P.oracle(call)
    # the oracle plans every candidate, also beyond the planner's limits, except beyond the spread limits it mirrors
    assert [int(x) == FB for x in o["status"]] == [cd.oracle_too for cd in P.calls[call].cands]
    check_hand_answers(o, P.calls[call].cands, cand_off)


@pytest.mark.parametrize("pool,call", D.CALLS, ids=IDS)
def test_cases_are_decisive(pool, call):
    P = D.get_pool(pool)
    open_nodes = set(P.open_nodes())
    for cd in P.calls[call].cands:
        assert cd.want is None or len(cd.want) == len(cd.pods)
        if cd.fail >= 0 and cd.want is not None:
            assert all(x == -1 for x in cd.want[cd.fail:]) and all(x >= 0 for x in cd.want[:cd.fail])
        for k, (alt, dom) in cd.decided.items():
            # another open node, which the pod takes as soon as what decides it is dropped
            assert alt in open_nodes and alt != cd.want[k], (cd.name, k)
            if cd.high:
                assert dom is not None and dom >= 31, (cd.name, k, dom)
        assert not cd.high or cd.decided


def test_z64_pool_shape():
    P = D.get_pool("z64")
    assert len(P.nodes) == 192 and -(-len(P.nodes) // 64) == 3  # three row words
    assert P.n_values(D.Z) == 64 and all(P.domain_id(D.Z, n) == n // 3 for n in range(192))
    assert P.domain_id(D.Z, 63) == P.domain_id(D.Z, 64) == 21  # zone 21 spans the 63 | 64 word boundary
    assert P.n_values(H) == 192  # node-local
    assert [P.n_values(k) for k in (D.RACK, D.TEAM, D.REGION, D.CELL)] == [2, 3, 2, 5]
    open_nodes = P.open_nodes()
    for z in range(64):
        mine = [n for n in open_nodes if n // 3 == z]
        assert len(mine) >= 2 and mine[0] == D.fo(z)
    assert [z for z in range(64) if D.fo(z) != 3 * z] == list(range(1, 64, 5))
    # the spread counts: one web pod per zone, none in zones 40 and 63
    web = [sum(1 for n in range(3 * z, 3 * z + 3) for p in P.base[n] if p.labels["app"] == "web") for z in range(64)]
    assert web == [0 if z in D.NO_WEB else 1 for z in range(64)]


def test_variant_pools_are_at_and_over_the_value_limit():
    assert D.get_pool("z65").n_values(D.Z) == 65 and len(D.get_pool("z65").nodes) == 193
    k = D.get_pool("z63k")
    assert k.n_values(D.Z) == 63 and [n for n, x in enumerate(k.nodes) if D.Z not in x.labels] == [189, 190, 191]
    e = D.get_pool("z63e")
    assert e.n_values(D.Z) == 64 and e.nodes[189].labels[D.Z] == "" and e.domain_id(D.Z, 189) == 63
    assert [n for n, x in enumerate(e.nodes) if D.Z not in x.labels] == [190, 191]
    assert [p.labels["app"] for p in e.base[191]] == ["web"] and not e.base[189]


def _anti_keys(cd):
    return {t.topology_key for p in cd.pods for t in p.pod_anti_affinity or []}


def _aff_keys(cd):
    return {t.topology_key for p in cd.pods for t in p.pod_affinity or []}


def test_value_limit_cases():
    """On 64 values nothing falls back; on 65 exactly the candidates whose pods interact through the zone key."""
    at, over = D.get_pool("z64").calls["values"].cands, D.get_pool("z65").calls["values"].cands
    assert [c.name for c in at[:-1]] == [c.name for c in over[:-1]] and not any(c.fallback for c in at)
    assert [c.name for c in over if c.fallback] == ["anti_zone", "follow_zone", "spread_zone"]
    nodes = D.get_pool("z65").nodes
    by = {c.name: c for c in over}
    assert anti_interacts_off_node(nodes, by["anti_zone"].pods) and aff_interacts(by["follow_zone"].pods)
    assert anti_interacts_off_node(nodes, by["anti_team"].pods) and _anti_keys(by["anti_team"]) == {D.TEAM}
    for name in ("static_one", "static_two"):  # zone terms against base pods only: nothing inside the candidate
        assert _anti_keys(by[name]) == {D.Z} and not anti_interacts_off_node(nodes, by[name].pods)


def test_key_slot_cases():
    calls = D.get_pool("z64").calls
    nodes = D.get_pool("z64").nodes

    def keys_in_order(call):  # anti-affinity first, then affinity: the order the encoder takes slots in
        out = []
        for keys_of in (_anti_keys, _aff_keys):
            for cd in calls[call].cands:
                for k in sorted(keys_of(cd)):
                    if k not in out and len(keys_of(cd)) == 1:
                        out.append(k)
        return out

    fwd = keys_in_order("keys_forward")
    assert fwd == [D.Z, D.RACK, D.TEAM, D.REGION, D.CELL]
    assert [c.name for c in calls["keys_forward"].cands if c.fallback] == ["anti_" + fwd[4]]
    all4 = next(c for c in calls["keys_forward"].cands if c.name == "anti_all_four")
    assert sorted(_anti_keys(all4)) == sorted(fwd[:4]) and len(all4.pods[-1].pod_anti_affinity) == 4
    assert all4.want[-1] == 97 and all4.decided[D.N_PRE + 1][0] == 5  # slot 3 (region) decides: 97, not 5
    rev = keys_in_order("keys_reverse")
    assert rev == [D.CELL, D.REGION, D.TEAM, D.RACK, D.Z]
    assert [c.name for c in calls["keys_reverse"].cands if c.fallback] == ["anti_" + rev[4], "anti_all_four"]
    assert keys_in_order("keys_hostname_fourth") == [D.Z, D.RACK, D.TEAM, H]
    assert not any(c.fallback for c in calls["keys_hostname_fourth"].cands)
    assert keys_in_order("keys_hostname_fifth") == [D.Z, D.RACK, D.TEAM, H, D.REGION]
    assert [c.name for c in calls["keys_hostname_fifth"].cands if c.fallback] == ["aff_region"]
    for name in ("keys_four_a", "keys_four_b"):
        assert len(keys_in_order(name)) == 4 and not any(c.fallback for c in calls[name].cands)
    assert set(keys_in_order("keys_four_a")) != set(keys_in_order("keys_four_b"))
    for call in calls.values():  # every key candidate's pods interact, the neighbours do not
        for cd in call.cands:
            if cd.name.startswith("anti_") and call.name.startswith("keys"):
                assert anti_interacts_off_node(nodes, cd.pods), cd.name
            if cd.name.startswith("plain"):
                assert not _anti_keys(cd) and not _aff_keys(cd) and not cd.fallback


def test_term_and_constraint_limit_cases():
    calls = D.get_pool("z64").calls
    by = {c.name: c for c in calls["terms"].cands}
    assert len(by["aff_four_terms"].pods[-1].pod_affinity) == 4 and not by["aff_four_terms"].fallback
    assert len(by["aff_five_terms"].pods[-1].pod_affinity) == 5 and by["aff_five_terms"].fallback
    assert len(_aff_keys(by["aff_four_terms"])) == 4 and H in _aff_keys(by["aff_four_terms"])
    assert aff_interacts(by["aff_four_terms"].pods) and aff_interacts(by["aff_five_terms"].pods)
    main = {c.name: c for c in calls["main"].cands}
    assert len(main["spread_zone_and_host"].pods[-1].topology_spread) == 2 and not main["spread_zone_and_host"].fallback
    assert len(main["spread_three_constraints"].pods[-1].topology_spread) == 3
    assert [c.name for c in calls["main"].cands if c.fallback] == ["spread_three_constraints"]
    # pod groups: one (<= 64 pods) and two (65..128) in the main call
    sizes = {c.name: len(c.pods) for c in calls["main"].cands}
    assert sizes["anti64_one_group"] == 64 and 64 < sizes["anti64"] <= 128 and 64 < sizes["spread_skew1"] <= 128
    # the pairs of spread_pairs_32_up: no domain id below 32
    P = D.get_pool("z64")
    pairs = {P.domain_id(D.Z, n) for n, x in enumerate(P.nodes) if x.labels[D.REGION] == "g1"}
    assert min(pairs) == 32 and max(pairs) == 63


@pytest.mark.parametrize("name", sorted(D.WIDE))
def test_wide_pool_shape(name):
    P = D.get_pool(name)
    n = D.WIDE[name]
    op = D.wide_open(n)
    assert len(P.nodes) == n and -(-n // 64) == {"wide2": 68, "wide3": 130}[name]
    assert P.open_nodes() == sorted(op)
    # 62 / 63 | 64 / 65, 4,094 / 4,095 | 4,096 / 4,097, 8,190 / 8,191 | 8,192 / 8,193 and the last two
    want = [62, 63, 64, 65, 4094, 4095, 4096, 4097] + ([8190, 8191, 8192, 8193] if n > 8200 else []) + [n - 2, n - 1]
    assert sorted(op) == want
    closed = [x for i, x in enumerate(P.nodes) if i not in op]
    s_rows, t_rows = sum(x.unschedulable for x in closed), sum(not x.unschedulable and x.cpu_milli < 10 for x in closed)
    assert s_rows + t_rows == len(closed) and abs(s_rows - t_rows) <= 16
    assert P.n_values(H) == n and P.n_values(D.Z) == 4
    # each zone's open nodes lie in different chunks; zd's only one is in the last chunk
    chunks = {}
    for i in op:
        chunks.setdefault(op[i]["zone"], set()).add(i // 4096)
    assert chunks["zd"] == {(n - 1) // 4096}
    if n > 8200:
        assert chunks["za"] == {0, 1} and chunks[None] == {1, 2} and chunks["zb"] == chunks["zc"] == {1}
        assert [P.domain_id(D.Z, i) for i in (62, 4097, 8191, 8298)] == [0, 1, 2, 3]
    else:
        assert chunks["za"] == {0, 1} and [P.domain_id(D.Z, i) for i in (62, 4097, 4299)] == [0, 1, 3]


def test_wide3_deciding_nodes_lie_beyond_the_first_chunk():
    by = {c.name: c for c in D.get_pool("wide3").calls["main"].cands}
    a = by["anti_chunks"]
    assert a.want[D.N_PRE] < 4096 < a.want[D.N_PRE + 1] < 8192 and a.decided[D.N_PRE + 1][0] < 4096
    assert 4096 <= a.want[D.N_PRE + 2] == a.want[D.N_PRE + 3] < 8192  # two pods share a key-less node in chunk 1
    assert 8192 <= a.want[D.N_PRE + 5] == a.want[D.N_PRE + 6]  # ... and one in chunk 2
    assert a.fail == len(a.pods) - 1
    assert [k for k, p in enumerate(a.pods) if p.containers[0].ports] == [D.N_PRE + i for i in (7, 8, 10, 11)]
    h = by["spread_hostname"]
    assert (h.want[D.N_PRE + 1], h.decided[D.N_PRE + 1][0]) == (4097, 4096)  # word 64: chunk 1, lane 0
    assert (h.want[D.N_PRE + 3], h.decided[D.N_PRE + 3][0]) == (8193, 8192)  # word 128: chunk 2, lane 0
    # node-local spread stays on the device while more pairs hold the minimum than the constraint counts pods
    assert len(h.pods) - D.N_PRE - 1 < 6 == len(h.pods[-1].required_node_affinity[0].match_expressions[0].values)
    assert by["aff_hostname_4097"].want[-1] == 4097 and by["aff_hostname_8193"].want[-1] == 8193
    assert by["spread_zone_last_chunk"].want[D.N_PRE + 3] == 8298 and by["aff_zone_last_chunk"].want[-1] == 8298


def oracle_with_filler(P, call):
    """The call planned from the base snapshot plus the filler pod on CHANGED_NODE."""
    cand_off, cand_pods = P.arrays(call)
    osnap = P.sc.oracle_snapshot()
    filler = P.calls["filler"].cands[0].pods[0]
    load_oracle().oracle_snapshot_add_pod(osnap.h, P.sc.ptr, P.pod_index(filler), D.CHANGED_NODE)
    return oracle_plan(osnap, P.sc.ptr, cand_off, cand_pods, mode=1)


@pytest.mark.parametrize("call", ["without", "with"])
def test_wide2_changed_node_changes_the_plan(call):
    P = D.get_pool("wide2")
    cand_off, _ = P.arrays(call)
    o = oracle_with_filler(P, call)
    check_hand_answers(o, P.calls[call].cands, cand_off, changed=D.CHANGED)
    base = P.oracle(call)
    assert not np.array_equal(o["node_of_pod"], base["node_of_pod"]) and not np.array_equal(o["status"], base["status"])
    dom = [c for c in P.calls[call].cands if anti_interacts_off_node(P.nodes, c.pods)]
    assert len(dom) == (1 if call == "with" else 0)


@pytest.mark.parametrize("name", sorted(D.sequence_cases()))
def test_sequence_cases(name):
    case, inp = D.get_sequence(name)
    ref, _ = inp.reference()
    assert list(ref.drained) == case.drained and (ref.stop, ref.stop_cand) == (capi.SR_SEQ_END, -1)
    check_hand_answers(dict(status=ref.status, node_of_pod=ref.node_of_pod), case.cands, inp.cand_off)
    kinds = [anti_interacts_off_node(D.get_pool("wide2").nodes, c.pods) for c in case.cands]
    first_domain = kinds.index(True)
    assert (first_domain == 0) == (name == "domain_first") and kinds.count(True) == 1
    # the later drain's mapping differs from the one it has from the base snapshot
    base = inp.base_plan()
    later = case.drained[1] if name == "node_order_first" else 1
    seg = slice(inp.cand_off[later], inp.cand_off[later + 1])
    assert not np.array_equal(base["node_of_pod"][seg], ref.node_of_pod[seg])
