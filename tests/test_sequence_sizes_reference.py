"""What test_gpu_sequence_sizes.py rests on, asserted on the CPU oracle: the
inputs of sequence_sizes.py reach past every stride of the ledger kernels and
into every K2 path of a large candidate.  A change to a generator that empties
one of those cases fails here, without a GPU."""
import numpy as np
import pytest

from randcluster import anti_interacts_off_node
from sequence_pdb_ref import PDB, pdb_facts, pdb_reference
from sequence_ref import FB, OK, divergence
from sequence_sizes import (DOMAIN_SIZES, EMPTIES, FALLBACK_AT, KINDS, LADDERS, PLAIN_FAILING, SPREAD_SIZES,
                            big_and_later, distinct_nodes, get_ladder, ladder_limits, large_drains, large_objects,
                            many_needs, masking_large, sliced)
from spotplanner import capi


@pytest.mark.parametrize("name", sorted(LADDERS))
def test_ladders(name):
    lad = get_ladder(name)
    inp = lad.inp
    n = len(inp.cand_off) - 1
    empties = [g for g in EMPTIES if g < n]
    assert n == LADDERS[name]["n"] and len(lad.active) == n - len(empties) and len(empties) >= 2
    assert all(inp.cand_off[g] == inp.cand_off[g + 1] for g in empties)
    assert lad.wins[-1] == len(lad.active) - 1  # the last active candidate
    assert not set(lad.twins) & set(lad.wins) and all(t + 1 in lad.wins for t in lad.twins)
    # pod offsets apart from candidate indices, the active index apart from the caller's above the first empty
    assert inp.cand_off[-1] > n
    for a in lad.wins:
        assert (lad.active[a] != a) == (lad.active[a] > min(EMPTIES))
    assert sum(lad.active[a] != a for a in lad.wins) >= len(lad.wins) - 3
    plain, _ = inp.reference()
    assert list(plain.drained) == lad.caller(sorted(lad.wins + lad.twins))
    assert (plain.stop, plain.stop_cand) == (capi.SR_SEQ_END, -1) and not np.any(plain.status == FB)
    allowed, pod_group = ladder_limits(lad)
    lim, _ = pdb_reference(inp, "ladder", allowed, pod_group, probe=True)
    assert list(lim.drained) == lad.caller(lad.wins)
    assert list(np.nonzero(lim.status == PDB)[0]) == lad.caller(lad.twins)
    assert all(lim.would[c] == OK for c in lad.caller(lad.twins))  # drainable where the pass met them ...
    assert pdb_facts(inp, allowed, pod_group)[:2] == (len(lad.twins), len(lad.twins))  # ... below a later drain
    assert list(lim.remaining) == [0, 0, 0, 0] and allowed[0] == 0 and np.all(allowed[1:] > 0)
    off = inp.cand_off - inp.cand_off[0]
    for a in lad.twins:  # directly below its winner
        assert lad.active[a + 1] == lad.active[a] + 1 and pod_group[off[lad.active[a] + 1] - 1] == 0


def test_ladders_reach_the_strides_and_the_default_dispatch():
    big, dom = get_ladder("ladder-17k"), get_ladder("ladder-4200-domain")
    for lad in (big, dom):
        assert any(63 <= a < 64 for a in lad.wins) and any(64 <= a < 1024 for a in lad.wins)
        assert any(1024 <= a < 16384 for a in lad.wins)  # k3_pdb_winner's second step
    assert any(a >= 16384 for a in big.wins)  # the ledger kernels' second step
    assert {16383, 16384}.issubset(big.wins) and {1023, 1024}.issubset(big.wins)
    # default dispatch: cost-ordered above 1,024 entries, four waves per block above 2,048, split above 4,096
    assert len(dom.active) > 4096 and len(big.active) > 16384
    assert len(dom.domain) >= 10
    small = set(dom.caller(dom.wins + dom.twins))
    for g in dom.domain:
        assert anti_interacts_off_node(dom.nodes, dom.cands[g]) and g not in small and len(dom.cands[g]) == 2
    assert not big.domain


def test_ladder_with_a_fallback_candidate():
    lad = get_ladder("ladder-17k-fallback")
    fb = int(lad.active[FALLBACK_AT])
    assert FALLBACK_AT > 16384 and lad.wins[-1] < FALLBACK_AT - 1
    plain, _ = lad.inp.reference()
    assert (plain.stop, plain.stop_cand) == (capi.SR_SEQ_FALLBACK, fb) and plain.status[fb] == FB
    last = int(plain.drained[-1])
    assert fb - last > 100 and np.all(plain.status[last + 1:fb] >= 0)  # failed candidates in between
    allowed, pod_group = ladder_limits(lad, also_refused=[FALLBACK_AT])
    lim, _ = pdb_reference(lad.inp, "ladder-fb", allowed, pod_group, probe=True)
    assert lim.status[fb] == PDB and lim.would[fb] == FB
    assert (lim.stop, lim.stop_cand) == (capi.SR_SEQ_END, -1) and list(lim.drained) == lad.caller(lad.wins)
    assert np.all(lim.status[fb + 1:] >= 0)


def _bucket(m):
    return 0 if m <= 64 else 1 if m <= 128 else 2 if m <= 256 else 3


@pytest.mark.parametrize("kind", KINDS)
def test_large_drains(kind):
    inp = large_drains(kind)
    ref, _ = inp.reference()
    sizes = np.diff(inp.cand_off)
    drained = [int(sizes[c]) for c in ref.drained]
    assert not np.any(inp.base_plan()["status"] == FB) and not np.any(ref.status == FB)
    assert ref.stop == capi.SR_SEQ_END
    if kind == "spread-out":
        assert drained == SPREAD_SIZES
        assert [distinct_nodes(inp, ref, c) for c in ref.drained] == SPREAD_SIZES  # 64 | 65, 128 | 129 and beyond
    else:
        # two, four and eight pod groups, and the largest candidate K2 plans
        assert {1, 2, 3}.issubset(_bucket(m) for m in drained) and 512 in drained
    assert divergence(inp, ref)[1] >= 3  # mappings an earlier drain changed
    if kind in ("plain", "ext"):
        for c in PLAIN_FAILING:
            assert ref.status[c] == sizes[c] - 1
        assert len(ref.drained) == len(sizes) - 1 - len(PLAIN_FAILING)
        big, _ = big_and_later(inp)
        assert distinct_nodes(inp, ref, big) > 64 and sizes[big] > 256  # pod order's second attempt
        assert sum(distinct_nodes(inp, ref, c) for c in ref.drained) > 100  # nodes the commits touched
    if kind == "domain":
        nodes, _, cands = large_objects(kind)
        assert len(nodes) == 72 and len({n.labels.get("zone") for n in nodes}) == 9  # 8 zones and "none"
        assert drained[:-1] == [m + 1 for m in DOMAIN_SIZES] and len(ref.drained) == len(sizes)
        assert all(anti_interacts_off_node(nodes, c) for c in cands[:-1])
        assert divergence(inp, ref)[1] >= 7
    if kind == "ext":
        _, _, cands = large_objects(kind)
        for c in ref.drained[:-1]:
            pods = cands[c]
            assert sum(1 for p in pods[:-1] if p.init_containers) >= 10  # accounting below the fit request
            assert sum(1 for p in pods if p.scalar_request()) >= 2  # two pods list one scalar name


@pytest.mark.parametrize("kind", ["plain", "domain"])
def test_many_needs(kind):
    inp = large_drains(kind)
    sizes = np.diff(inp.cand_off)
    big, other = big_and_later(inp)
    m = int(sizes[big])
    assert m == 512 and sizes[other] >= 64
    # accepted at equality: 512 needs committed, every one of its groups left at 0
    allowed, pod_group = many_needs(inp)
    ref, _ = pdb_reference(inp, ("needs", False), allowed, pod_group, probe=True)
    assert len(allowed) == m + 1 and ref.status[big] == OK and np.all(ref.remaining[1:] == 0)
    if other > big:  # refused behind it by needs that are not its first, with an unrefused drain behind
        assert ref.status[other] == PDB and ref.would[other] == OK and ref.remaining[0] == 1
        assert ref.drained[-1] > other
        off = inp.cand_off - inp.cand_off[0]
        assert pod_group[off[other]] == 0 and np.all(pod_group[off[other] + 1:off[other + 1]] > 1)
    else:  # drains in front of it through the shared groups
        assert ref.status[other] == OK and not np.any(ref.status == PDB)
    # refused by its last need only, drainable, below a later drain
    allowed, pod_group = many_needs(inp, refuse_last=True)
    ref, _ = pdb_reference(inp, ("needs", True), allowed, pod_group, probe=True)
    assert list(np.nonzero(allowed == 0)[0]) == [m] and list(np.nonzero(ref.status == PDB)[0]) == [big]
    assert ref.would[big] == OK and ref.drained[-1] > big
    assert pdb_facts(inp, allowed, pod_group)[:2] == (1, 1)


@pytest.mark.parametrize("kind", ["plain", "domain"])
def test_masking_large(kind):
    """A refused candidate of more than 128 pods, drainable, directly below a winner of more than 128 pods."""
    inp = large_drains(kind)
    sizes = np.diff(inp.cand_off)
    c, allowed, pod_group = masking_large(inp, inp.reference()[0])
    ref, _ = pdb_reference(inp, "masking-large", allowed, pod_group, probe=True)
    assert ref.status[c] == PDB and ref.would[c] == OK and sizes[c] > 128
    w = int(ref.drained[list(ref.drained > c).index(True)])
    assert sizes[w] > 128 and np.all(ref.status[c + 1:w] != OK)


def test_sliced_list_is_the_same_list():
    inp = large_drains("plain")
    s = sliced(inp)
    assert s.cand_off[0] == 37 and np.array_equal(np.diff(s.cand_off), np.diff(inp.cand_off))
    assert np.array_equal(s.cand_pods[37:], inp.cand_pods) and set(s.cand_pods[:37]) <= set(inp.cand_pods)
    a, b = s.reference()[0], inp.reference()[0]
    assert np.array_equal(a.status, b.status) and np.array_equal(a.node_of_pod, b.node_of_pod)
