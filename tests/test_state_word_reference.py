"""The state-word cases of state_word.py proved without a GPU: the oracle (the
plain HostPortInfo / InterPodAffinity restatement: it has no state word)
reproduces every hand-derived plan and puts b on node 0 in every twin, so the
bit is what decides; and the encoder's host view (lib/libsrstateview.so,
tools/state_word_view.cpp) gives every pod exactly the bits, the swap_mask and
the fallback set of the Python layout rule, with the deciding bits at the
positions each case names.  test_gpu_state_word.py runs the same calls through
the planner."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import state_word as S
from sequence_ref import from_scenario
from spotplanner import capi

VIEW_LIB = os.path.join(capi.LIB_DIR, "libsrstateview.so")
_view = None


def load_view():
    global _view
    if _view is None:
        if not os.path.exists(VIEW_LIB):  # host only: builds without a GPU, like the oracle
            subprocess.run(["make", "-C", capi.PKG_ROOT, "lib/libsrstateview.so"], check=True, capture_output=True)
        lib = ctypes.CDLL(VIEW_LIB)
        PC, VP = ctypes.POINTER(capi.sr_cluster), ctypes.c_void_p
        lib.sr_snapshot_create.argtypes = [PC, capi.P32, ctypes.c_int32, capi.P32, capi.P32, ctypes.POINTER(VP)]
        lib.sr_snapshot_create.restype = ctypes.c_int32
        lib.sr_snapshot_destroy.argtypes = [VP]
        lib.sr_snapshot_destroy.restype = None
        lib.sr_snapshot_add_pod.argtypes = [VP, PC, ctypes.c_int32, ctypes.c_int32]
        lib.sr_snapshot_add_pod.restype = ctypes.c_int32
        lib.sr_state_word_view.argtypes = [PC, VP, ctypes.POINTER(capi.sr_candidates), ctypes.POINTER(ctypes.c_uint64),
                                           capi.P32, ctypes.POINTER(ctypes.c_uint64), capi.P32, ctypes.c_int32,
                                           capi.P32]
        lib.sr_state_word_view.restype = ctypes.c_int32
        _view = lib
    return _view


def view(inp, drop=(), fillers=()):
    """(swap_mask, host status per candidate, per candidate the mask of every pod or None when not active)."""
    lib = load_view()
    sc = inp.sc
    cands, pods, cand_off, cand_pods = inp.arrays(drop)
    h = ctypes.c_void_p()
    assert lib.sr_snapshot_create(sc.ptr, capi.ptr(sc.spot, capi.P32), len(sc.spot), capi.ptr(sc.node_pod_off, capi.P32),
                                  capi.ptr(sc.node_pod_idx, capi.P32), ctypes.byref(h)) == capi.SR_OK
    try:
        for pod, pos in fillers:
            assert lib.sr_snapshot_add_pod(h, sc.ptr, pod, pos) == capi.SR_OK
        n, n_pods = len(cand_off) - 1, int(cand_off[-1])
        c = capi.sr_candidates(n, capi.ptr(cand_off, capi.P32), capi.ptr(cand_pods, capi.P32), None)
        swap, n_active = ctypes.c_uint64(), ctypes.c_int32()
        status, src = np.zeros(n, np.int32), np.zeros(n_pods, np.int32)
        bits = np.zeros(n_pods, np.uint64)
        st = lib.sr_state_word_view(sc.ptr, h, ctypes.byref(c), ctypes.byref(swap), capi.ptr(status, capi.P32),
                                    bits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), capi.ptr(src, capi.P32),
                                    n_pods, ctypes.byref(n_active))
        assert st == capi.SR_OK
    finally:
        lib.sr_snapshot_destroy(h)
    flat = [None] * n_pods
    for q in range(n_active.value):
        assert flat[src[q]] is None
        flat[src[q]] = int(bits[q])
    return int(swap.value), [int(s) for s in status], [flat[cand_off[i]:cand_off[i + 1]] for i in range(n)]


def positions(mask):
    return [b for b in range(64) if mask >> b & 1]


def check_plan(o, cands, cand_off, want=None):
    """The oracle's answer for every candidate the case plans (it also plans the ones the planner hands back)."""
    status, nodes, _, _, _, _ = S.expected(cands, want)
    for i, cd in enumerate(cands):
        if cd.status == S.FB:
            continue
        seg = slice(int(cand_off[i]), int(cand_off[i + 1]))
        assert int(o["status"][i]) == cd.status, (cd.name, int(o["status"][i]))
        assert list(o["node_of_pod"][seg]) == list(nodes[seg]), (cd.name, list(o["node_of_pod"][seg]))


def check_view(got, cands, pods, bits=None, swap_mask=None):
    swap, status, masks = got
    want_masks, want_swap, want_fb = S.layout(pods)
    assert swap == want_swap, (hex(swap), hex(want_swap))
    if swap_mask is not None:
        assert swap == swap_mask, (hex(swap), hex(swap_mask))
    assert {i for i, s in enumerate(status) if s == S.FB} == want_fb == {i for i, cd in enumerate(cands)
                                                                        if cd.status == S.FB}
    for i, cd in enumerate(cands):
        if cd.status == S.FB:
            assert masks[i] == [None] * len(cd.pods), cd.name
            continue
        assert masks[i] == want_masks[i], (cd.name, [positions(m) for m in masks[i]],
                                          [positions(m) for m in want_masks[i]])
        for k, pos in (bits[cd.name] if bits is not None and cd.name in bits else cd.bits).items():
            assert positions(masks[i][k]) == sorted(pos), (cd.name, k, positions(masks[i][k]), pos)
    used = 0
    for ms in masks:
        for m in ms:
            used |= m or 0
    return used


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_oracle_reproduces_the_hand_plan(name):
    inp = S.get_input(name)
    check_plan(inp.oracle(), inp.cands, inp.cand_off)


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_twin_shares_node_0(name):
    """Without the deciding port, disk, term or base pod the second pod joins the first: the bit decides."""
    case = S.CASES[name]
    if not any(cd.twin_want is not None for cd in case.cands):
        # the cases without a twin are the ones whose pods share a node, and the limits
        assert name.startswith(("ip_two", "ip_proto", "disk_62_ro_ro", "limit_65", "anti33", "anti32_and_port")), name
        return
    inp = S.get_input(name, twin=True)
    o = inp.oracle()
    for i, cd in enumerate(inp.cands):
        if cd.twin_want is None or cd.status == S.FB:
            continue
        seg = slice(int(inp.cand_off[i]), int(inp.cand_off[i + 1]))
        assert int(o["status"][i]) == S.OK and list(o["node_of_pod"][seg]) == cd.twin_want, (
            cd.name, list(o["node_of_pod"][seg]))
        assert cd.twin_want != cd.want


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_view_equals_the_layout_rule(name):
    inp = S.get_input(name)
    used = check_view(view(inp), inp.cands, inp.pods, swap_mask=S.CASES[name].swap_mask)
    decided = [b for cd in inp.cands for pos in cd.bits.values() for b in pos]
    assert all(used >> b & 1 for b in decided)


def test_the_cases_reach_the_high_bits():
    """Every family decides at bit 32 or above, bit 63 in particular, and the calls that fill the word fill it."""
    top = {}
    for name, case in S.CASES.items():
        top[name] = max([b for cd in case.cands for pos in cd.bits.values() for b in pos] + [-1])
    for prefix in ("singles_", "ip_same_63", "ip_two_63", "ip_proto_63", "pairs_30_32", "disk_62", "anti32_", "mixed",
                   "limit_64", "limit_reuse", "limit_middle", "base_", "form_", "ticks"):
        names = [n for n in top if n.startswith(prefix)]
        assert names and all(top[n] >= 33 for n in names), (prefix, names)
        assert prefix == "pairs_30_32" or any(top[n] == 63 for n in names), prefix  # (pair 16 tops at I(ip), 35)
    for name in ("singles_excl", "singles_mid", "singles_low", "limit_64", "mixed", "anti32_has_second"):
        inp = S.get_input(name)
        assert check_view(view(inp), inp.cands, inp.pods) == S.FULL, name


def test_ticks_script():
    inp = S.get_input("ticks")
    for drop, filler, nodes, bits, swap_mask in S.TICKS:
        fillers = ((inp.extra_pod[0], S.TICK_FILLER_NODE),) if filler else ()
        cands, pods, cand_off, _ = inp.arrays(drop)
        check_plan(inp.oracle(drop, fillers), cands, cand_off, want={"probe_tick": nodes})
        check_view(view(inp, drop, fillers), cands, pods, bits={"probe_tick": bits}, swap_mask=swap_mask)


def test_sequence_reference():
    nodes, base, cands, want, drained = S.sequence_case()
    ref, _ = from_scenario(nodes, base, cands).reference()
    assert list(ref.drained) == drained
    assert list(ref.node_of_pod) == want
