"""Lifetime of the numpy arrays behind sr_candidates / sr_plan_out.

The binding's callers (plan_arrays, the tests, the bench) fill both structs
from `capi.ptr(array, type)` and often keep no other reference to the array:
the struct is then the only thing between the array and the collector while
the library reads candidates from it and writes results into it.  A struct
that holds only the address lets the array go under a live struct ("cand_global
holds a negative index" was such an array, freed and reused).  Checked here
without a GPU: the arrays live exactly as long as the struct that points to
them, a reassigned field releases the old array and holds the new one, and
the ctypes layout (the C ABI) is what include/sr_planner.h declares."""
import ctypes
import gc
import weakref

import numpy as np

from spotplanner import capi


def _candidates_from_temporaries():
    """As plan_arrays and the tests build it: pointers as constructor arguments."""
    off = np.array([0, 2, 3, 6], np.int32)
    pods = np.array([10, 11, 12, 13, 14, 15], np.int32)
    glob = np.array([1, 3, 5], np.int32)
    refs = [weakref.ref(a) for a in (off, pods, glob)]
    c = capi.sr_candidates(3, capi.ptr(off, capi.P32), capi.ptr(pods, capi.P32), capi.ptr(glob, capi.P32))
    return c, refs


def _plan_out_from_temporaries():
    """As plan_arrays and the tests build it: pointers assigned to the fields."""
    status = np.full(3, -99, np.int32)
    nodes = np.full(6, -99, np.int32)
    wmap = np.full(3, -1, np.int32)
    refs = [weakref.ref(a) for a in (status, nodes, wmap)]
    o = capi.sr_plan_out()
    o.status = capi.ptr(status, capi.P32)
    o.node_of_pod = capi.ptr(nodes, capi.P32)
    o.winner_map = capi.ptr(wmap, capi.P32)
    return o, refs


def _alive(refs):
    return [r() is not None for r in refs]


def test_candidates_keep_their_arrays_while_alive():
    c, refs = _candidates_from_temporaries()
    gc.collect()
    assert _alive(refs) == [True, True, True]
    # (only now is reading through the pointers defined behaviour)
    assert c.n_cand == 3
    assert [c.cand_pod_off[i] for i in range(4)] == [0, 2, 3, 6]
    assert [c.cand_pods[i] for i in range(6)] == [10, 11, 12, 13, 14, 15]
    assert [c.cand_global[i] for i in range(3)] == [1, 3, 5]
    del c
    gc.collect()
    assert _alive(refs) == [False, False, False]  # and no longer: nothing leaks


def test_plan_out_keeps_its_arrays_while_alive():
    o, refs = _plan_out_from_temporaries()
    gc.collect()
    assert _alive(refs) == [True, True, True]
    assert [o.status[i] for i in range(3)] == [-99] * 3
    assert [o.node_of_pod[i] for i in range(6)] == [-99] * 6
    assert [o.winner_map[i] for i in range(3)] == [-1] * 3
    o.winner = 2  # plain fields stay plain
    assert o.winner == 2
    del o
    gc.collect()
    assert _alive(refs) == [False, False, False]


def test_keyword_arguments_keep_their_arrays():
    off = np.array([0, 1], np.int32)
    pods = np.array([7], np.int32)
    refs = [weakref.ref(off), weakref.ref(pods)]
    c = capi.sr_candidates(n_cand=1, cand_pod_off=capi.ptr(off, capi.P32), cand_pods=capi.ptr(pods, capi.P32))
    del off, pods
    gc.collect()
    assert _alive(refs) == [True, True]
    assert not c.cand_global  # unset: NULL
    assert c.cand_pods[0] == 7
    del c
    gc.collect()
    assert _alive(refs) == [False, False]


def test_reassigned_field_releases_the_old_array_and_holds_the_new_one():
    o, refs = _plan_out_from_temporaries()
    new = np.full(4, 5, np.int32)
    new_ref = weakref.ref(new)
    o.status = capi.ptr(new, capi.P32)
    del new
    gc.collect()
    assert _alive(refs) == [False, True, True]  # the old status array went, the others stay
    assert new_ref() is not None
    assert [o.status[i] for i in range(4)] == [5] * 4
    o.node_of_pod = None  # as plan_arrays(full=False) sets it: NULL, the array released
    gc.collect()
    assert _alive(refs) == [False, False, True]
    assert not o.node_of_pod

    c, crefs = _candidates_from_temporaries()
    c.cand_global = capi.ptr(None, capi.P32)  # a NULL pointer object releases too
    gc.collect()
    assert _alive(crefs) == [True, True, False]
    assert not c.cand_global
    del o, c
    gc.collect()
    assert new_ref() is None and _alive(refs) == [False] * 3 and _alive(crefs) == [False] * 3


def test_struct_copies_made_by_ctypes_see_the_same_memory():
    """byref(struct) is what the library gets: the addresses in the struct are
    the arrays' own, not copies."""
    off = np.array([0, 1], np.int32)
    pods = np.array([4], np.int32)
    c = capi.sr_candidates(1, capi.ptr(off, capi.P32), capi.ptr(pods, capi.P32), None)
    assert ctypes.cast(c.cand_pod_off, ctypes.c_void_p).value == off.ctypes.data
    assert ctypes.cast(c.cand_pods, ctypes.c_void_p).value == pods.ctypes.data
    pods[0] = 9
    assert c.cand_pods[0] == 9


def test_field_layout_is_the_headers():
    """The C ABI of the two structs: field order, offsets and sizes as
    include/sr_planner.h declares them (LP64)."""
    P = ctypes.sizeof(ctypes.c_void_p)
    assert P == 8
    assert [(n, getattr(capi.sr_candidates, n).offset) for n, _ in capi.sr_candidates._fields_] == \
        [("n_cand", 0), ("cand_pod_off", 8), ("cand_pods", 16), ("cand_global", 24)]
    assert ctypes.sizeof(capi.sr_candidates) == 32
    assert [(n, getattr(capi.sr_plan_out, n).offset) for n, _ in capi.sr_plan_out._fields_] == \
        [("winner", 0), ("first_ok", 4), ("first_fallback", 8), ("winner_npods", 12), ("checks", 16),
         ("fallback_pods", 24), ("status", 32), ("node_of_pod", 40), ("winner_map", 48), ("checks_dense", 56)]
    assert ctypes.sizeof(capi.sr_plan_out) == 64
