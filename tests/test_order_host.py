"""PFACX_orderHitsFromHost against the two models of tests/order_ref.py (checked against each other here): every column combination, ties with
and without the flag, INT_MIN / INT_MAX / negative starts and ids, the already-ordered exit, all starts equal, a strictly descending list,
n = 0 and n = 1, every refusal with each pairwise overlap, a host-only handle on every platform, and one real class-signature list.  All arrays
are poisoned around the list; every comparison is exact."""

import ctypes as C
import itertools

import numpy as np
import pytest

from pfac_amd import api
from tests import cover_ref
from tests import order_ref as ref

INVALID, NOT_EXIST = api.STATUS.INVALID_PARAMETER, api.STATUS.LIB_NOT_EXIST
TIES = api.PFACX_ORDER_TIES_BY_ID
GUARD = 16
POISON = -7


@pytest.fixture(scope="module")
def handle():
    h = api.PFAC.createHostOnly()
    yield h
    h.destroy()


def guarded(values):
    a = np.full(GUARD + len(values) + GUARD, POISON, dtype=np.int32)
    a[GUARD:GUARD + len(values)] = values
    return a, a.ctypes.data + 4 * GUARD


def run_host(h, starts, ids=None, ends=None, aux=None, ties=False, with_perm=True):
    """the host form over guarded copies -> (columns given ..., perm, was_ordered)"""
    n = len(starts)
    cols = [guarded(np.asarray(c, dtype=np.int32)) if c is not None else None for c in (starts, ids, ends, aux)]
    perm = guarded(np.full(n, POISON, dtype=np.int32)) if with_perm else None
    ptr = [c[1] if c is not None and n else None for c in cols]
    st, was = h.orderHitsFromHost(ptr[0], ptr[1], ptr[2], ptr[3], n, TIES if ties else 0, perm[1] if perm and n else None)
    assert st == 0
    for c in cols + [perm]:
        if c is not None:
            assert (c[0][:GUARD] == POISON).all() and (c[0][GUARD + n:] == POISON).all(), "wrote outside the arrays"
    out = [c[0][GUARD:GUARD + n].copy() for c in cols if c is not None]
    return (*out, perm[0][GUARD:GUARD + n].copy() if perm else None, was)


def check(h, starts, ids=None, ends=None, aux=None, ties=False, what=""):
    want = ref.model(starts, ids, ends, aux, ties)
    got = run_host(h, starts, ids, ends, aux, ties)
    ref.same(got, want, what)
    return want


def test_the_two_models_agree():
    for seed in ref.RANDOM_SEEDS:
        starts, ids, _, _ = ref.random_list(seed)
        for ties in (False, True):
            assert ref.perm_numpy(starts, ids, ties).tolist() == ref.perm_python(starts, ids, ties), seed
    for name, starts, ids in ref.HAND:
        for ties in (False, True):
            assert ref.perm_numpy(starts, ids, ties).tolist() == ref.perm_python(starts, ids, ties), name
    # worked out by hand: stable without the flag, by id with it
    assert ref.perm_python([4, 4, 4, 1, 1], [9, 8, 7, 6, 5]) == [3, 4, 0, 1, 2]
    assert ref.perm_python([4, 4, 4, 1, 1], [9, 8, 7, 6, 5], True) == [4, 3, 2, 1, 0]
    assert ref.perm_python([5, 5 + ref.INT_MIN], [1, 1]) == [1, 0]


@pytest.mark.parametrize("combo", ref.COLUMN_COMBINATIONS, ids=lambda c: "".join("iea"[k] if c[k] else "-" for k in range(3)))
def test_every_column_combination(handle, combo):
    for seed in ref.RANDOM_SEEDS[:24]:
        starts, ids, ends, aux = ref.random_list(seed)
        cols = ref.pick_columns(starts, ids, ends, aux, combo)
        check(handle, *cols, ties=False, what=(seed, combo))
        if combo[0]:
            check(handle, *cols, ties=True, what=(seed, combo, "ties"))


@pytest.mark.parametrize("name,starts,ids", ref.HAND, ids=[h[0] for h in ref.HAND])
def test_lists_by_hand(handle, name, starts, ids):
    aux = np.arange(len(starts), dtype=np.int32)
    for ties in (False, True):
        want = check(handle, starts, ids, None, aux, ties, what=(name, ties))
        assert np.array_equal(want[2], want[3]), "aux = arange comes out as the permutation"


def test_ties_with_and_without_the_flag(handle):
    starts, ids = [4, 4, 4, 1, 1], [9, 8, 7, 6, 5]
    got = run_host(handle, starts, ids)
    assert got[0].tolist() == [1, 1, 4, 4, 4] and got[1].tolist() == [6, 5, 9, 8, 7] and got[2].tolist() == [3, 4, 0, 1, 2] and got[3] == 0
    got = run_host(handle, starts, ids, ties=True)
    assert got[0].tolist() == [1, 1, 4, 4, 4] and got[1].tolist() == [5, 6, 7, 8, 9] and got[2].tolist() == [4, 3, 2, 1, 0] and got[3] == 0


def test_already_ordered_exit_writes_no_column(handle):
    starts, ids, ends = [1, 1, 2, 3, 3, 3], [2, 1, 1, 2, 4, 3], [9, 8, 7, 6, 5, 4]
    got = run_host(handle, starts, ids, ends)
    assert got[0].tolist() == starts and got[1].tolist() == ids and got[2].tolist() == ends and got[3].tolist() == list(range(6)) and got[4] == 1
    got = run_host(handle, starts, ids, ends, ties=True)                     # the same list is not in (start, id) order
    assert got[4] == 0 and got[1].tolist() == [1, 2, 1, 2, 3, 4] and got[3].tolist() == [1, 0, 2, 3, 5, 4]
    # read-only pages behind the columns would be the strict proof; here: a list of one start, no flag -- ordered whatever the other columns say
    got = run_host(handle, [9] * 5, [5, 4, 3, 2, 1], None, [4, 3, 2, 1, 0])
    assert got[4] == 1 and got[1].tolist() == [5, 4, 3, 2, 1] and got[3].tolist() == [0, 1, 2, 3, 4]
    got = run_host(handle, [9] * 5, [5, 4, 3, 2, 1], None, [4, 3, 2, 1, 0], with_perm=False)
    assert got[4] == 1 and got[3] is None


def test_no_hit_and_one_hit(handle):
    st, was = handle.orderHitsFromHost(None, None, None, None, 0, 0, None)
    assert (st, was) == (0, 1)
    junk = np.full(4, POISON, dtype=np.int32)
    st, was = handle.orderHitsFromHost(junk.ctypes.data, None, None, None, 0, 0, junk.ctypes.data)   # the same array twice: no byte of it counts
    assert (st, was) == (0, 1) and (junk == POISON).all()
    lib = api.load_library()
    assert lib.PFACX_orderHitsFromHost(handle._h, None, None, None, None, 0, 0, None, None) == 0
    for ties in (False, True):
        got = run_host(handle, [ref.INT_MIN], [ref.INT_MAX], [3], [4], ties)
        assert [g.tolist() for g in got[:5]] == [[ref.INT_MIN], [ref.INT_MAX], [3], [4], [0]] and got[5] == 1


def test_every_refusal_and_every_overlap(handle):
    lib = api.load_library()
    arrays = [guarded(np.array(v, dtype=np.int32)) for v in ([5, 3, 9, 1], [1, 2, 3, 4], [6, 4, 10, 2], [0, 1, 2, 3], [POISON] * 4)]
    before = [a[0].copy() for a in arrays]
    ps, pi, pe, pa, pp = (a[1] for a in arrays)
    was = C.c_int(77)
    H, W = handle._h, C.byref(was)
    for form in (lib.PFACX_orderHitsFromHost, lib.PFACX_orderHitsFromDevice):
        assert form(None, ps, pi, pe, pa, 4, 0, pp, W) == INVALID, "a null handle"
        assert form(H, None, pi, pe, pa, 4, 0, pp, W) == INVALID, "no starts"
        assert form(H, ps, pi, pe, pa, 2 ** 31, 0, pp, W) == INVALID
        for flags in (2, 3, 0x80000000):
            assert form(H, ps, pi, pe, pa, 4, flags, pp, W) == INVALID, flags
        assert form(H, ps, None, pe, pa, 4, api.PFACX_ORDER_TIES_BY_ID, pp, W) == INVALID, "the ties flag without ids"
        # every pair of the five arrays: the same array twice, and one byte shared at either end
        for i, j in itertools.combinations(range(5), 2):
            for shift in (0, 12, -12):
                args = [ps, pi, pe, pa, pp]
                args[j] = args[i] + shift
                assert form(H, args[0], args[1], args[2], args[3], 4, 0, args[4], W) == INVALID, (i, j, shift)
    assert was.value == 77 and all(np.array_equal(a[0], b) for a, b in zip(arrays, before)), "a refused call wrote something"
    # arrays that only touch are apart
    row = np.array([5, 3, 9, 1, 1, 2, 3, 4], dtype=np.int32)
    assert lib.PFACX_orderHitsFromHost(H, row.ctypes.data, row.ctypes.data + 16, None, None, 4, 0, None, W) == 0 and was.value == 0
    assert row.tolist() == [1, 3, 5, 9, 4, 2, 1, 3]


@pytest.mark.parametrize("platform", [api.PFAC_PLATFORM_GPU, api.PFAC_PLATFORM_CPU, api.PFAC_PLATFORM_CPU_OMP])
def test_host_only_handle_on_every_platform(platform):
    h = api.PFAC.createHostOnly()
    try:
        h.setPlatform(platform, check=False)
        starts, ids, ends, aux = ref.random_list(5)
        check(h, starts, ids, ends, aux, True, platform)
        a = np.array([3, 1], dtype=np.int32)
        st, _ = h.orderHitsFromDevice(a.ctypes.data, None, None, None, 2, 0, None, check=False)
        assert st == NOT_EXIST and a.tolist() == [3, 1], "the device form needs a device"
        st, _ = h.orderHitsFromDevice(None, None, None, None, 0, 0, None, check=False)
        assert st == NOT_EXIST
    finally:
        h.destroy()


def test_order_hits_host_array(handle):
    starts, ids, ends, aux = ref.random_list(8)
    want = ref.model(starts, ids, ends, aux, True)
    keep = starts.copy()
    ref.same(handle.order_hits_host_array(starts, ids, ends, aux, ties_by_id=True), want)
    assert np.array_equal(starts, keep), "the caller's arrays are copied"
    ref.same(handle.order_hits_host_array(starts, ends=ends), ref.model(starts, None, ends))
    ref.same(handle.order_hits_host_array(starts), ref.model(starts))
    got = handle.order_hits_host_array([])
    assert got[0].size == 0 and got[1].size == 0 and got[2] == 1


def test_a_class_signature_list():
    text = cover_ref.token_text(3, 16 * 1024)
    h = api.PFAC.createHostOnly()
    h.setPlatform(api.PFAC_PLATFORM_CPU)
    try:
        with h.clsigOpenText(b"".join(r + b"\n" for r in ref.CLSIG_RULES)) as sg:
            pos, ids, end = sg.match_host_array(np.frombuffer(text, dtype=np.uint8))
        assert pos.size >= 100 and set(ids.tolist()) == {1, 2, 3, 4} and (np.diff(pos) < 0).any(), "the list is not in start order"
        for ties in (False, True):
            want = ref.model(pos, ids, end, None, ties)
            ref.same(h.order_hits_host_array(pos, ids, end, ties_by_id=ties), want, ties)
            assert (np.diff(want[0]) >= 0).all() and want[-1] == 0
    finally:
        h.destroy()
