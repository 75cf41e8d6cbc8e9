"""PFACX_approxOpen / PFACX_approxGetPieces / PFACX_approxMatchFromHost on the CPU platforms (host-only handles: no device needed) against the
models of tests/approx_ref.py: every case of the table with its ordered list and distances, the getter against the documented cut and against the
handle's own pattern list, every refusal with its badPattern and the handle's set untouched, the getter with n too small and with NULL arrays, the
count query and truncation at capacities 0, 1, total - 1 and total between guard words, the status rows, the stale object, the ApproxSet wrapper,
and the seeded random cases the GPU file runs."""

import ctypes as C

import numpy as np
import pytest

from pfac_amd import api
from tests import approx_ref as ref
from tests.approx_ref import test_the_models_agree_on_every_case  # noqa: F401  (runs here: approx_ref.py is not collected)

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
INVALID, NOT_EXIST, TRUNCATED, BAD_HANDLE = (api.STATUS.INVALID_PARAMETER, api.STATUS.LIB_NOT_EXIST, api.STATUS.OUTPUT_TRUNCATED,
                                             api.STATUS.INVALID_HANDLE)
GUARD = 16


def host_handle(platform=api.PFAC_PLATFORM_CPU):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    return h


def host_approx(ap, data, capacity=None, with_mis=True):
    """match_host into poisoned arrays of `capacity` entries (default: the full length, asked for first) with GUARD poisoned ints on both sides
    -> (status, (pos, ids, mis) of the entries written, the full length); nothing outside the written entries may change, nor the input"""
    buf = ref.as_array(data).copy()
    n = buf.size
    if capacity is None:
        st, capacity = ap.match_host(buf.ctypes.data, n, None, None, None, 0, check=False)
        assert st in (0, TRUNCATED) and (st == TRUNCATED) == (capacity > 0)
    ids, pos, mis = (np.full(GUARD + capacity + GUARD, -7, dtype=np.int32) for _ in range(3))
    st, total = ap.match_host(buf.ctypes.data, n, ids.ctypes.data + 4 * GUARD, pos.ctypes.data + 4 * GUARD,
                              mis.ctypes.data + 4 * GUARD if with_mis else None, capacity, check=False)
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > capacity)
    k = min(total, capacity)
    for a in (ids, pos, mis):
        assert np.all(a[:GUARD] == -7) and np.all(a[GUARD + capacity:] == -7), "wrote outside the arrays"
        assert np.all(a[GUARD + k:GUARD + capacity] == -7), "wrote behind the list"
    assert with_mis or np.all(mis == -7)
    assert buf.tobytes() == bytes(ref.as_array(data)), "the caller's input was modified"
    return st, tuple(a[GUARD:GUARD + k].copy() for a in (pos, ids, mis)), total


def check_getter(h, ap, patterns, budgets, min_len=0, max_len=0):
    """the getter equals the documented cut, and handle id q IS the q-th distinct piece: the handle finds each piece under that id"""
    got = ap.pieces()
    want, pieces = ref.model_pieces(patterns, budgets, min_len, max_len)
    for g, w, what in zip(got, want, ("piece offsets", "piece id", "piece start", "piece length")):
        assert g.tolist() == w.tolist(), what
    for q, piece in enumerate(pieces, start=1):
        found = h.match_host_array(np.frombuffer(piece, dtype=np.uint8))
        assert int(found[0]) == q, f"the handle's pattern {q} is not the {q}-th distinct piece"
    assert h.caseInsensitive() == 0
    return got


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_equals_the_models(case, platform, pname):
    name, patterns, budgets, min_len, max_len, data = ref.case_of(case)
    want = ref.check_models(patterns, budgets, data, name, max_len)
    h = host_handle(platform)
    try:
        with h.approxOpen(patterns, budgets, min_len, max_len) as ap:
            assert ap.status == 0 and ap.bad == 0 and ap.num_patterns == len(patterns) and ap.num_pieces == sum(budgets) + len(budgets)
            check_getter(h, ap, patterns, budgets, min_len, max_len)
            st, got, total = host_approx(ap, data)
            assert st == 0 and total == want[0].size
            ref.same(got, want, f"{name}/{pname}")
            if name in ref.WANT:
                ids, pos, mis = ref.WANT[name]
                ref.same(got, (pos, ids, mis), f"{name}/{pname}: against the list worked out by hand")
            ref.same(ap.match_host_array(ref.as_array(data)), want, f"{name}/match_host_array")
            ref.same(host_approx(ap, data, with_mis=False)[1][:2], want[:2], f"{name}/{pname}/no distances")
    finally:
        h.destroy()


@pytest.mark.parametrize("name", ["keywords-with-typos", "two-patterns-share-a-piece"])
def test_the_count_query_and_truncation(name):
    _, patterns, budgets, min_len, max_len, data = ref.case_of(next(c for c in ref.CASES if c[0] == name))
    want = ref.check_models(patterns, budgets, data, name, max_len)
    total = int(want[0].size)
    assert total > 2
    h = host_handle()
    try:
        with h.approxOpen(patterns, budgets, min_len, max_len) as ap:
            buf = ref.as_array(data).copy()
            assert ap.match_host(buf.ctypes.data, buf.size, None, None, None, 0, check=False) == (TRUNCATED, total), "the count query"
            for cap in (0, 1, total - 1, total, total + 3):
                st, got, n = host_approx(ap, data, capacity=cap)
                assert (st, n) == (TRUNCATED if cap < total else 0, total)
                ref.same(got, tuple(w[:cap] for w in want), f"capacity {cap}")
    finally:
        h.destroy()


LONG = b"x" * 65536


@pytest.mark.parametrize("patterns,budgets,min_len,max_len,bad,why", [
    ([b"abcd", b"", b"efgh"], [0, 0, 0], 0, 0, 2, "an empty pattern"),
    ([b"abcd", LONG], [0, 0], 0, 0, 2, "65 536 bytes"),
    ([b"abcd", b"x" * 64], [0, 8], 0, 0, 2, "a budget of 8"),
    ([b"abcd", b"x" * 64, b"y" * 64], [0, 0, -1], 0, 0, 3, "a negative budget"),
    ([b"abcdefg"], [1], 0, 0, 1, "7 bytes for two pieces of 4"),
    ([b"abcdefgh", b"abcdefghijk"], [1, 2], 0, 0, 2, "11 bytes for three pieces of 4"),
    ([b"abcdefghi"], [1], 5, 0, 1, "9 bytes for two pieces of minPieceLen 5"),
    ([b"ab"], [2], 1, 0, 1, "fewer bytes than parts"),
    ([b"abcd"], [0], 65536, 0, 1, "a minPieceLen no pattern can have"),
    ([b"abcd", b"ab\ncdefgh"], [0, 0], 0, 0, 2, "0x0A in the only piece"),
    ([b"abcdefgh", b"abcdefg\n"], [1, 1], 0, 0, 2, "0x0A at the end of the last piece"),
    ([b"abcdefgh", b"abcd\nfgh"], [1, 1], 0, 0, 2, "0x0A at the head of piece 1"),
    ([b"abcde\nfgh"], [0], 0, 6, 1, "0x0A as the last byte the cut keeps"),
])
def test_the_open_call_refuses_with_the_pattern(patterns, budgets, min_len, max_len, bad, why):
    assert ref.refusal(patterns, budgets, min_len, max_len) == bad, "the model of the rule"
    h = host_handle()
    try:
        h.readPatternFromMemory(b"kept\n")
        ap = h.approxOpen(patterns, budgets, min_len, max_len, check=False)
        assert (ap.status, ap.bad) == (INVALID, bad), why
        assert not ap._c, "no object behind a refusal"
        assert int(h.match_host_array(np.frombuffer(b"kept", dtype=np.uint8))[0]) == 1, "a refusal leaves the handle's set alone"
    finally:
        h.destroy()


def test_what_lies_just_inside_the_refusals():
    h = host_handle()
    try:
        with h.approxOpen([LONG[:65535]], [7]) as ap:
            off, _, start, length = ap.pieces()
            assert off.tolist() == [0, 0, 8] and start.tolist() == [j * 65535 // 8 for j in range(8)] and length.tolist() == [32] * 8
        with h.approxOpen([b"abcde\nfgh", b"abcdefgh"], [0, 1], 0, 5) as ap:              # 0x0A right behind the cut; exactly (k + 1) minPieceLen bytes
            assert ap.pieces()[3].tolist() == [5, 4, 4]
            pos, ids, mis = ap.match_host_array(np.frombuffer(b"abcde\nfgh abcdeXfgh abcdefgx", dtype=np.uint8))
            assert (ids.tolist(), pos.tolist(), mis.tolist()) == ([1, 2], [0, 20], [0, 1]), "a 0x0A outside every piece is compared like any byte"
        with h.approxOpen((np.frombuffer(b"..abcdefgh", dtype=np.uint8), [2, 6, 10]), [0, 0]) as ap:   # the CSR form need not start at 0
            assert ap.match_host_array(np.frombuffer(b"abcdefgh..", dtype=np.uint8))[1].tolist() == [1, 2]
    finally:
        h.destroy()


def test_the_open_call_refuses_arguments():
    lib = api.load_library()
    h = host_handle()
    try:
        blob = np.frombuffer(b"abcdefgh", dtype=np.uint8).copy()
        off, budget = np.array([0, 4, 8], dtype=np.uint64), np.zeros(2, dtype=np.int32)
        a, bad = C.c_void_p(), C.c_int(-1)
        args = lambda **kw: [kw.get("h", h._h), kw.get("b", blob.ctypes.data), kw.get("off", off.ctypes.data), kw.get("k", budget.ctypes.data),  # noqa: E731
                             kw.get("n", 2), 0, 0, kw.get("a", C.byref(a)), kw.get("bad", C.byref(bad))]
        h.readPatternFromMemory(b"kept\n")
        assert lib.PFACX_approxOpen(*args(h=None)) == BAD_HANDLE
        for null in ("b", "off", "k", "a"):
            assert lib.PFACX_approxOpen(*args(**{null: None})) == INVALID, null
        assert lib.PFACX_approxOpen(*args(n=0)) == INVALID and bad.value == 0, "numPatterns == 0"
        assert lib.PFACX_approxOpen(*args(n=(1 << 31) - 1)) == INVALID and bad.value == 0, "numPatterns >= 2^31 - 1"
        descending = np.array([0, 6, 4], dtype=np.uint64)
        assert lib.PFACX_approxOpen(*args(off=descending.ctypes.data)) == INVALID and bad.value == 2, "an h_patOff that descends"
        assert int(h.match_host_array(np.frombuffer(b"kept", dtype=np.uint8))[0]) == 1, "a refusal leaves the handle's set alone"
        assert lib.PFACX_approxOpen(*args(bad=None)) == 0 and a.value, "badPattern may be null"
        assert lib.PFACX_approxClose(a) == 0
        assert lib.PFACX_approxClose(None) == BAD_HANDLE
    finally:
        h.destroy()


def test_the_getter_with_n_too_small_and_with_null_arrays():
    lib = api.load_library()
    patterns, budgets = [b"abcdefgh", b"abcdWXYZ0123", b"efghabcd"], [1, 2, 0]
    h = host_handle()
    try:
        with h.approxOpen(patterns, budgets) as ap:
            want, pieces = ref.model_pieces(patterns, budgets)
            assert pieces == [b"abcd", b"efgh", b"WXYZ", b"0123", b"efghabcd"] and want[1].tolist() == [1, 2, 1, 3, 4, 5]
            E = 6
            off = np.full(5, 99, dtype=np.uint64)
            arrays = [np.full(E, -7, dtype=np.int32) for _ in range(3)]
            ptr = [a.ctypes.data for a in arrays]
            for given in ([0], [1], [2], [0, 1, 2]):                # n < the number of pieces with a per-piece array given: nothing is written
                use = [ptr[i] if i in given else None for i in range(3)]
                assert lib.PFACX_approxGetPieces(ap._c, off.ctypes.data, *use, E - 1) == INVALID
            assert off.tolist() == [99] * 5 and all(np.all(a == -7) for a in arrays)
            assert lib.PFACX_approxGetPieces(ap._c, off.ctypes.data, None, None, None, 0) == 0, "the offsets alone: n is not looked at"
            assert off.tolist() == want[0].tolist() == [0, 0, 2, 5, 6]
            for i in range(3):                                      # each array alone
                use = [ptr[j] if j == i else None for j in range(3)]
                assert lib.PFACX_approxGetPieces(ap._c, None, *use, E) == 0
                assert arrays[i].tolist() == want[i + 1].tolist()
            assert lib.PFACX_approxGetPieces(ap._c, None, None, None, None, 0) == 0
            assert lib.PFACX_approxGetPieces(None, None, None, None, None, 0) == BAD_HANDLE
    finally:
        h.destroy()


def test_status_rows_and_the_stale_object():
    lib = api.load_library()
    h = host_handle()
    try:
        ap = h.approxOpen([b"abcdefgh"], [1])
        data = np.frombuffer(b"abcdefgx", dtype=np.uint8).copy()
        ids, pos, mis = (np.full(8, -7, dtype=np.int32) for _ in range(3))
        n = C.c_size_t(99)
        call = lambda fn, size=8, cap=8, inp=data.ctypes.data, i=ids.ctypes.data, p=pos.ctypes.data, m=mis.ctypes.data, num=C.byref(n): fn(  # noqa: E731
            ap._c, inp, size, i, p, m, cap, num)
        assert call(lib.PFACX_approxMatchFromHost) == 0 and n.value == 1 and (ids[0], pos[0], mis[0]) == (1, 0, 1)
        assert call(lib.PFACX_approxMatchFromHost, size=0) == 0 and n.value == 0, "size == 0"
        assert call(lib.PFACX_approxMatchFromHost, size=1 << 31) == INVALID, "size >= 2^31"
        assert call(lib.PFACX_approxMatchFromHost, inp=None) == INVALID and call(lib.PFACX_approxMatchFromHost, num=None) == INVALID
        assert call(lib.PFACX_approxMatchFromHost, i=None) == INVALID and call(lib.PFACX_approxMatchFromHost, p=None) == INVALID
        assert call(lib.PFACX_approxMatchFromHost, m=None) == 0 and n.value == 1, "the distances are optional"
        assert call(lib.PFACX_approxMatchFromHost, cap=0, i=None, p=None, m=None) == TRUNCATED and n.value == 1, "the count query"
        assert call(lib.PFACX_approxMatchFromDevice) == NOT_EXIST, "a device form on a host-only handle"
        assert call(lib.PFACX_approxMatchFromDevice, cap=7) == INVALID, "capacity < size"
        assert lib.PFACX_approxPairsFromDevice(ap._c, data.ctypes.data, 8, ids.ctypes.data, pos.ctypes.data, 1, None, None, None, 0, C.byref(n)) == NOT_EXIST
        assert lib.PFACX_approxMatchFromHost(None, data.ctypes.data, 8, None, None, None, 0, C.byref(n)) == BAD_HANDLE
        # the handle reads another set: only the close call works
        h.readPatternFromMemory(b"a\n")
        assert call(lib.PFACX_approxMatchFromHost) == INVALID and call(lib.PFACX_approxMatchFromDevice) in (INVALID, NOT_EXIST)
        assert lib.PFACX_approxGetPieces(ap._c, None, ids.ctypes.data, None, None, 8) == INVALID
        with pytest.raises(api.PFACError):
            ap.pieces()
        assert ap.close() == 0
        # a second open replaces the set of the first: the first object goes stale the same way
        first = h.approxOpen([b"abcd"], [0])
        second = h.approxOpen([b"efgx"], [0])
        assert first.match_host(data.ctypes.data, 8, None, None, None, 0, check=False)[0] == INVALID
        assert second.match_host(data.ctypes.data, 8, None, None, None, 0, check=False) == (TRUNCATED, 1)
        assert first.close() == 0 and second.close() == 0
    finally:
        h.destroy()


def test_destroy_closes_the_object_and_the_handle_counts_no_device_tables():
    h = host_handle()
    ap = h.approxOpen([b"abcdefgh"], [1])
    assert h.info().deviceTableBytes == 0, "a host-only handle uploads nothing"
    h.destroy()
    ap._c = C.c_void_p()                                        # PFAC_destroy closed it


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_the_compare_edges(k):
    """lengths (k + 1) .. 64 with exactly k and k + 1 substitutions, the deciding one at byte 0, 15 / 16, 31 / 32, the last whole dword, each
    tail byte"""
    patterns, budgets, data, _ = ref.edge_case(k)
    want = ref.check_edge_case(k)
    h = host_handle(api.PFAC_PLATFORM_CPU_OMP)
    try:
        with h.approxOpen(patterns, budgets, 1) as ap:
            ref.same(ap.match_host_array(ref.as_array(data)), want, f"edges k = {k}")
    finally:
        h.destroy()


@pytest.mark.parametrize("kind", ["acgt", "text"])
def test_the_seeded_random_cases(kind):
    """the cases tests/test_approx_gpu.py runs: 100 patterns of 12 .. 150 letters with budgets 0 .. 4 over 64 KiB, each embedded with exactly k,
    k + 1 and 0 substitutions"""
    patterns, budgets, data = ref.random_case(kind)
    assert len(patterns) == 100 and data.size == 1 << 16 and set(budgets) == {0, 1, 2, 3, 4}
    want = ref.random_want(kind)
    assert 100 <= want[0].size <= 2000 and set(want[2].tolist()) >= {0, 1, 2, 3, 4}
    h = host_handle(api.PFAC_PLATFORM_CPU_OMP)
    try:
        with h.approxOpen(patterns, budgets) as ap:
            check_getter(h, ap, patterns, budgets)
            ref.same(ap.match_host_array(data), want, f"random {kind}/host")
    finally:
        h.destroy()
