"""PFACX_editOpen / PFACX_editGetPieces / PFACX_editMatchFromHost on the CPU platforms (host-only handles: no device needed) against the models
of tests/edit_ref.py: the models against each other and against the lists worked out by hand, every case of the table with and without
PFACX_EDIT_BEST_ENDS, the getter, every refusal with its badPattern and the handle's set untouched, an unknown flag, the count query and
truncation at capacities 0, 1, total - 1 and total between guard words with each of the two optional arrays NULL, the status rows, the stale
object, the band edges, the early exit, starts at 0 and ends at n, each occurrence once, and the seeded random cases the GPU file runs."""

import ctypes as C

import numpy as np
import pytest

from pfac_amd import api
from tests import edit_ref as ref

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
INVALID, NOT_EXIST, TRUNCATED, BAD_HANDLE = (api.STATUS.INVALID_PARAMETER, api.STATUS.LIB_NOT_EXIST, api.STATUS.OUTPUT_TRUNCATED,
                                             api.STATUS.INVALID_HANDLE)
BEST = api.PFACX_EDIT_BEST_ENDS
GUARD = 16
FLAGS = pytest.mark.parametrize("flags", [0, BEST], ids=["all-ends", "best-ends"])


def host_handle(platform=api.PFAC_PLATFORM_CPU):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    return h


def host_edit(ed, data, capacity=None, with_end=True, with_dist=True):
    """match_host into poisoned arrays of `capacity` entries (default: the full length, asked for first) with GUARD poisoned ints on both sides
    -> (status, (ids, start, end, dist) of the entries written, the full length); nothing outside the written entries may change, nor the input"""
    buf = ref.as_array(data).copy()
    n = buf.size
    if capacity is None:
        st, capacity = ed.match_host(buf.ctypes.data, n, None, None, None, None, 0, check=False)
        assert st in (0, TRUNCATED) and (st == TRUNCATED) == (capacity > 0)
    arrays = [np.full(GUARD + capacity + GUARD, -7, dtype=np.int32) for _ in range(4)]
    ptr = [a.ctypes.data + 4 * GUARD for a in arrays]
    st, total = ed.match_host(buf.ctypes.data, n, ptr[0], ptr[1], ptr[2] if with_end else None, ptr[3] if with_dist else None, capacity, check=False)
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > capacity)
    k = min(total, capacity)
    for a in arrays:
        assert np.all(a[:GUARD] == -7) and np.all(a[GUARD + capacity:] == -7), "wrote outside the arrays"
        assert np.all(a[GUARD + k:GUARD + capacity] == -7), "wrote behind the list"
    assert (with_end or np.all(arrays[2] == -7)) and (with_dist or np.all(arrays[3] == -7))
    assert buf.tobytes() == bytes(ref.as_array(data)), "the caller's input was modified"
    return st, tuple(a[GUARD:GUARD + k].copy() for a in arrays), total


def host_list(patterns, budgets, data, what, min_len=0, max_len=0, flags=0, platform=api.PFAC_PLATFORM_CPU_OMP):
    """the host form against both models -> the list"""
    want = ref.check_models(patterns, budgets, data, what, flags, max_len)
    h = host_handle(platform)
    try:
        with h.editOpen(patterns, budgets, min_len, max_len, flags) as ed:
            ref.same(ed.match_host_array(ref.as_array(data)), want, what)
    finally:
        h.destroy()
    return want


def rows(want):
    return list(zip(*[w.tolist() for w in want]))


# ---------------------------------------------------------------- the models


@FLAGS
@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_the_models_agree_on_every_case(case, flags):
    name, patterns, budgets, min_len, max_len, data = ref.case_of(case)
    want = ref.check_models(patterns, budgets, data, name, flags, max_len)                 # brute force == pigeonhole, as sets
    assert ref.edit_naive(patterns, budgets, data, flags) == ref.edit_brute(patterns, budgets, data, flags), "the recursion pins the brute force"
    if name in ref.WANT:
        ref.same(want, ref.want_of(name, flags), f"{name}: against the list worked out by hand")


def test_an_exact_copy_with_k_2_gives_five_ends_and_one_under_the_rule():
    _, patterns, budgets, _, _, data = ref.case_of(next(c for c in ref.CASES if c[0] == "exact-copy-k2"))
    assert len(ref.edit_brute(patterns, budgets, data, 0)) == 5 and len(ref.edit_brute(patterns, budgets, data, BEST)) == 1


# ---------------------------------------------------------------- the case table


def check_getter(h, ed, patterns, budgets, min_len=0, max_len=0):
    """the getter equals the documented cut, and handle id q IS the q-th distinct piece: the handle finds each piece under that id"""
    got = ed.pieces()
    want, pieces = ref.model_pieces(patterns, budgets, min_len, max_len)
    for g, w, what in zip(got, want, ("piece offsets", "piece id", "piece start", "piece length")):
        assert g.tolist() == w.tolist(), what
    for q, piece in enumerate(pieces, start=1):
        found = h.match_host_array(np.frombuffer(piece, dtype=np.uint8))
        assert int(found[0]) == q, f"the handle's pattern {q} is not the {q}-th distinct piece"
    assert h.caseInsensitive() == 0


@FLAGS
@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_equals_the_models(case, platform, pname, flags):
    name, patterns, budgets, min_len, max_len, data = ref.case_of(case)
    want = ref.check_models(patterns, budgets, data, name, flags, max_len)
    h = host_handle(platform)
    try:
        with h.editOpen(patterns, budgets, min_len, max_len, flags) as ed:
            assert ed.status == 0 and ed.bad == 0 and ed.num_patterns == len(patterns) and ed.num_pieces == sum(budgets) + len(budgets)
            check_getter(h, ed, patterns, budgets, min_len, max_len)
            st, got, total = host_edit(ed, data)
            assert st == 0 and total == want[0].size
            ref.same(got, want, f"{name}/{pname}")
            for with_end, with_dist in ((False, True), (True, False), (False, False)):
                got = host_edit(ed, data, with_end=with_end, with_dist=with_dist)[1]
                ref.same(got[:2], want[:2], f"{name}/{pname}/NULL arrays")
                assert not with_end or got[2].tolist() == want[2].tolist()
                assert not with_dist or got[3].tolist() == want[3].tolist()
    finally:
        h.destroy()


def test_the_count_query_and_truncation():
    name = "exact-copy-k2"
    _, patterns, budgets, min_len, max_len, data = ref.case_of(next(c for c in ref.CASES if c[0] == name))
    want = ref.check_models(patterns, budgets, data, name, 0, max_len)
    total = int(want[0].size)
    assert total == 5
    h = host_handle()
    try:
        with h.editOpen(patterns, budgets, min_len, max_len) as ed:
            buf = ref.as_array(data).copy()
            assert ed.match_host(buf.ctypes.data, buf.size, None, None, None, None, 0, check=False) == (TRUNCATED, total), "the count query"
            for cap in (0, 1, total - 1, total, total + 3):
                st, got, n = host_edit(ed, data, capacity=cap)
                assert (st, n) == (TRUNCATED if cap < total else 0, total)
                ref.same(got, tuple(w[:cap] for w in want), f"capacity {cap}")
    finally:
        h.destroy()


# ---------------------------------------------------------------- the open call

LONG = b"x" * 65536


@pytest.mark.parametrize("patterns,budgets,min_len,max_len,bad,why", [
    ([b"abcd", b"", b"efgh"], [0, 0, 0], 0, 0, 2, "an empty pattern"),
    ([b"abcd", LONG], [0, 0], 0, 0, 2, "65 536 bytes"),
    ([b"abcd", b"x" * 64], [0, 8], 0, 0, 2, "a budget of 8"),
    ([b"abcd", b"x" * 64, b"y" * 64], [0, 0, -1], 0, 0, 3, "a negative budget"),
    ([b"abcdefg"], [1], 0, 0, 1, "7 bytes for two pieces of 4"),
    ([b"abcdefgh", b"abcdefghijk"], [1, 2], 0, 0, 2, "11 bytes for three pieces of 4"),
    ([b"abcdefghi"], [1], 5, 0, 1, "9 bytes for two pieces of minPieceLen 5"),
    ([b"ab"], [2], 1, 0, 1, "fewer bytes than parts: L > k is enforced"),
    ([b"abcd"], [0], 65536, 0, 1, "a minPieceLen no pattern can have"),
    ([b"abcd", b"ab\ncdefgh"], [0, 0], 0, 0, 2, "0x0A in the only piece"),
    ([b"abcdefgh", b"abcd\nfgh"], [1, 1], 0, 0, 2, "0x0A at the head of piece 1"),
    ([b"abcde\nfgh"], [0], 0, 6, 1, "0x0A as the last byte the cut keeps"),
])
def test_the_open_call_refuses_with_the_pattern(patterns, budgets, min_len, max_len, bad, why):
    assert ref.refusal(patterns, budgets, min_len, max_len) == bad, "the model of the rule"
    h = host_handle()
    try:
        h.readPatternFromMemory(b"kept\n")
        ed = h.editOpen(patterns, budgets, min_len, max_len, check=False)
        assert (ed.status, ed.bad) == (INVALID, bad), why
        assert not ed._c, "no object behind a refusal"
        assert int(h.match_host_array(np.frombuffer(b"kept", dtype=np.uint8))[0]) == 1, "a refusal leaves the handle's set alone"
    finally:
        h.destroy()


def test_the_open_call_refuses_arguments_and_unknown_flags():
    lib = api.load_library()
    h = host_handle()
    try:
        blob = np.frombuffer(b"abcdefgh", dtype=np.uint8).copy()
        off, budget = np.array([0, 4, 8], dtype=np.uint64), np.zeros(2, dtype=np.int32)
        a, bad = C.c_void_p(), C.c_int(-1)
        args = lambda **kw: [kw.get("h", h._h), kw.get("b", blob.ctypes.data), kw.get("off", off.ctypes.data), kw.get("k", budget.ctypes.data),  # noqa: E731
                             kw.get("n", 2), 0, 0, kw.get("flags", 0), kw.get("a", C.byref(a)), kw.get("bad", C.byref(bad))]
        h.readPatternFromMemory(b"kept\n")
        assert lib.PFACX_editOpen(*args(h=None)) == BAD_HANDLE
        for null in ("b", "off", "k", "a"):
            assert lib.PFACX_editOpen(*args(**{null: None})) == INVALID, null
        assert lib.PFACX_editOpen(*args(n=0)) == INVALID and bad.value == 0, "numPatterns == 0"
        assert lib.PFACX_editOpen(*args(n=(1 << 31) - 1)) == INVALID and bad.value == 0, "numPatterns >= 2^31 - 1"
        for flags in (2, 3, 1 << 31):
            assert lib.PFACX_editOpen(*args(flags=flags)) == INVALID and not a.value, "an unknown flag bit"
        descending = np.array([0, 6, 4], dtype=np.uint64)
        assert lib.PFACX_editOpen(*args(off=descending.ctypes.data)) == INVALID and bad.value == 2, "an h_patOff that descends"
        assert int(h.match_host_array(np.frombuffer(b"kept", dtype=np.uint8))[0]) == 1, "a refusal leaves the handle's set alone"
        assert lib.PFACX_editOpen(*args(bad=None, flags=BEST)) == 0 and a.value, "badPattern may be null"
        assert lib.PFACX_editClose(a) == 0
        assert lib.PFACX_editClose(None) == BAD_HANDLE
    finally:
        h.destroy()


def test_the_getter_with_n_too_small_and_with_null_arrays():
    lib = api.load_library()
    patterns, budgets = [b"abcdefgh", b"abcdWXYZ0123", b"efghabcd"], [1, 2, 0]
    h = host_handle()
    try:
        with h.editOpen(patterns, budgets) as ed:
            want, pieces = ref.model_pieces(patterns, budgets)
            assert pieces == [b"abcd", b"efgh", b"WXYZ", b"0123", b"efghabcd"] and want[1].tolist() == [1, 2, 1, 3, 4, 5]
            E = 6
            off = np.full(5, 99, dtype=np.uint64)
            arrays = [np.full(E, -7, dtype=np.int32) for _ in range(3)]
            ptr = [a.ctypes.data for a in arrays]
            for given in ([0], [1], [2], [0, 1, 2]):                # n < the number of pieces with a per-piece array given: nothing is written
                use = [ptr[i] if i in given else None for i in range(3)]
                assert lib.PFACX_editGetPieces(ed._c, off.ctypes.data, *use, E - 1) == INVALID
            assert off.tolist() == [99] * 5 and all(np.all(a == -7) for a in arrays)
            assert lib.PFACX_editGetPieces(ed._c, off.ctypes.data, None, None, None, 0) == 0, "the offsets alone: n is not looked at"
            assert off.tolist() == want[0].tolist() == [0, 0, 2, 5, 6]
            for i in range(3):                                      # each array alone
                use = [ptr[j] if j == i else None for j in range(3)]
                assert lib.PFACX_editGetPieces(ed._c, None, *use, E) == 0
                assert arrays[i].tolist() == want[i + 1].tolist()
            assert lib.PFACX_editGetPieces(None, None, None, None, None, 0) == BAD_HANDLE
    finally:
        h.destroy()


def test_status_rows_and_the_stale_object():
    lib = api.load_library()
    h = host_handle()
    try:
        ed = h.editOpen([b"abcdefgh"], [1])
        data = np.frombuffer(b"abcdefgx", dtype=np.uint8).copy()
        ids, pos, end, dist = (np.full(8, -7, dtype=np.int32) for _ in range(4))
        n = C.c_size_t(99)
        call = lambda fn, size=8, cap=8, inp=data.ctypes.data, i=ids.ctypes.data, p=pos.ctypes.data, e=end.ctypes.data, d=dist.ctypes.data, num=C.byref(n): fn(  # noqa: E731
            ed._c, inp, size, i, p, e, d, cap, num)
        # abcdefg + x: D(7) = 1 (the h left out), D(8) = 1 (x for h)
        assert call(lib.PFACX_editMatchFromHost) == 0 and n.value == 2
        assert (ids[:2].tolist(), pos[:2].tolist(), end[:2].tolist(), dist[:2].tolist()) == ([1, 1], [0, 0], [7, 8], [1, 1])
        assert call(lib.PFACX_editMatchFromHost, size=0) == 0 and n.value == 0, "size == 0"
        assert call(lib.PFACX_editMatchFromHost, size=1 << 31) == INVALID, "size >= 2^31"
        assert call(lib.PFACX_editMatchFromHost, inp=None) == INVALID and call(lib.PFACX_editMatchFromHost, num=None) == INVALID
        assert call(lib.PFACX_editMatchFromHost, i=None) == INVALID and call(lib.PFACX_editMatchFromHost, p=None) == INVALID
        assert call(lib.PFACX_editMatchFromHost, e=None, d=None) == 0 and n.value == 2, "end and distance are optional"
        assert call(lib.PFACX_editMatchFromHost, cap=0, i=None, p=None, e=None, d=None) == TRUNCATED and n.value == 2, "the count query"
        assert call(lib.PFACX_editMatchFromDevice) == NOT_EXIST, "a device form on a host-only handle"
        assert call(lib.PFACX_editMatchFromDevice, cap=7) == INVALID, "capacity < size"
        assert lib.PFACX_editPairsFromDevice(ed._c, data.ctypes.data, 8, ids.ctypes.data, pos.ctypes.data, 1, None, None, None, None, 0,
                                             C.byref(n)) == NOT_EXIST
        assert lib.PFACX_editMatchFromHost(None, data.ctypes.data, 8, None, None, None, None, 0, C.byref(n)) == BAD_HANDLE
        h.readPatternFromMemory(b"a\n")                            # the handle reads another set: only the close call works
        assert call(lib.PFACX_editMatchFromHost) == INVALID and call(lib.PFACX_editMatchFromDevice) in (INVALID, NOT_EXIST)
        assert lib.PFACX_editGetPieces(ed._c, None, ids.ctypes.data, None, None, 8) == INVALID
        with pytest.raises(api.PFACError):
            ed.pieces()
        assert ed.close() == 0
        first = h.editOpen([b"abcd"], [0])                         # a second open replaces the set of the first
        second = h.editOpen([b"efgx"], [0])
        assert first.match_host(data.ctypes.data, 8, None, None, None, None, 0, check=False)[0] == INVALID
        assert second.match_host(data.ctypes.data, 8, None, None, None, None, 0, check=False) == (TRUNCATED, 1)
        assert first.close() == 0 and second.close() == 0
    finally:
        h.destroy()


def test_destroy_closes_the_object_and_the_handle_counts_no_device_tables():
    h = host_handle()
    ed = h.editOpen([b"abcdefgh"], [1])
    assert h.info().deviceTableBytes == 0, "a host-only handle uploads nothing"
    h.destroy()
    ed._c = C.c_void_p()                                        # PFAC_destroy closed it


# ---------------------------------------------------------------- the band, the exit, the bounds, ownership


@FLAGS
@pytest.mark.parametrize("k,length", ref.BAND, ids=[f"k{k}-L{n}" for k, n in ref.BAND])
def test_band_edges_with_k_and_k_plus_1_edits(k, length, flags):
    pattern = ref.edge_pattern(length)
    want = host_list([pattern], [k], ref.band_input(pattern, k), f"band k={k} L={length}", 1, 0, flags)
    assert (want[3] == k).sum() >= (4 if k and length > 2 * k else 1), "the variants with exactly k edits are occurrences"


@FLAGS
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_two_letter_inputs_where_best_alignments_miss_the_piece(seed, flags):
    rng = np.random.default_rng(seed)
    patterns = [bytes(rng.choice(np.frombuffer(b"ab", dtype=np.uint8), int(rng.integers(8, 17)))) for _ in range(6)]
    budgets = [min(k, len(p) // 2 - 1) for p, k in zip(patterns, [1, 2, 3, 1, 2, 3])]
    data = rng.choice(np.frombuffer(b"ab", dtype=np.uint8), 203)
    assert host_list(patterns, budgets, data, f"two letters {seed}", 2, 0, flags)[0].size > 20


@pytest.mark.parametrize("row", [4, 8, 12])
def test_the_deciding_edit_on_either_side_of_a_row_at_which_the_exit_is_tested(row):
    pattern = ref.edge_pattern(24)
    at = [row - 1, row, row + 1]
    texts = [ref.apply_edits(pattern, [("s", r - 1)]) for r in at] + [ref.apply_edits(pattern, [("s", 0), ("s", r - 1)]) for r in at]
    want = host_list([pattern], [1], b"....." + b"....".join(texts) + b".....", f"early exit at row {row}")
    assert want[3].tolist() == [1, 1, 1]


def test_starts_at_0_and_ends_at_n():
    pattern = ref.edge_pattern(12)
    for c in (1, 2, 3, 4):
        data = pattern[c:] + b"........" + pattern[:12 - c]
        got = set(rows(host_list([pattern], [2], data, f"bounds c={c}")))
        assert ((1, 0, 12 - c, c) in got) == (c <= 2) and ((1, len(data) - (12 - c), len(data), c) in got) == (c <= 2)


@pytest.mark.parametrize("exact", [(0,), (1,), (2,), (3,), (0, 1, 2, 3), (1, 3), (0, 2), (2, 3)], ids=lambda e: "pieces-" + "".join(map(str, e)))
def test_an_occurrence_is_listed_once_whichever_pieces_are_exact(exact):
    pattern = ref.edge_pattern(32)
    data = b"...." + ref.apply_edits(pattern, [("s", 8 * j + 5) for j in range(4) if j not in exact]) + b"...."
    got = rows(host_list([pattern], [3], data, f"exact pieces {exact}"))
    assert (1, 4, 36, 4 - len(exact)) in got and len({(r[0], r[2]) for r in got}) == len(got)


def test_a_periodic_input_in_which_one_piece_covers_an_end_from_two_positions():
    got = rows(host_list([b"abcabcabcabc"], [2], b".." + b"abc" * 7 + b"..", "periodic"))
    assert len({(r[0], r[2]) for r in got}) == len(got) and len(got) > 5


@pytest.mark.parametrize("kind", ["acgt", "text"])
def test_the_seeded_random_cases(kind):
    """the cases tests/test_edit_gpu.py runs: 100 patterns of 12 .. 150 letters with budgets 0 .. 3 over 32 KiB, each embedded with exactly k,
    k + 1 and 0 edits of all three kinds; both models agree as sets, the list has 100 .. 20 000 entries and holds every distance"""
    patterns, budgets, min_len, data, want = ref.random_case(kind)
    assert len(patterns) == 100 and data.size == 32 << 10 and set(budgets) == {0, 1, 2, 3}
    h = host_handle(api.PFAC_PLATFORM_CPU_OMP)
    try:
        with h.editOpen(patterns, budgets, min_len) as ed:
            check_getter(h, ed, patterns, budgets, min_len)
            ref.same(ed.match_host_array(data), want, f"random {kind}/host")
    finally:
        h.destroy()
