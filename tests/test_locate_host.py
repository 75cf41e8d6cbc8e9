"""PFACX_locatePairsFromHost and PFACX_matchLocatedFromHost (include/pfac_ext.h) on a host-only handle, no GPU needed: the hand-checked table and
random cases against tests/locate_ref.py (the offsets of the split and a searchsorted), every flag combination, the class extremes, the line
invariant against PFACX_matchLinesFromHost, the positions at the edges, every status of the contract, truncation with guard words around both
arrays, and the scan form's pairs against PFAC_matchFromHostReduce."""

import numpy as np
import pytest

from pfac_amd import api
from tests import locate_ref as ref
from tests import split_ref

GUARD = -0x5A5A5A5B                       # no record, no column, not -1
PAD = 4                                   # guard words on each side of an output array

PATTERNS = b"ab\nabc\nERROR\nxyz\nb\n"
TEXT = b"an ab here\nERROR abc\n\nxyz ab\nlast abc b"


def guarded(n):
    buf = np.full(n + 2 * PAD, GUARD, dtype=np.int32)
    return buf, buf.ctypes.data + 4 * PAD


def intact(buf, n):
    return bool(np.all(buf[:PAD] == GUARD) and np.all(buf[PAD + n:] == GUARD))


def locate_host(h, data, positions, cls, flags, column=True, want_records=True):
    """-> (status, records, columns or None, number of records); checks the guards and that input and list are as they were"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    pos = np.ascontiguousarray(positions, dtype=np.int32)
    data0, pos0 = data.copy(), pos.copy()
    rec, rec_ptr = guarded(pos.size)
    col, col_ptr = guarded(pos.size)
    src = data if data.size else np.zeros(1, dtype=np.uint8)
    st, n = h.locatePairsFromHost(src.ctypes.data, data.size, cls, flags, pos.ctypes.data if pos.size else None, pos.size, rec_ptr,
                                  col_ptr if column else None, want_records=want_records, check=False)
    assert intact(rec, pos.size) and intact(col, pos.size), "written outside an array"
    assert column or np.all(col == GUARD)
    assert np.array_equal(data, data0) and np.array_equal(pos, pos0), "input and list are never written"
    return st, rec[PAD:PAD + pos.size].copy(), col[PAD:PAD + pos.size].copy() if column else None, n


def check_against_reference(h, data, positions, cls, flags):
    record, column, segments = ref.locate(data, positions, cls, flags)
    st, rec, col, n = locate_host(h, data, positions, cls, flags)
    assert st == api.STATUS.SUCCESS and n == segments
    assert np.array_equal(rec, record) and np.array_equal(col, column)


@pytest.fixture(scope="module")
def handle():
    h = api.PFAC.createHostOnly()          # no pattern set: the pairs forms need none
    yield h
    h.destroy()


@pytest.fixture(scope="module")
def scanning():
    h = api.PFAC.createHostOnly()
    h.readPatternFromMemory(PATTERNS)
    yield h
    h.destroy()


@pytest.mark.parametrize("case", list(ref.table_cases()), ids=lambda c: "%s-%d-%d" % (bytes(c[0][:4]).hex(), c[2], c[3].size))
def test_hand_table(handle, case):
    data, cls, flags, positions, record, column, segments = case
    st, rec, col, n = locate_host(handle, data, positions, cls, flags)
    assert st == api.STATUS.SUCCESS and n == segments
    assert rec.tolist() == record.tolist() and col.tolist() == column.tolist()
    rec2, col2, n2 = handle.locate_host_array(data, positions, cls, before=bool(flags & ref.BEFORE), runs=bool(flags & ref.RUNS))
    assert np.array_equal(rec2, record) and np.array_equal(col2, column) and n2 == segments


@pytest.mark.parametrize("members", [1, 3, 128])
def test_random_cases_equal_the_reference_under_every_flag(handle, members):
    rng = np.random.Generator(np.random.PCG64(2000 + members))
    for size in [1, 2, 3, 17, 255, 256, 1000, 4097] + [int(s) for s in rng.integers(1, 5001, size=6)]:
        data, cls = split_ref.random_case(rng, size, members)
        some = np.sort(rng.integers(-2, size + 2, size=max(1, size // 3))).astype(np.int32)      # duplicates, and both ends outside
        for flags in ref.ALL_FLAGS:
            check_against_reference(handle, data, some, cls, flags)
            check_against_reference(handle, data, np.arange(size, dtype=np.int32), cls, flags)


def test_class_extremes_and_null_class(handle):
    data = np.frombuffer(TEXT, dtype=np.uint8)
    every = np.arange(data.size, dtype=np.int32)
    for flags in ref.ALL_FLAGS:
        st, rec, col, n = locate_host(handle, data, every, split_ref.EMPTY_CLASS, flags)
        assert (st, n) == (0, 1) and np.all(rec == 0) and np.array_equal(col, every), "an empty class: one record, column = p"
        check_against_reference(handle, data, every, split_ref.FULL_CLASS, flags)
        by_null = locate_host(handle, data, every, None, flags)
        by_newline = locate_host(handle, data, every, b"\n", flags)
        assert all(np.array_equal(x, y) for x, y in zip(by_null[1:3], by_newline[1:3])) and by_null[3] == by_newline[3]
    st, rec, col, n = locate_host(handle, data, every, split_ref.FULL_CLASS, 0)
    assert n == data.size and np.array_equal(rec, every) and np.all(col == 0), "a full class: every byte its own record"


def test_record_is_the_line_index_of_the_lines_call(scanning):
    data = np.frombuffer(TEXT, dtype=np.uint8).copy()
    ids = np.zeros(data.size, dtype=np.int32)
    pos = np.zeros(data.size, dtype=np.int32)
    _, count = scanning.matchFromHostReduce(data.ctypes.data, data.size, ids.ctypes.data, pos.ctypes.data)
    pos = pos[:count]
    assert count >= 8
    st, rec, col, n = locate_host(scanning, data, pos, None, 0)
    lines, start, length, index = scanning.match_lines_host_array(data)
    assert n == lines
    seen = 0
    for s, ln, k in zip(start, length, index):
        inside = (pos >= s) & (pos < s + ln)
        assert inside.any(), "a selected line holds a pair"
        assert np.all(rec[inside] == k) and np.array_equal(col[inside], pos[inside] - s)
        seen += int(inside.sum())
    assert seen == count, "every pair lies in a selected line"


def test_positions_at_the_edges(handle):
    data = np.frombuffer(b"abc\ndef\n", dtype=np.uint8)                    # delimiters at 3 and 7 = size - 1
    positions = [0, 0, 3, 3, 4, 4, 4, 7, 7]                                # the first byte, on a delimiter, the byte behind it, size - 1, duplicates
    st, rec, col, n = locate_host(handle, data, positions, None, 0)
    assert (st, n) == (0, 2)
    assert rec.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1] and col.tolist() == [0, 0, 3, 3, 0, 0, 0, 3, 3]
    for flags in ref.ALL_FLAGS:
        check_against_reference(handle, data, positions, None, flags)
        check_against_reference(handle, data, [-(1 << 31), -5, -1, 0, 7, 8, 9, (1 << 31) - 1], None, flags)     # -1 for p < 0 and p >= size


def test_optional_pointers_and_empty_calls(handle):
    data = np.frombuffer(b"abc\ndef\n", dtype=np.uint8)
    st, rec, col, n = locate_host(handle, data, [1, 5], None, 0, column=False)
    assert (st, n) == (0, 2) and rec.tolist() == [0, 1] and col is None
    st, rec, col, n = locate_host(handle, data, [1, 5], None, 0, want_records=False)
    assert st == 0 and rec.tolist() == [0, 1] and col.tolist() == [1, 1]
    # numPairs == 0: nothing is touched, the count is still written; null arrays are fine
    st, n = handle.locatePairsFromHost(data.ctypes.data, data.size, None, 0, None, 0, None, None)
    assert (st, n) == (0, 2)
    st, n = handle.locatePairsFromHost(data.ctypes.data, data.size, b"c", api.PFACX_SPLIT_BEFORE, None, 0, None, None)
    assert (st, n) == (0, 2)
    assert handle.locatePairsFromHost(data.ctypes.data, data.size, None, 0, None, 0, None, None, want_records=False)[0] == 0
    # size == 0: success, 0 records, nothing is touched even with pairs
    st, rec, col, n = locate_host(handle, np.zeros(0, dtype=np.uint8), [0, 1], None, 0)
    assert (st, n) == (0, 0) and np.all(rec == GUARD) and np.all(col == GUARD)


def test_every_invalid_parameter(handle):
    data = np.frombuffer(b"abc\ndef\n", dtype=np.uint8)
    pos = np.array([1, 5], dtype=np.int32)
    rec = np.zeros(2, dtype=np.int32)
    col = np.zeros(2, dtype=np.int32)
    bad = api.STATUS.INVALID_PARAMETER
    call = handle.locatePairsFromHost
    good = (data.ctypes.data, data.size, None, 0, pos.ctypes.data, 2, rec.ctypes.data, col.ctypes.data)
    assert call(*good, check=False)[0] == 0
    for flags in (4, 8, 1 << 31, 7):
        assert call(*good[:3], flags, *good[4:], check=False)[0] == bad, "an unknown flag bit"
    assert call(None, *good[1:], check=False)[0] == bad, "a null input"
    assert call(*good[:4], None, *good[5:], check=False)[0] == bad, "a null list with pairs"
    assert call(*good[:6], None, good[7], check=False)[0] == bad, "a null record array with pairs"
    assert call(good[0], 1 << 31, *good[2:], check=False)[0] == bad, "size >= 2^31"
    assert call(*good[:5], 1 << 31, *good[6:], check=False)[0] == bad, "numPairs >= 2^31"
    lib = api.load_library()
    n = api.C.c_size_t(0)
    assert lib.PFACX_locatePairsFromHost(None, *good[:2], None, 0, *good[4:], api.C.byref(n)) == bad, "a null handle"
    assert lib.PFACX_locatePairsFromDevice(None, *good[:2], None, 0, *good[4:], api.C.byref(n)) == bad
    # the device form on a host-only handle
    assert handle.locatePairsFromDevice(*good, check=False)[0] == api.STATUS.LIB_NOT_EXIST
    # the scan forms: the checks of the reduce call, and the flags
    ids = np.zeros(data.size, dtype=np.int32)
    p2 = np.zeros(data.size, dtype=np.int32)
    scan = (data.ctypes.data, data.size, None, 0, ids.ctypes.data, p2.ctypes.data, rec.ctypes.data, col.ctypes.data, 2)
    assert handle.matchLocatedFromHost(*scan, check=False)[0] == api.STATUS.PATTERNS_NOT_READY
    h = api.PFAC.createHostOnly()
    h.readPatternFromMemory(PATTERNS)
    assert h.matchLocatedFromHost(*scan, check=False)[0] in (0, api.STATUS.OUTPUT_TRUNCATED)
    assert h.matchLocatedFromHost(*scan[:3], 4, *scan[4:], check=False)[0] == bad
    for k in (0, 4, 5):
        assert h.matchLocatedFromHost(*scan[:k], None, *scan[k + 1:], check=False)[0] == bad, "a null input, ids or pos array"
    assert h.matchLocatedFromHost(*scan[:6], None, *scan[7:], check=False)[0] == bad, "a null record array with locCapacity > 0"
    assert h.matchLocatedFromHost(scan[0], 1 << 31, *scan[2:], check=False)[0] == bad
    assert h.matchLocatedFromDevice(*scan, check=False)[0] == api.STATUS.LIB_NOT_EXIST
    assert h.matchLocatedFromHost(scan[0], 0, *scan[2:], check=False) == (0, 0), "size == 0"
    h.destroy()


def scan_located(h, data, cls, flags, capacity, column=True):
    data = np.ascontiguousarray(data, dtype=np.uint8).copy()
    data0 = data.copy()
    ids = np.full(data.size, GUARD, dtype=np.int32)
    pos = np.full(data.size, GUARD, dtype=np.int32)
    rec, rec_ptr = guarded(capacity)
    col, col_ptr = guarded(capacity)
    st, count = h.matchLocatedFromHost(data.ctypes.data, data.size, cls, flags, ids.ctypes.data, pos.ctypes.data, rec_ptr if capacity else None,
                                       col_ptr if column and capacity else None, capacity, check=False)
    assert intact(rec, capacity) and intact(col, capacity), "written outside an array"
    assert np.array_equal(data, data0)
    return st, count, ids, pos, rec[PAD:PAD + capacity].copy(), col[PAD:PAD + capacity].copy()


@pytest.mark.parametrize("nocase", [False, True])
def test_scan_form_equals_reduce_then_locate(nocase):
    h = api.PFAC.createHostOnly()
    h.readPatternFromMemoryEx(PATTERNS, api.PFACX_READ_NOCASE if nocase else 0)
    data = np.frombuffer(b"An AB here\nerror ABC\n\nxyz ab\nLAST abc B" if nocase else TEXT, dtype=np.uint8).copy()
    ids_w = np.zeros(data.size, dtype=np.int32)
    pos_w = np.zeros(data.size, dtype=np.int32)
    _, count_w = h.matchFromHostReduce(data.ctypes.data, data.size, ids_w.ctypes.data, pos_w.ctypes.data)
    assert count_w >= 8
    # a caseless handle folds for the match and never for the class: 'A' cuts at 'A' only
    for cls, flags in ((None, 0), (b"A", 0), (b"a ", ref.RUNS), (b"\n", ref.BEFORE)):
        record, column, _ = ref.locate(data, pos_w[:count_w], cls, flags)
        for capacity in (0, count_w - 1, count_w, count_w + 2):
            st, count, ids, pos, rec, col = scan_located(h, data, cls, flags, capacity)
            assert count == count_w, "the full count whatever the capacity"
            assert st == (api.STATUS.SUCCESS if capacity >= count_w else api.STATUS.OUTPUT_TRUNCATED)
            assert np.array_equal(ids[:count], ids_w[:count_w]) and np.array_equal(pos[:count], pos_w[:count_w])
            kept = min(capacity, count_w)
            assert np.array_equal(rec[:kept], record[:kept]) and np.array_equal(col[:kept], column[:kept])
            assert np.all(rec[kept:] == GUARD) and np.all(col[kept:] == GUARD), "exactly the first locCapacity entries"
    st, count, ids, pos, rec, col = scan_located(h, data, None, 0, count_w, column=False)
    assert st == 0 and np.all(col == GUARD) and np.array_equal(rec, ref.locate(data, pos_w[:count_w], None, 0)[0])
    if nocase:
        upper = ref.locate(data, pos_w[:count_w], b"A", 0)[0]
        lower = ref.locate(data, pos_w[:count_w], b"a", 0)[0]
        assert not np.array_equal(upper, lower), "the test text tells the two classes apart"
    h.destroy()
