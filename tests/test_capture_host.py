"""PFACX_capturePairsFromHost and PFACX_matchCapturedFromHost (include/pfac_ext.h) on a host-only handle, no GPU needed: the hand-checked table and
random texts against tests/capture_ref.py, every status of the contract, PFACX_CAPTURE_AT_POS with null ids and without a pattern set, a caseless
handle, the cross-check against PFACX_splitFromHost, truncation with guard words around both arrays, and the four forms against each other (the two
device forms: tests/test_capture_gpu.py)."""

import numpy as np
import pytest

from pfac_amd import api
from tests import capture_ref as ref
from tests import split_ref

GUARD = -0x5A5A5A5B                       # no start, no length, not -1
PAD = 4                                   # guard words on each side of an output array
AT_POS = api.PFACX_CAPTURE_AT_POS

PATTERNS, LENS = ref.pattern_file(ref.KEYS)


def guarded(n):
    buf = np.full(n + 2 * PAD, GUARD, dtype=np.int32)
    return buf, buf.ctypes.data + 4 * PAD


def intact(buf, n):
    return bool(np.all(buf[:PAD] == GUARD) and np.all(buf[PAD + n:] == GUARD))


def capture_host(h, data, ids, positions, skip, stop, window, flags):
    """-> (status, valStart, valLen); checks the guards and that input and list are as they were"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    pos = np.ascontiguousarray(positions, dtype=np.int32)
    idv = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
    data0, pos0, ids0 = data.copy(), pos.copy(), None if idv is None else idv.copy()
    start, start_ptr = guarded(pos.size)
    length, length_ptr = guarded(pos.size)
    src = data if data.size else np.zeros(1, dtype=np.uint8)
    st = h.capturePairsFromHost(src.ctypes.data, data.size, skip, stop, window, flags, None if idv is None or not idv.size else idv.ctypes.data,
                                pos.ctypes.data if pos.size else None, pos.size, start_ptr, length_ptr, check=False)
    assert intact(start, pos.size) and intact(length, pos.size), "written outside an array"
    assert np.array_equal(data, data0) and np.array_equal(pos, pos0) and (idv is None or np.array_equal(idv, ids0)), "input and list are never written"
    return st, start[PAD:PAD + pos.size].copy(), length[PAD:PAD + pos.size].copy()


def check_against_reference(h, data, ids, positions, lens, skip, stop, window, flags):
    want = ref.capture(data, ids, positions, lens, skip, stop, window, flags)
    st, start, length = capture_host(h, data, ids, positions, skip, stop, window, flags)
    assert st == api.STATUS.SUCCESS
    assert np.array_equal(start, want[0]) and np.array_equal(length, want[1]), (skip, stop, window, flags)


@pytest.fixture(scope="module")
def bare():
    h = api.PFAC.createHostOnly()          # no pattern set: PFACX_CAPTURE_AT_POS needs none
    yield h
    h.destroy()


@pytest.fixture(scope="module")
def keyed():
    h = api.PFAC.createHostOnly()
    h.readPatternFromMemory(PATTERNS)
    yield h
    h.destroy()


@pytest.mark.parametrize("case", list(ref.table_cases()), ids=lambda c: "%s-%d-%d-%d" % (bytes(c[0][:4]).hex(), c[5], c[6], c[8].size))
def test_hand_table(bare, case):
    data, file, lens, skip, stop, window, flags, ids, pos, start, length = case
    h = bare
    if file is not None:
        h = api.PFAC.createHostOnly()
        h.readPatternFromMemory(file)
    st, got_start, got_length = capture_host(h, data, None if flags & AT_POS else ids, pos, skip, stop, window, flags)
    assert st == api.STATUS.SUCCESS
    assert got_start.tolist() == start.tolist() and got_length.tolist() == length.tolist()
    if file is not None:
        h.destroy()


def random_text(rng, size, skip, stop):
    """bytes in which skip bytes and stop bytes are frequent, singly and in runs"""
    pool = list(b"abcxyz=:0123") + list(skip or b"") * 3 + list(stop if stop is not None else b"\n") * 2
    return np.asarray(rng.choice(pool, size=size), dtype=np.uint8)


@pytest.mark.parametrize("skip,stop", [(None, None), (b" \t", b"\r\n"), (b" ", b";"), (b" ;", b";,"), (split_ref.FULL_CLASS, b""),
                                       (b"ab", bytes(range(56, 256)))])
def test_random_texts_equal_the_reference(keyed, skip, stop):
    rng = np.random.Generator(np.random.PCG64(3000 + len(skip or b"") + 7 * len(stop or b"")))
    for size in [1, 2, 3, 17, 255, 1000] + [int(s) for s in rng.integers(1, 3001, size=4)]:
        data = random_text(rng, size, skip, stop)
        pos = np.sort(rng.integers(-2, size + 2, size=max(1, size // 2))).astype(np.int32)      # duplicates, and both ends outside
        ids = rng.integers(0, len(LENS) + 1, size=pos.size).astype(np.int32)                    # 0 and F + 1 among them
        for window in (0, 1, 7, size, size + 100):
            check_against_reference(keyed, data, ids, pos, LENS, skip, stop, window, 0)
            check_against_reference(keyed, data, None, pos, None, skip, stop, window, AT_POS)


def test_at_pos_needs_neither_ids_nor_a_pattern_set(bare, keyed):
    data = np.frombuffer(ref.TEXT, dtype=np.uint8)
    pos = np.arange(-1, data.size + 2, dtype=np.int32)
    junk = np.full(pos.size, 99, dtype=np.int32)
    want = ref.capture(data, None, pos, None, b" ", b"\r\n", 0, AT_POS)
    for h, ids in ((bare, None), (bare, junk), (keyed, None), (keyed, junk)):
        st, start, length = capture_host(h, data, ids, pos, b" ", b"\r\n", 0, AT_POS)
        assert st == 0 and np.array_equal(start, want[0]) and np.array_equal(length, want[1]), "the ids are not read"
    assert want[0][0] == -1 and want[0][data.size + 1] == -1, "pos == n is outside"


def test_every_status(bare, keyed):
    data = np.frombuffer(ref.TEXT, dtype=np.uint8)
    ids = np.array([1, 2], dtype=np.int32)
    pos = np.array([0, 11], dtype=np.int32)
    start = np.zeros(2, dtype=np.int32)
    length = np.zeros(2, dtype=np.int32)
    bad = api.STATUS.INVALID_PARAMETER
    call = keyed.capturePairsFromHost
    good = (data.ctypes.data, data.size, None, None, 0, 0, ids.ctypes.data, pos.ctypes.data, 2, start.ctypes.data, length.ctypes.data)
    assert call(*good, check=False) == 0
    for flags in (2, 4, 3, 1 << 31):
        assert call(*good[:5], flags, *good[6:], check=False) == bad, "an unknown flag bit"
    assert call(None, *good[1:], check=False) == bad, "a null input"
    assert call(*good[:7], None, *good[8:], check=False) == bad, "a null list with pairs"
    assert call(*good[:9], None, good[10], check=False) == bad, "a null valStart with pairs"
    assert call(*good[:10], None, check=False) == bad, "a null valLen with pairs"
    assert call(*good[:6], None, *good[7:], check=False) == bad, "null ids without PFACX_CAPTURE_AT_POS"
    assert call(*good[:5], AT_POS, None, *good[7:], check=False) == 0, "null ids with it"
    assert call(good[0], 1 << 31, *good[2:], check=False) == bad, "size >= 2^31"
    assert call(*good[:8], 1 << 31, *good[9:], check=False) == bad, "numPairs >= 2^31"
    lib = api.load_library()
    assert lib.PFACX_capturePairsFromHost(None, *good[:2], None, None, 0, 0, *good[6:]) == bad, "a null handle"
    assert lib.PFACX_capturePairsFromDevice(None, *good[:2], None, None, 0, 0, *good[6:]) == bad
    # numPairs == 0 or size == 0: success, nothing is touched, null arrays are fine
    start[:] = GUARD
    assert call(*good[:6], None, None, 0, None, None, check=False) == 0
    assert call(good[0], 0, *good[2:], check=False) == 0 and np.all(start == GUARD)
    # no pattern set: only with PFACX_CAPTURE_AT_POS
    assert bare.capturePairsFromHost(*good, check=False) == api.STATUS.PATTERNS_NOT_READY
    assert bare.capturePairsFromHost(*good[:5], AT_POS, *good[6:], check=False) == 0
    # the device forms on a host-only handle
    assert keyed.capturePairsFromDevice(*good, check=False) == api.STATUS.LIB_NOT_EXIST
    assert bare.capturePairsFromDevice(*good[:5], AT_POS, *good[6:], check=False) == api.STATUS.LIB_NOT_EXIST
    # the scan forms: the checks of the reduce call, the flags, the output arrays
    all_ids = np.zeros(data.size, dtype=np.int32)
    all_pos = np.zeros(data.size, dtype=np.int32)
    scan = (data.ctypes.data, data.size, None, None, 0, 0, all_ids.ctypes.data, all_pos.ctypes.data, start.ctypes.data, length.ctypes.data, 2)
    assert bare.matchCapturedFromHost(*scan, check=False)[0] == api.STATUS.PATTERNS_NOT_READY
    assert bare.matchCapturedFromHost(*scan[:5], AT_POS, *scan[6:], check=False)[0] == api.STATUS.PATTERNS_NOT_READY, "the scan needs the set"
    assert keyed.matchCapturedFromHost(*scan, check=False)[0] in (0, api.STATUS.OUTPUT_TRUNCATED)
    assert keyed.matchCapturedFromHost(*scan[:5], 2, *scan[6:], check=False)[0] == bad
    for k in (0, 6, 7):
        assert keyed.matchCapturedFromHost(*scan[:k], None, *scan[k + 1:], check=False)[0] == bad, "a null input, ids or pos array"
    for k in (8, 9):
        assert keyed.matchCapturedFromHost(*scan[:k], None, *scan[k + 1:], check=False)[0] == bad, "a null output array with capCapacity > 0"
    assert keyed.matchCapturedFromHost(*scan[:8], None, None, 0, check=False) == (api.STATUS.OUTPUT_TRUNCATED, 4), "capCapacity 0: both may be null"
    assert keyed.matchCapturedFromHost(scan[0], 1 << 31, *scan[2:], check=False)[0] == bad
    assert keyed.matchCapturedFromDevice(*scan, check=False)[0] == api.STATUS.LIB_NOT_EXIST
    assert keyed.matchCapturedFromHost(scan[0], 0, *scan[2:], check=False) == (0, 0), "size == 0"
    n = api.C.c_int(0)
    assert lib.PFACX_matchCapturedFromHost(None, *scan[:2], None, None, 0, 0, *scan[6:], api.C.byref(n)) == api.STATUS.INVALID_HANDLE


def scan_captured(h, data, skip, stop, window, flags, capacity):
    data = np.ascontiguousarray(data, dtype=np.uint8).copy()
    data0 = data.copy()
    ids = np.full(data.size, GUARD, dtype=np.int32)
    pos = np.full(data.size, GUARD, dtype=np.int32)
    start, start_ptr = guarded(capacity)
    length, length_ptr = guarded(capacity)
    st, count = h.matchCapturedFromHost(data.ctypes.data, data.size, skip, stop, window, flags, ids.ctypes.data, pos.ctypes.data,
                                        start_ptr if capacity else None, length_ptr if capacity else None, capacity, check=False)
    assert intact(start, capacity) and intact(length, capacity), "written outside an array"
    assert np.array_equal(data, data0)
    return st, count, ids, pos, start[PAD:PAD + capacity].copy(), length[PAD:PAD + capacity].copy()


HEADERS = b"GET / HTTP/1.1\r\nHost:   example.org\r\nuser= bob \nContent-Length:\t42\r\nk=\r\nx=last"
HEADERS_UPPER = b"GET / HTTP/1.1\r\nHOST:   example.org\r\nUSER= bob \nContent-Length:\t42\r\nK=\r\nX=last"
HEADER_KEYS = [b"host:", b"user=", b"content-length:", b"k=", b"x="]


@pytest.mark.parametrize("nocase", [False, True])
def test_the_four_forms_agree(nocase):
    """the scan form is the reduce call, then the pairs form over its list; a caseless handle folds for the match and never for the classes"""
    file, lens = ref.pattern_file(HEADER_KEYS if nocase else [b"Host:", b"user=", b"Content-Length:", b"k=", b"x="])
    h = api.PFAC.createHostOnly()
    h.readPatternFromMemoryEx(file, api.PFACX_READ_NOCASE if nocase else 0)
    data = np.frombuffer(HEADERS_UPPER if nocase else HEADERS, dtype=np.uint8).copy()
    ids_w = np.zeros(data.size, dtype=np.int32)
    pos_w = np.zeros(data.size, dtype=np.int32)
    _, count_w = h.matchFromHostReduce(data.ctypes.data, data.size, ids_w.ctypes.data, pos_w.ctypes.data)
    assert count_w >= 5
    ids_w, pos_w = ids_w[:count_w], pos_w[:count_w]
    # 'E' and 'e' tell a folded class from the caller's: the text holds only the lower-case one behind the keys
    for skip, stop, window, flags in ((b" \t", b"\r\n", 0, 0), (None, None, 0, 0), (b" ", b"E", 0, 0), (b" ", b"e", 0, 0), (b" \t", b"\r\n", 3, 0),
                                      (b" \t", b"\r\n", 0, AT_POS)):
        want = ref.capture(data, ids_w, pos_w, lens, skip, stop, window, flags)
        st, start, length = capture_host(h, data, ids_w, pos_w, skip, stop, window, flags)
        assert st == 0 and np.array_equal(start, want[0]) and np.array_equal(length, want[1])
        for capacity in (0, count_w - 1, count_w, count_w + 2):
            st, count, ids, pos, start, length = scan_captured(h, data, skip, stop, window, flags, capacity)
            assert count == count_w, "the full count whatever the capacity"
            assert st == (api.STATUS.SUCCESS if capacity >= count_w else api.STATUS.OUTPUT_TRUNCATED)
            assert np.array_equal(ids[:count], ids_w) and np.array_equal(pos[:count], pos_w)
            kept = min(capacity, count_w)
            assert np.array_equal(start[:kept], want[0][:kept]) and np.array_equal(length[:kept], want[1][:kept])
            assert np.all(start[kept:] == GUARD) and np.all(length[kept:] == GUARD), "exactly the first capCapacity entries"
    by_upper = ref.capture(data, ids_w, pos_w, lens, b" ", b"E", 0, 0)
    by_lower = ref.capture(data, ids_w, pos_w, lens, b" ", b"e", 0, 0)
    assert not np.array_equal(by_upper[1], by_lower[1]), "the test text tells the two classes apart"
    want = ref.capture(data, ids_w, pos_w, lens, b" \t", b"\r\n", 0, 0)
    assert ref.values_text(data, want[0], want[1]) == b"example.org\nbob \n42\n\nlast\n"
    h.destroy()


@pytest.mark.parametrize("members", [1, 2, 40])
def test_the_value_ends_where_the_record_of_the_split_ends(members):
    """S empty, window 0, flags 0 on both calls: valStart + valLen = offsets[record + 1] - 1 where that byte is in D, else n -- the record of b"""
    rng = np.random.Generator(np.random.PCG64(4000 + members))
    h = api.PFAC.createHostOnly()
    h.readPatternFromMemory(PATTERNS)
    for size in (1, 2, 50, 1000, 4097):
        data, cls = split_ref.random_case(rng, size, members)
        offsets, _ = h.split_host_array(data, cls)
        offsets = offsets.astype(np.int64)
        pos = np.sort(rng.integers(0, size, size=max(1, size // 3))).astype(np.int32)
        ids = rng.integers(1, len(LENS), size=pos.size).astype(np.int32)
        st, start, length = capture_host(h, data, ids, pos, None, cls, 0, 0)
        assert st == 0
        b = np.minimum(pos.astype(np.int64) + np.asarray(LENS)[ids], size)
        assert np.array_equal(start, b), "nothing is skipped"
        table = split_ref.class_lookup(cls)
        for k in range(pos.size):
            end = size
            if b[k] < size:
                last = offsets[np.searchsorted(offsets, b[k], side="right")] - 1          # the last byte of the record of b
                end = int(last) if table[data[last]] else size
            assert int(start[k]) + int(length[k]) == end, (size, k)
    h.destroy()


def test_the_reference_assembles_the_text_of_the_values():
    data = np.frombuffer(ref.TEXT, dtype=np.uint8)
    ids = [i for i, _ in ref.KEY_PAIRS] + [9]
    pos = [p for _, p in ref.KEY_PAIRS] + [5]
    start, length = ref.capture(data, ids, pos, LENS, b" \t", b"\r\n", 0, 0)
    assert ref.values_text(data, start, length) == b"a.b\nbob\n\nv\n\n", "an empty value and an entry with valStart == -1: an empty line each"
