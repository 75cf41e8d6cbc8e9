"""PFACX_splitFromHost (include/pfac_ext.h) on a host-only handle, no GPU needed: the table and random cases against tests/split_ref.py,
truncation at every capacity that matters with guard words around the array, every status of the contract, the line invariant against
PFACX_matchLinesFromHost, and the batch calls over the offsets it returns."""

import ctypes

import numpy as np
import pytest

from pfac_amd import api
from tests import split_ref as ref

GUARD = 0xA5A5A5A5A5A5A5A5
PAD = 4                                   # guard words on each side of an offsets array


def guarded(capacity):
    """an array of `capacity` offsets between guard words -> (the whole buffer, the pointer to entry 0)"""
    buf = np.full(capacity + 2 * PAD, GUARD, dtype=np.uint64)
    return buf, buf.ctypes.data + 8 * PAD


def split_host(h, data, cls, flags, capacity, null_array=False):
    """-> (status, segments, longest, the entries the call had room for); checks the guards and that the input is as it was"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    before = data.copy()
    buf, ptr = guarded(capacity)
    src = data if data.size else np.zeros(1, dtype=np.uint8)
    st, segments, longest = h.splitFromHost(src.ctypes.data, data.size, cls, flags, None if null_array else ptr, capacity, check=False)
    assert np.all(buf[:PAD] == GUARD) and np.all(buf[PAD + capacity:] == GUARD), "written outside the array"
    assert np.array_equal(data, before), "the input is never written"
    return st, segments, longest, buf[PAD:PAD + capacity].copy()


def check_against_reference(h, data, cls, flags):
    want, segments, longest = ref.split(data, cls, flags)
    st, n, most, got = split_host(h, data, cls, flags, want.size + 3)
    assert st == api.STATUS.SUCCESS
    assert (n, most) == (segments, longest)
    assert np.array_equal(got[:want.size], want)
    assert np.all(got[want.size:] == GUARD), "nothing behind the closing entry"


@pytest.fixture(scope="module")
def handle():
    h = api.PFAC.createHostOnly()          # no pattern set: the call needs none
    yield h
    h.destroy()


@pytest.mark.parametrize("case", list(ref.table_cases()), ids=lambda c: c[0])
def test_table(handle, case):
    _, data, cls, flags, want, segments, longest = case
    st, n, most, got = split_host(handle, data, cls, flags, want.size + 2)
    assert st == api.STATUS.SUCCESS
    assert (n, most) == (segments, longest)
    assert np.array_equal(got[:want.size], want) and np.all(got[want.size:] == GUARD)
    offsets, most2 = handle.split_host_array(data, cls, before=bool(flags & ref.BEFORE), runs=bool(flags & ref.RUNS))
    assert offsets.dtype == np.uint64 and np.array_equal(offsets, want) and most2 == longest


@pytest.mark.parametrize("members", [1, 3, 128])
def test_random_cases_equal_the_reference(handle, members):
    rng = np.random.Generator(np.random.PCG64(1000 + members))
    for size in [0, 1, 2, 3, 17, 255, 256, 1000, 4097, 5000] + [int(s) for s in rng.integers(0, 5001, size=10)]:
        data, cls = ref.random_case(rng, size, members)
        for flags in ref.ALL_FLAGS:
            check_against_reference(handle, data, cls, flags)


def test_default_class_is_the_newline(handle):
    data = np.frombuffer(b"one\ntwo\n\nthree", dtype=np.uint8)
    for flags in ref.ALL_FLAGS:
        a = split_host(handle, data, None, flags, 16)
        b = split_host(handle, data, b"\n", flags, 16)
        assert a[:3] == b[:3] and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("flags", ref.ALL_FLAGS)
def test_truncation(handle, flags):
    rng = np.random.Generator(np.random.PCG64(77))
    data, cls = ref.random_case(rng, 3000, 3)
    want, segments, longest = ref.split(data, cls, flags)
    assert segments > 8
    for capacity in (0, 1, segments // 2, segments, segments + 1):
        st, n, most, got = split_host(handle, data, cls, flags, capacity, null_array=capacity == 0)
        assert (n, most) == (segments, longest), "the full values whatever the capacity"
        assert st == (api.STATUS.SUCCESS if capacity >= segments + 1 else api.STATUS.OUTPUT_TRUNCATED)
        assert np.array_equal(got, want[:capacity]), "exactly the first `capacity` entries"
    # h_longest may be null
    st, n, most = handle.splitFromHost(data.ctypes.data, data.size, cls, flags, None, 0, want_longest=False, check=False)
    assert (st, n, most) == (api.STATUS.OUTPUT_TRUNCATED, segments, 0)


def test_statuses(handle, workloads):
    lib = api.load_library()
    S = api.STATUS
    data = np.frombuffer(b"a\nb\n", dtype=np.uint8)
    buf, ptr = guarded(8)
    n = ctypes.c_size_t(99)
    args = (data.ctypes.data, data.size, None, 0, ptr, 8, ctypes.byref(n), None)
    raw = handle._h
    assert lib.PFACX_splitFromHost(raw, *args) == S.SUCCESS and n.value == 2
    assert lib.PFACX_splitFromHost(raw, data.ctypes.data, data.size, None, 4, ptr, 8, ctypes.byref(n), None) == S.INVALID_PARAMETER     # an unknown flag bit
    assert lib.PFACX_splitFromHost(raw, data.ctypes.data, data.size, None, 0x80000000, ptr, 8, ctypes.byref(n), None) == S.INVALID_PARAMETER
    for mis in (1, 2, 4, 7):                                                                                  # a misaligned offsets array
        assert lib.PFACX_splitFromHost(raw, data.ctypes.data, data.size, None, 0, ptr + mis, 4, ctypes.byref(n), None) == S.INVALID_PARAMETER
    assert lib.PFACX_splitFromHost(None, *args) == S.INVALID_PARAMETER                                     # null pointers
    assert lib.PFACX_splitFromHost(raw, None, data.size, None, 0, ptr, 8, ctypes.byref(n), None) == S.INVALID_PARAMETER
    assert lib.PFACX_splitFromHost(raw, data.ctypes.data, data.size, None, 0, ptr, 8, None, None) == S.INVALID_PARAMETER
    assert lib.PFACX_splitFromHost(raw, data.ctypes.data, data.size, None, 0, None, 1, ctypes.byref(n), None) == S.INVALID_PARAMETER     # a null array with capacity > 0
    assert lib.PFACX_splitFromDevice(None, *args) == S.INVALID_PARAMETER
    assert lib.PFACX_splitFromDevice(raw, data.ctypes.data, data.size, None, 4, ptr, 8, ctypes.byref(n), None) == S.INVALID_PARAMETER
    assert lib.PFACX_splitFromDevice(raw, data.ctypes.data, data.size, None, 0, ptr + 4, 8, ctypes.byref(n), None) == S.INVALID_PARAMETER
    assert np.all(buf[:PAD] == GUARD) and np.all(buf[PAD + 3:] == GUARD)
    # size 0: success, 0 segments, the longest 0, nothing written
    st, segments, longest, got = split_host(handle, np.zeros(0, dtype=np.uint8), None, 0, 4)
    assert (st, segments, longest) == (S.SUCCESS, 0, 0) and np.all(got == GUARD)
    # the device form on a host-only handle, behind the argument checks; size 0 needs no device
    assert handle.splitFromDevice(data.ctypes.data, data.size, None, 0, ptr, 8, check=False)[0] == S.LIB_NOT_EXIST
    assert handle.splitFromDevice(data.ctypes.data, 0, None, 0, ptr, 8, check=False) == (S.SUCCESS, 0, 0)
    # a handle with a pattern set, and a caseless one: the same answers ('A' in the class does not cut at 'a')
    for flags in (0, api.PFACX_READ_NOCASE):
        h = api.PFAC.createHostOnly()
        h.readPatternFromFileEx(workloads["c1"].pattern_file, flags)
        text = np.frombuffer(b"xAyaz", dtype=np.uint8)
        assert h.split_host_array(text, b"A")[0].tolist() == [0, 2, 5]
        h.destroy()


@pytest.mark.parametrize("name", ["c3", "c1"])
def test_line_invariant(workloads, name):
    """flags 0, the default class: the segments are the lines of PFACX_matchLines* with their newlines"""
    w = workloads[name]
    h = api.PFAC.createHostOnly()
    h.readPatternFromFile(w.pattern_file)
    tail = np.frombuffer(b"\nlast line without a newline", dtype=np.uint8)
    for data in (w.data[:200000], np.concatenate([w.data[:5000], tail]), np.frombuffer(b"\n\n", dtype=np.uint8)):
        lines, start, _, _ = h.match_lines_host_array(data)
        lines2, start2, _, _ = h.match_lines_host_array(data, invert=True)
        assert lines == lines2
        offsets, _ = h.split_host_array(data)
        assert np.array_equal(offsets[:-1], np.sort(np.concatenate([start, start2])).astype(np.uint64))
        assert offsets.size - 1 == lines
    h.destroy()


def test_composition_with_the_batch_calls():
    data, patterns, (rule_off, rule_patterns) = ref.make_log()
    h = api.PFAC.createHostOnly()
    h.readPatternFromMemory(patterns)
    rules = h.rulesOpen(rule_off, rule_patterns)
    for flags in ref.ALL_FLAGS:
        want = ref.split(data, None, flags)[0]
        got, _ = h.split_host_array(data, None, before=bool(flags & ref.BEFORE), runs=bool(flags & ref.RUNS))
        assert got.size > 100
        a, b = h.count_batch_host_array(data, got), h.count_batch_host_array(data, want)
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3] and a[3] > 0
        c, d = rules.match_host_array(data, got), rules.match_host_array(data, want)
        assert all(np.array_equal(x, y) for x, y in zip(c, d)) and c[0].size > 0
    rules.close()
    h.destroy()
