"""PFACX_coverSpansFromHost (host-only handles: no device needed) against the two models of tests/cover_ref.py, which share no code with the
library or with each other: every single interval over a size of 70 with ends and with lengths, hostile entries, duplicates, nesting and touching
pairs, the alternating list at its bound, 200 seeded lists in three orders, truncation at every capacity around the list with guard words, the
count query, empty calls, every refusal, and the cross-checks against PFACX_matchSpansFromHost and through PFACX_clsigMatchFromHost with
Python's re.  Every comparison is exact; the interval arrays must stay untouched."""

import ctypes as C
import re

import numpy as np
import pytest

from pfac_amd import api
from tests import cover_ref as ref

INVALID, NOT_EXIST, TRUNCATED, BAD_HANDLE = (api.STATUS.INVALID_PARAMETER, api.STATUS.LIB_NOT_EXIST, api.STATUS.OUTPUT_TRUNCATED,
                                             api.STATUS.INVALID_HANDLE)
LENGTHS = api.PFACX_COVER_LENGTHS
GUARD = 16
POISON = -7


@pytest.fixture(scope="module")
def handle():
    h = api.PFAC.createHostOnly()
    yield h
    h.destroy()


def host_cover(h, starts, second, size, lengths=False, capacity=None):
    """coverSpansFromHost into poisoned arrays of `capacity` entries (default: the full length, asked for first) with GUARD poisoned entries on
    both sides of each -> (status, (starts, lengths, covered) written, the number of spans); nothing else may change, nor the intervals"""
    a = np.ascontiguousarray(starts, dtype=np.int32)
    b = np.ascontiguousarray(second, dtype=np.int32)
    a_before, b_before, n = a.copy(), b.copy(), int(a.size)
    flags = LENGTHS if lengths else 0
    pa, pb = (a.ctypes.data, b.ctypes.data) if n else (None, None)
    if capacity is None:
        st, capacity, covered = h.coverSpansFromHost(pa, pb, n, size, flags, None, None, 0, check=False)
        assert st in (0, TRUNCATED) and (st == TRUNCATED) == (capacity > 0)
    out = [np.full(GUARD + capacity + GUARD, POISON, dtype=np.int32) for _ in range(2)]
    ptr = [o.ctypes.data + 4 * GUARD if capacity else None for o in out]
    st, spans, covered = h.coverSpansFromHost(pa, pb, n, size, flags, ptr[0], ptr[1], capacity, check=False)
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (spans > capacity), (st, spans, capacity)
    k = min(spans, capacity)
    for o in out:
        assert np.all(o[:GUARD] == POISON) and np.all(o[GUARD + capacity:] == POISON), "wrote outside the arrays"
        assert np.all(o[GUARD + k:GUARD + capacity] == POISON), "wrote behind the list"
    assert np.array_equal(a, a_before) and np.array_equal(b, b_before), "the interval arrays were modified"
    return st, (out[0][GUARD:GUARD + k].copy(), out[1][GUARD:GUARD + k].copy(), covered), spans


def check(h, starts, second, size, lengths, what):
    want = ref.model(starts, second, size, lengths)
    st, got, spans = host_cover(h, starts, second, size, lengths)
    assert st == 0 and spans == len(want[0]), what
    ref.same(got, want, what)
    return want


# ---------------------------------------------------------------- 1. every single interval


@pytest.mark.parametrize("lengths", [False, True], ids=["ends", "lengths"])
def test_every_single_interval_over_70_bytes(handle, lengths):
    size, cases = 70, 0
    for s in range(size + 1):
        for e in range(size + 1):
            second = e - s if lengths else e
            st, got, spans = host_cover(handle, [s], [second], size, lengths, capacity=2)
            want = ([s], [e - s], e - s) if s < e and s < size else ([], [], 0)
            assert st == 0 and spans == len(want[0]), (s, e)
            assert (got[0].tolist(), got[1].tolist(), got[2]) == want, (s, e)
            cases += 1
    assert cases == 71 * 71
    for s, e in ((0, 70), (69, 70), (35, 35), (40, 30), (70, 70)):         # ... and the models say the same of a few of them
        check(handle, [s], [e - s if lengths else e], size, lengths, (s, e))


# ---------------------------------------------------------------- 2. hostile entries, shapes, the bound


@pytest.mark.parametrize("case", ref.HOSTILE, ids=[c[0] for c in ref.HOSTILE])
def test_hostile_entries_are_clamped(handle, case):
    name, starts, second, lengths = case
    check(handle, starts, second, ref.HOSTILE_SIZE, lengths, name)


def test_hostile_entries_by_hand(handle):
    size = ref.HOSTILE_SIZE
    for starts, second, lengths, want in (
            ([-5], [7], False, ([0], [7], 7)), ([90], [250], False, ([90], [10], 10)), ([ref.INT_MIN], [ref.INT_MAX], False, ([0], [100], 100)),
            ([50], [ref.INT_MAX], True, ([50], [50], 50)), ([ref.INT_MAX], [ref.INT_MAX], True, ([], [], 0)), ([50], [-10], True, ([], [], 0)),
            ([-5], [10], True, ([0], [5], 5)), ([-5], [5], True, ([], [], 0)), ([100], [130], False, ([], [], 0)), ([60], [20], False, ([], [], 0))):
        st, got, spans = host_cover(handle, starts, second, size, lengths)
        assert st == 0 and (got[0].tolist(), got[1].tolist(), got[2]) == want, (starts, second, lengths)


@pytest.mark.parametrize("case", ref.SHAPES, ids=[c[0] for c in ref.SHAPES])
def test_duplicates_nesting_touching_and_overlap(handle, case):
    name, starts, ends = case
    check(handle, starts, ends, ref.SHAPES_SIZE, False, name)
    check(handle, starts, ref.as_lengths(starts, ends), ref.SHAPES_SIZE, True, name + "/lengths")


def test_touching_intervals_are_one_span_and_a_gap_of_one_is_two(handle):
    _, got, spans = host_cover(handle, [3, 8], [8, 11], 64)
    assert spans == 1 and (got[0].tolist(), got[1].tolist(), got[2]) == ([3], [8], 8)
    _, got, spans = host_cover(handle, [3, 9], [8, 11], 64)
    assert spans == 2 and (got[0].tolist(), got[1].tolist(), got[2]) == ([3, 9], [5, 2], 7)


def test_word_edge_table_written_out_by_hand(handle):
    for intervals, want in ref.EDGE_TABLE:
        starts, ends = [s for s, _ in intervals], [e for _, e in intervals]
        st, got, spans = host_cover(handle, starts, ends, ref.EDGE_SIZE)
        assert st == 0 and list(zip(got[0].tolist(), got[1].tolist())) == want and got[2] == sum(n for _, n in want), intervals
        ref.model(starts, ends, ref.EDGE_SIZE)


@pytest.mark.parametrize("size", [1, 2, 63, 64, 65, 1000, 1001])
def test_alternating_list_reaches_the_bound(handle, size):
    starts, ends = ref.alternating(size)
    want = check(handle, starts, ends, size, False, size)
    assert len(want[0]) == (size + 1) // 2 and want[2] == (size + 1) // 2


# ---------------------------------------------------------------- 3. seeded lists in three orders


@pytest.mark.parametrize("block", range(10))
def test_seeded_lists_ascending_descending_and_shuffled(handle, block):
    for seed in ref.RANDOM_SEEDS[20 * block:20 * block + 20]:
        starts, ends, size = ref.random_list(seed)
        want = ref.model(starts, ends, size)
        order = np.argsort(np.array(starts), kind="stable")
        shuffled = np.random.RandomState(seed + 1000).permutation(len(starts))
        for name, idx in (("given", np.arange(len(starts))), ("ascending", order), ("descending", order[::-1]), ("shuffled", shuffled)):
            s, e = [starts[i] for i in idx], [ends[i] for i in idx]
            st, got, spans = host_cover(handle, s, e, size)
            assert st == 0 and spans == len(want[0])
            ref.same(got, want, f"seed {seed}/{name}")
        lens = ref.as_lengths(starts, ends)
        st, got, _ = host_cover(handle, starts, lens, size, lengths=True)
        ref.same(got, want, f"seed {seed}/lengths")


# ---------------------------------------------------------------- 4. capacity


def test_truncation_at_every_capacity_around_the_list(handle):
    starts, ends = [40, 3, 90, 20, 3, 60, 21], [45, 8, 99, 22, 5, 61, 30]
    want = ref.model(starts, ends, 100)
    spans = len(want[0])
    assert spans == 5
    for capacity in (0, 1, spans - 1, spans, spans + 1):
        st, got, total = host_cover(handle, starts, ends, 100, capacity=capacity)
        assert total == spans and got[2] == want[2], "both counts are complete whatever the capacity"
        assert st == (TRUNCATED if capacity < spans else 0)
        k = min(capacity, spans)
        assert got[0].tolist() == want[0][:k].tolist() and got[1].tolist() == want[1][:k].tolist()


def test_count_query_with_null_arrays(handle):
    a, b = np.array([5, 50], dtype=np.int32), np.array([9, 70], dtype=np.int32)
    st, spans, covered = handle.coverSpansFromHost(a.ctypes.data, b.ctypes.data, 2, 100, 0, None, None, 0, check=False)
    assert (st, spans, covered) == (TRUNCATED, 2, 24)
    st, spans, covered = handle.coverSpansFromHost(a.ctypes.data, b.ctypes.data, 2, 4, 0, None, None, 0, check=False)
    assert (st, spans, covered) == (0, 0, 0)


def test_no_intervals_and_no_size(handle):
    out = [np.full(4, POISON, dtype=np.int32) for _ in range(2)]
    st, spans, covered = handle.coverSpansFromHost(None, None, 0, 100, 0, out[0].ctypes.data, out[1].ctypes.data, 4, check=False)
    assert (st, spans, covered) == (0, 0, 0) and all(np.all(o == POISON) for o in out)
    a, b = np.array([0], dtype=np.int32), np.array([5], dtype=np.int32)
    st, spans, covered = handle.coverSpansFromHost(a.ctypes.data, b.ctypes.data, 1, 0, 0, out[0].ctypes.data, out[1].ctypes.data, 4, check=False)
    assert (st, spans, covered) == (0, 0, 0) and all(np.all(o == POISON) for o in out)
    starts, lens, cb = handle.cover_spans_host_array([], [], 10)
    assert starts.size == 0 and lens.size == 0 and cb == 0


def test_array_wrapper(handle):
    starts, lens, cb = handle.cover_spans_host_array([7, 1, 2], [9, 2, 4], 10)
    assert (starts.tolist(), lens.tolist(), cb) == ([1, 7], [3, 2], 5)
    starts, lens, cb = handle.cover_spans_host_array([7, 1, 2], [2, 1, 2], 10, lengths=True)
    assert (starts.tolist(), lens.tolist(), cb) == ([1, 7], [3, 2], 5)


# ---------------------------------------------------------------- 5. refusals, handles


def test_every_refusal(handle):
    lib = api.load_library()
    a, b = np.array([1, 5], dtype=np.int32), np.array([3, 9], dtype=np.int32)
    out = [np.full(4, POISON, dtype=np.int32) for _ in range(2)]
    ns, cb = C.c_size_t(77), C.c_size_t(77)
    pa, pb, po, pl = a.ctypes.data, b.ctypes.data, out[0].ctypes.data, out[1].ctypes.data

    def call(h, start, end, n, size, flags, span_start, span_len, capacity, p_ns, p_cb):
        return lib.PFACX_coverSpansFromHost(h, start, end, n, size, flags, span_start, span_len, capacity, p_ns, p_cb)

    H, NS, CB = handle._h, C.byref(ns), C.byref(cb)
    assert call(None, pa, pb, 2, 10, 0, po, pl, 4, NS, CB) == BAD_HANDLE
    assert call(H, pa, pb, 2, 10, 0, po, pl, 4, None, CB) == INVALID, "a null span count"
    assert call(H, pa, pb, 2, 10, 0, po, pl, 4, NS, None) == INVALID, "a null byte count"
    assert call(H, None, pb, 2, 10, 0, po, pl, 4, NS, CB) == INVALID, "null starts with intervals"
    assert call(H, pa, None, 2, 10, 0, po, pl, 4, NS, CB) == INVALID, "null ends with intervals"
    assert call(H, pa, pb, 2, 10, 0, None, pl, 4, NS, CB) == INVALID, "a null span array with a capacity"
    assert call(H, pa, pb, 2, 10, 0, po, None, 4, NS, CB) == INVALID, "a null length array with a capacity"
    assert call(H, pa, pb, 2, 2 ** 31, 0, po, pl, 4, NS, CB) == INVALID, "size 2^31"
    assert call(H, pa, pb, 2 ** 31, 10, 0, po, pl, 4, NS, CB) == INVALID, "2^31 intervals"
    for flags in (2, 3, 4, 0x80000000):
        assert call(H, pa, pb, 2, 10, flags, po, pl, 4, NS, CB) == INVALID, flags
    assert (ns.value, cb.value) == (77, 77) and all(np.all(o == POISON) for o in out), "a refused call wrote something"
    assert call(H, pa, pb, 2, 2 ** 31 - 1, 0, po, pl, 4, NS, CB) == 0 and (ns.value, cb.value) == (2, 6), "size 2^31 - 1 is legal"


@pytest.mark.parametrize("platform", [api.PFAC_PLATFORM_GPU, api.PFAC_PLATFORM_CPU, api.PFAC_PLATFORM_CPU_OMP])
def test_host_only_handle_on_every_platform_and_without_a_pattern_set(platform):
    h = api.PFAC.createHostOnly()
    try:
        h.setPlatform(platform, check=False)
        check(h, [30, 2, 4], [40, 6, 5], 50, False, platform)
        out = [np.full(4, POISON, dtype=np.int32) for _ in range(2)]
        a, b = np.array([1], dtype=np.int32), np.array([3], dtype=np.int32)
        st, _, _ = h.coverSpansFromDevice(a.ctypes.data, b.ctypes.data, 1, 10, 0, out[0].ctypes.data, out[1].ctypes.data, 4, check=False)
        assert st == NOT_EXIST, "the device form on a host-only handle"
    finally:
        h.destroy()


# ---------------------------------------------------------------- 6. against the library's own calls

def prefix_handle_and_text(seed, size):
    h = api.PFAC.createHostOnly()
    h.setPlatform(api.PFAC_PLATFORM_CPU)
    h.readPatternFromMemory(b"".join(p + b"\n" for p in ref.PREFIX_PATTERNS))
    return h, ref.prefix_text(seed, size)


def test_same_spans_as_match_spans_from_the_all_match_list():
    h, data = prefix_handle_and_text(11, 3000)
    try:
        pos, ids = h.match_all_host_array(data)
        assert pos.size > 500 and len(set(ids.tolist())) == len(ref.PREFIX_PATTERNS)
        ends = pos + np.array([len(ref.PREFIX_PATTERNS[i - 1]) for i in ids.tolist()], dtype=np.int32)
        want = h.match_spans_host_array(data)
        st, got, spans = host_cover(h, pos, ends, data.size)
        assert st == 0 and spans == want[0].size
        ref.same(got, want, "matchSpans")
        ref.same(got, ref.model(pos.tolist(), ends.tolist(), data.size), "models")
        shuffled = np.random.RandomState(5).permutation(pos.size)
        ref.same(host_cover(h, pos[shuffled], ends[shuffled], data.size)[1], want, "matchSpans/shuffled")
    finally:
        h.destroy()


def test_redaction_through_clsig_equals_re_sub():
    text = ref.token_text(2026, 4096)
    h = api.PFAC.createHostOnly()
    h.setPlatform(api.PFAC_PLATFORM_CPU)
    try:
        with h.clsigOpenText(b"".join(r + b"\n" for r in ref.CLSIG_RULES)) as sg:
            pos, ids, end = sg.match_host_array(np.frombuffer(text, dtype=np.uint8))
        assert pos.size >= 30 and set(ids.tolist()) == {1, 2, 3}
        st, got, spans = host_cover(h, pos, end, len(text))
        assert st == 0
        ref.same(got, ref.model(pos.tolist(), end.tolist(), len(text)), "models over the library's list")
        redacted = np.frombuffer(text, dtype=np.uint8).copy()
        for s, n in zip(got[0].tolist(), got[1].tolist()):
            redacted[s:s + n] = ord("#")
        want = text
        for rule in ref.CLSIG_RULES:                                # no match of one rule overlaps one of another: their alphabets' literals differ
            want = re.sub(rule, lambda m: b"#" * (m.end() - m.start()), want, flags=re.DOTALL)
        assert redacted.tobytes() == want and want.count(b"#") == got[2]
    finally:
        h.destroy()
