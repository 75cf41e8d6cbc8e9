"""PFACX_countBatchFromHost on the CPU platforms and on host-only handles (no device needed) against the two references of tests/segcount_ref.py:
every case under every segmentation, nocase, duplicate lines, offsets == NULL, truncation inside a segment and at a segment border, the count query,
size == 0, every refused argument with its status, the device forms on a host-only handle, the total against PFACX_countFromHost over the segments.
All arrays are poisoned and carry guard words on both sides."""

import ctypes as C

import numpy as np
import pytest

from pfac_amd import api
from tests import allmatch_ref as am
from tests import segcount_ref as ref
from tests.segcount_ref import test_the_two_segment_references_agree_on_every_case  # noqa: F401  (runs here: segcount_ref.py is not collected)
from tests.spans_helpers import pattern_file

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
INVALID, NOT_READY, NOT_EXIST, TRUNCATED = (api.STATUS.INVALID_PARAMETER, api.STATUS.PATTERNS_NOT_READY, api.STATUS.LIB_NOT_EXIST,
                                            api.STATUS.OUTPUT_TRUNCATED)
LONGEST, ACCUMULATE = api.PFACX_COUNT_LONGEST, api.PFACX_COUNT_ACCUMULATE
GUARD = 8
POISON, POISON32 = 0xDEADBEEFDEADBEEF, 0xDEADBEEF


def host_handle(pf, platform=api.PFAC_PLATFORM_CPU, flags=0):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    h.readPatternFromFileEx(pf, flags)
    return h


def host_list(h, data, offsets, flags=0, capacity=None):
    """countBatchFromHost over poisoned arrays with GUARD words on both sides -> (status, (segFirst, ids, counts), entries, total).  capacity None:
    the count query first, with null arrays, as a caller would.  The guards and the input must stay as they were"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    n = buf.size
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uintp)
    segs = 1 if off is None else off.size - 1
    first = np.full(GUARD + segs + 1 + GUARD, POISON, dtype=np.uintp)
    I, O, F = buf.ctypes.data if n else first.ctypes.data, None if off is None else off.ctypes.data, first.ctypes.data + 8 * GUARD
    if capacity is None:
        st, capacity, total0 = h.countBatchFromHost(I, n, O, segs, flags, None, None, 0, F, check=False)
        assert st in (0, TRUNCATED) and (st == TRUNCATED) == (capacity > 0)
        first[:] = POISON
    ids = np.full(GUARD + capacity + GUARD, -7, dtype=np.int32)
    counts = np.full(GUARD + capacity + GUARD, POISON32, dtype=np.uint32)
    st, entries, total = h.countBatchFromHost(I, n, O, segs, flags, ids.ctypes.data + 4 * GUARD, counts.ctypes.data + 4 * GUARD, capacity, F, check=False)
    k = min(entries, capacity)
    assert np.all(ids[:GUARD] == -7) and np.all(ids[GUARD + k:] == -7), "wrote outside the list or behind capacity"
    assert np.all(counts[:GUARD] == POISON32) and np.all(counts[GUARD + k:] == POISON32), "wrote outside the list or behind capacity"
    assert np.all(first[:GUARD] == POISON) and np.all(first[GUARD + segs + 1:] == POISON), "wrote outside segFirst"
    assert buf.tobytes() == bytes(data), "the caller's input was modified"
    return st, (first[GUARD:GUARD + segs + 1].copy(), ids[GUARD:GUARD + k].copy(), counts[GUARD:GUARD + k].copy()), entries, total


def check_host(h, want, data, offsets, flags, what):
    st, got, entries, total = host_list(h, data, offsets, flags)
    assert st == 0 and entries == want[1].size, f"{what}: status {st}, {entries} entries, want {want[1].size}"
    ref.same(got, want, what)
    assert total == int(want[2].sum(dtype=np.uint64)), f"{what}: the total"


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_equals_both_references(workdir, case, platform, pname):
    name, pats, data, offsets = case
    nocase = ref.is_nocase(name)
    folded = [ref.fold(p) for p in pats] if nocase else pats
    prefix, chain, _ = am.prefix_table(folded)
    seg_result = ref.brute_seg_result(pats, data, offsets, nocase)
    h = host_handle(pattern_file(workdir, "segcount_" + name.replace("/", "_"), pats), platform, api.PFACX_READ_NOCASE if nocase else 0)
    try:
        for longest in (False, True):
            want = ref.segcounts_py(pats, data, offsets, nocase, longest)
            check_host(h, want, data, offsets, LONGEST if longest else 0, f"{name}/{pname}/longest {longest}")
            ref.same(ref.segcounts_from_result(seg_result, offsets, (prefix, chain), longest), want, f"{name}/the second reference")
            first, ids, counts, total = h.count_batch_host_array(np.frombuffer(data, dtype=np.uint8), offsets, longest)
            ref.same((first, ids, counts), want, f"{name}/count_batch_host_array")
            # the sum of the counts is what PFACX_countFromHost adds over the segments, one by one
            each = [h.count_host_array(np.frombuffer(data[offsets[k]:offsets[k + 1]], dtype=np.uint8), longest)[1] for k in range(len(offsets) - 1)]
            assert total == sum(each), f"{name}/{pname}: *h_total against count_host_array over the segments"
    finally:
        h.destroy()


def test_offsets_null_is_one_segment(workdir):
    pats = [b"ab", b"abc", b"b"]
    data = b"abc ab b"
    h = host_handle(pattern_file(workdir, "segcount_null", pats))
    try:
        for longest in (False, True):
            want = ref.segcounts_py(pats, data, None, longest=longest)
            check_host(h, want, data, None, LONGEST if longest else 0, f"offsets NULL/longest {longest}")
        first, ids, counts, total = h.count_batch_host_array(np.frombuffer(data, dtype=np.uint8))
        assert (first.tolist(), ids.tolist(), counts.tolist(), total) == ([0, 3], [1, 2, 3], [2, 1, 3], 6)
    finally:
        h.destroy()


@pytest.mark.parametrize("platform,pname", PLATFORMS)
def test_truncation_inside_a_segment_at_a_border_and_the_count_query(workdir, platform, pname):
    data, offsets = b"a" * 20 + b"b" + b"a" * 3, [0, 10, 10, 21, 24]
    want = ref.segcounts_py(ref.NESTED, data, offsets)
    n = want[1].size
    assert want[0].tolist() == [0, 8, 8, 16, 19]
    h = host_handle(pattern_file(workdir, "segcount_trunc", ref.NESTED), platform)
    try:
        for cap in (0, 1, 5, 8, 16, n - 1, n, n + 3):                        # 5: inside segment 0; 8 and 16: exactly at a border
            st, got, entries, total = host_list(h, data, offsets, 0, capacity=cap)
            assert (st, entries, total) == (TRUNCATED if cap < n else 0, n, int(want[2].sum())), f"{pname}/capacity {cap}"
            ref.same(got, (want[0], want[1][:cap], want[2][:cap]), f"{pname}/capacity {cap}")
        first = np.full(5, POISON, dtype=np.uintp)
        buf = np.frombuffer(data, dtype=np.uint8).copy()
        off = np.array(offsets, dtype=np.uintp)
        assert h.countBatchFromHost(buf.ctypes.data, buf.size, off.ctypes.data, 4, 0, None, None, 0, first.ctypes.data, check=False) == \
            (TRUNCATED, n, int(want[2].sum())), "the count query: null arrays, everything else complete"
        assert first.tolist() == want[0].tolist()
    finally:
        h.destroy()


def test_size_zero(workdir):
    h = host_handle(pattern_file(workdir, "segcount_zero", [b"ab", b"cd"]))
    try:
        for offsets in ([0, 0, 0, 0], None):
            st, got, entries, total = host_list(h, b"", offsets, capacity=4)
            assert (st, entries, total) == (0, 0, 0) and not got[0].any() and got[1].size == 0
        lib = api.load_library()
        n, t = C.c_size_t(5), C.c_ulonglong(5)
        byte = np.zeros(1, dtype=np.uint8)
        assert lib.PFACX_countBatchFromHost(h._h, byte.ctypes.data, 0, byte.ctypes.data, 0, 0, None, None, 0, None, C.byref(n), C.byref(t)) == 0
        assert (n.value, t.value) == (0, 0), "no segments and no bytes: success, segFirst not needed"
    finally:
        h.destroy()


def test_every_refused_argument_with_its_status(workdir):
    pf = pattern_file(workdir, "segcount_errors", [b"ab", b"cd"])
    data = np.frombuffer(b"ab.cd.", dtype=np.uint8).copy()
    n = data.size
    off = np.array([0, 3, 6], dtype=np.uintp)
    ids = np.full(8, -7, dtype=np.int32)
    counts = np.full(8, POISON32, dtype=np.uint32)
    first = np.full(3 + GUARD, POISON, dtype=np.uintp)
    pair_first = np.array([0, 1, 2], dtype=np.int32)
    I, O, D, K, F, P = data.ctypes.data, off.ctypes.data, ids.ctypes.data, counts.ctypes.data, first.ctypes.data, pair_first.ctypes.data
    lib = api.load_library()
    h = host_handle(pf)
    try:
        call = lambda *a: h.countBatchFromHost(*a, check=False)[0]  # noqa: E731
        assert call(I, n, O, 2, ACCUMULATE, D, K, 8, F) == INVALID, "PFACX_COUNT_ACCUMULATE"
        assert call(I, n, O, 2, LONGEST | ACCUMULATE, D, K, 8, F) == INVALID
        assert call(I, n, O, 2, 4, D, K, 8, F) == INVALID and call(I, n, O, 2, 0x80000000, D, K, 8, F) == INVALID, "an unknown flag bit"
        for broken in ([1, 3, 6], [0, 3, 5], [0, 3, 7], [0, 4, 3], [0, 7, 6]):
            bad = np.array(broken, dtype=np.uintp)
            assert call(I, n, bad.ctypes.data, 2, 0, D, K, 8, F) == INVALID, f"offsets {broken}"
        assert call(None, n, O, 2, 0, D, K, 8, F) == INVALID
        assert call(I, n, O, 2, 0, None, K, 8, F) == INVALID and call(I, n, O, 2, 0, D, None, 8, F) == INVALID
        assert call(I, n, O, 2, 0, D, K, 8, None) == INVALID, "segFirst is the row pointer: required"
        assert call(I, n, None, 2, 0, D, K, 8, F) == INVALID, "offsets NULL with numSegments != 1"
        assert call(I, n, O, 0, 0, D, K, 8, F) == INVALID, "numSegments == 0 with size > 0"
        assert call(I, 1 << 31, O, 2, 0, D, K, 8, F) == INVALID and call(I, n, O, 1 << 31, 0, D, K, 8, F) == INVALID
        nn, tt = C.c_size_t(5), C.c_ulonglong(5)
        assert lib.PFACX_countBatchFromHost(h._h, I, n, O, 2, 0, D, K, 8, F, None, C.byref(tt)) == INVALID
        assert lib.PFACX_countBatchFromHost(h._h, I, n, O, 2, 0, D, K, 8, F, C.byref(nn), None) == INVALID
        # the device forms on a host-only handle, behind their argument checks
        assert h.countBatchFromDevice(I, n, O, 2, 0, D, K, 8, F, check=False)[0] == NOT_EXIST
        assert h.countBatchFromDevice(I, 0, O, 2, 0, D, K, 8, F, check=False)[0] == NOT_EXIST
        assert h.countBatchPairsFromDevice(D, 2, P, 2, 0, D, K, 8, F, check=False)[0] == NOT_EXIST
        assert h.countBatchPairsFromDevice(None, 0, P, 2, 0, D, K, 8, F, check=False)[0] == NOT_EXIST
        assert h.countBatchFromDevice(I, n, O, 2, ACCUMULATE, D, K, 8, F, check=False)[0] == INVALID
        assert h.countBatchFromDevice(I, n, O, 2, 0, D, K, 8, None, check=False)[0] == INVALID
        assert h.countBatchPairsFromDevice(D, 2, P, 2, 2, D, K, 8, F, check=False)[0] == INVALID
        assert h.countBatchPairsFromDevice(None, 2, P, 2, 0, D, K, 8, F, check=False)[0] == INVALID
        assert h.countBatchPairsFromDevice(D, 1 << 31, P, 2, 0, D, K, 8, F, check=False)[0] == INVALID
        assert h.countBatchPairsFromDevice(D, 2, None, 2, 0, D, K, 8, F, check=False)[0] == INVALID
        assert np.all(ids == -7) and np.all(counts == POISON32) and np.all(first == POISON) and (nn.value, tt.value) == (5, 5), "a refused call wrote"
        assert bytes(data) == b"ab.cd."
        assert h.countBatchFromHost(I, n, O, 2, 0, D, K, 8, F) == (0, 2, 2)
        assert (ids[:2].tolist(), counts[:2].tolist(), first[:3].tolist()) == ([1, 2], [1, 1], [0, 1, 2]) and np.all(first[3:] == POISON)
    finally:
        h.destroy()
    bare = api.PFAC.createHostOnly()
    try:
        assert bare.countBatchFromHost(I, n, O, 2, 0, D, K, 8, F, check=False)[0] == NOT_READY
        assert bare.countBatchFromHost(I, 0, None, 1, 0, D, K, 8, F, check=False)[0] == NOT_READY
    finally:
        bare.destroy()
    nn, tt = C.c_size_t(0), C.c_ulonglong(0)
    for fn in (lib.PFACX_countBatchFromHost, lib.PFACX_countBatchFromDevice):
        assert fn(None, I, n, O, 2, 0, D, K, 8, F, C.byref(nn), C.byref(tt)) == api.STATUS.INVALID_HANDLE
    assert lib.PFACX_countBatchPairsFromDevice(None, D, 2, P, 2, 0, D, K, 8, F, C.byref(nn), C.byref(tt)) == api.STATUS.INVALID_HANDLE


def test_the_three_sizes_are_exported():
    """(their values are pinned through behaviour: the window, touched-list and trip cases of tests/test_segcount_gpu.py are built from them)"""
    assert (api.PFACX_SEGCOUNT_WINDOW, api.PFACX_SEGCOUNT_TOUCHED, api.PFACX_SEGCOUNT_BLOCK_PAIRS) == (8192, 1024, 256)
