"""PFACX_locatePairsFromDevice and PFACX_matchLocatedFromDevice (include/pfac_ext.h; scan_locate.hip) on the GPU.  Every result is compared with
tests/locate_ref.py AND with a searchsorted over the offsets that PFACX_splitFromDevice writes for the same buffer, class and flags, so the two calls
cannot drift apart.  Every call: guard words on both sides of both output arrays, the input and the list unmodified."""

import numpy as np
import pytest
import torch                              # before the library loads its HIP runtime, as in every GPU test module

from pfac_amd import api  # noqa: E402
from tests import locate_ref as ref  # noqa: E402
from tests import split_ref  # noqa: E402

pytestmark = pytest.mark.gpu

T = api.PFACX_SPLIT_TILE
GUARD = -0x5A5A5A5B                       # no record, no column, not -1
PAD = 4                                   # guard words on each side of an output array
EDGE = 32                                 # bytes in front of and behind the input

PATTERNS = b"ab\nabc\nERROR\nxyz\nb\n"


@pytest.fixture(scope="module")
def handle():
    assert torch.cuda.is_available(), "GPU tests need a device; there is no CPU fallback to test"
    torch.cuda.set_device(0)
    h = api.PFAC.create()                  # no pattern set: the pairs form needs none
    yield h
    h.destroy()


def on_device(data, mis=0):
    """the bytes at an address that is `mis` mod 16, delimiters of most classes here around them -> (the whole buffer, the input's view)"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    whole = torch.full((EDGE + 16 + data.size + EDGE,), 0x0A, dtype=torch.uint8, device="cuda:0")
    view = whole[EDGE + mis:EDGE + mis + data.size]
    view.copy_(torch.from_numpy(data.copy()))
    assert view.data_ptr() % 16 == mis
    return whole, view


def guarded(n):
    return torch.full((n + 2 * PAD,), GUARD, dtype=torch.int32, device="cuda:0")


def inner(buf, n):
    got = buf.cpu().numpy()
    assert np.all(got[:PAD] == GUARD) and np.all(got[PAD + n:] == GUARD), "written outside an array"
    return got[PAD:PAD + n].copy()


def locate_device(h, view, size, positions, cls, flags, column=True):
    """-> (status, records, columns, number of records); the guards and the list checked"""
    pos = np.ascontiguousarray(positions, dtype=np.int32)
    d_pos = torch.from_numpy(pos.copy()).to("cuda:0")
    rec, col = guarded(pos.size), guarded(pos.size)
    st, n = h.locatePairsFromDevice(view.data_ptr(), size, cls, flags, d_pos.data_ptr(), pos.size, rec.data_ptr() + 4 * PAD,
                                    col.data_ptr() + 4 * PAD if column else None, check=False)
    torch.cuda.synchronize()
    assert np.array_equal(d_pos.cpu().numpy(), pos), "the list is never written"
    return st, inner(rec, pos.size), inner(col, pos.size), n


def by_split_offsets(h, view, size, positions, cls, flags):
    """what a caller does without the call: PFACX_splitFromDevice's own offsets of the same buffer, then a searchsorted"""
    _, segments, _ = h.splitFromDevice(view.data_ptr(), size, cls, flags, None, 0, check=False)
    off = torch.zeros(segments + 1, dtype=torch.int64, device="cuda:0")
    st, n, _ = h.splitFromDevice(view.data_ptr(), size, cls, flags, off.data_ptr(), segments + 1)
    assert (st, n) == (0, segments)
    off = off.cpu().numpy()
    pos = np.asarray(positions, dtype=np.int64)
    inside = (pos >= 0) & (pos < size)
    record = np.full(pos.size, -1, dtype=np.int32)
    column = np.full(pos.size, -1, dtype=np.int32)
    r = np.searchsorted(off, pos[inside], side="right") - 1
    record[inside] = r
    column[inside] = pos[inside] - off[r]
    return record, column, segments


def check(h, data, positions, cls, flags, mis=0, device=None):
    whole, view = device if device is not None else on_device(data, mis)
    want = ref.locate(data, positions, cls, flags)
    split = by_split_offsets(h, view, data.size, positions, cls, flags)
    st, rec, col, n = locate_device(h, view, data.size, positions, cls, flags)
    assert st == api.STATUS.SUCCESS
    for record, column, segments in (want, split):
        assert n == segments
        assert np.array_equal(rec, record), np.nonzero(rec != record)[0][:8]
        assert np.array_equal(col, column), np.nonzero(col != column)[0][:8]
    back = whole.cpu().numpy()
    lo = EDGE + mis
    assert np.array_equal(back[lo:lo + data.size], data) and np.all(back[:lo] == 0x0A) and np.all(back[lo + data.size:] == 0x0A), "the input is never written"


def text_with(n, delimiters, byte=ord("\n")):
    data = np.full(n, ord("x"), dtype=np.uint8)
    at = np.asarray([p for p in delimiters if 0 <= p < n], dtype=np.int64)
    data[at] = byte
    return data


def test_hand_table(handle):
    for data, cls, flags, positions, record, column, segments in ref.table_cases():
        check(handle, data, positions, cls, flags, 3)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, T - 1, T, T + 1, 5 * T + 17])
def test_size_edges(handle, n):
    """every position of inputs that end around every edge of the cut code, delimiters around the same edges and at random"""
    rng = np.random.Generator(np.random.PCG64(n))
    data = text_with(n, [0, 1, 15, 16, 1023, 1024, 4095, 4096, T - 1, T, n - 2, n - 1] + rng.integers(0, n, size=n // 50).tolist())
    device = on_device(data, 5)
    every = np.arange(n, dtype=np.int32)
    for flags in ref.ALL_FLAGS:
        check(handle, data, every, None, flags, 5, device)
    check(handle, data, every, b"\n;", 0, 5, device)                       # ... and through the class table in LDS


@pytest.mark.parametrize("mis", range(1, 16))
def test_pointer_alignment(handle, mis):
    n = 2 * T + 37
    rng = np.random.Generator(np.random.PCG64(100 + mis))
    data, cls = split_ref.random_case(rng, n, 1)
    positions = np.sort(rng.integers(0, n, size=500)).astype(np.int32)
    device = on_device(data, mis)
    for flags in (0, ref.RUNS | ref.BEFORE):
        check(handle, data, positions, cls, flags, mis, device)


EDGES = (16, 1024, 4096, T)               # behind a lane's 16 bytes, a trip, a region, a tile


def test_delimiters_at_every_edge(handle):
    """delimiters exactly at the last byte of a lane's 16, of a trip, of a region and of a tile, and at the first byte behind each"""
    n = 2 * T + 5
    data = text_with(n, [e - 1 for e in EDGES] + list(EDGES) + [T + e - 1 for e in EDGES[:3]] + [T + e for e in EDGES[:3]])
    every = np.arange(n, dtype=np.int32)
    for mis in (0, 9):
        device = on_device(data, mis)
        for flags in ref.ALL_FLAGS:
            check(handle, data, every, None, flags, mis, device)


@pytest.mark.parametrize("flags", [ref.RUNS, ref.RUNS | ref.BEFORE])
def test_runs_across_every_edge(handle, flags):
    n = 2 * T + 5
    runs = [(e - 2, e + 1) for e in EDGES] + [(T + 4094, T + 4097), (2 * T - 3, 2 * T + 4)]             # the last one to the input's end
    data = text_with(n, [p for lo, hi in runs for p in range(lo, hi + 1)], ord(";"))
    every = np.arange(n, dtype=np.int32)
    check(handle, data, every, b";", flags, 7)
    data[runs[0][0]] = ord(",")                                            # the same run out of two members of a class
    check(handle, data, every, b";,", flags, 2)


def test_pair_placement(handle):
    """pairs at the first and last byte of a tile and of a word of the bitmap, on a cut and one byte in front of it"""
    n = 3 * T + 100
    cuts_at = [64, 127, 128, T - 1, T, T + 63, T + 64, 2 * T + 1000]
    data = text_with(n, [c - 1 for c in cuts_at])                          # flags 0: the cut is the byte behind the delimiter
    positions = sorted({p for c in cuts_at for p in (c - 1, c, c + 1)} | {0, 63, 64, T - 1, T, 2 * T - 1, 2 * T, 2 * T + 63, 2 * T + 64, n - 1})
    for flags in ref.ALL_FLAGS:
        check(handle, data, positions, None, flags, 1)


def test_carried_start_across_tiles_without_a_cut(handle):
    """three tiles without any cut between two that have cuts, pairs only in the last: the start comes from the prefix maximum"""
    n = 5 * T
    data = text_with(n, [100, T - 7, 4 * T + 5000, 4 * T + 9000])
    in_last = [4 * T, 4 * T + 1, 4 * T + 4999, 4 * T + 5000, 4 * T + 5001, 4 * T + 8999, 4 * T + 9001, n - 1]
    for flags in ref.ALL_FLAGS:
        check(handle, data, in_last, None, flags, 0)
    check(handle, data, [3 * T + 17, 4 * T - 1], None, 0, 0)              # ... and a tile that has no cut of its own at all
    check(handle, text_with(n, [T - 1]), [T, 3 * T, n - 1], None, 0, 0)   # a cut at a tile's first byte, from the byte in front of the tile


def test_tiles_without_pairs_between_tiles_with_pairs(handle):
    n = 6 * T + 11
    rng = np.random.Generator(np.random.PCG64(6))
    data, cls = split_ref.random_case(rng, n, 3)
    positions = np.sort(np.concatenate([rng.integers(0, T, size=40), rng.integers(2 * T, 3 * T, size=40), rng.integers(5 * T, n, size=40)]))
    for flags in ref.ALL_FLAGS:
        check(handle, data, positions, cls, flags, 4)


def test_more_pairs_in_a_tile_than_the_block_has_threads(handle):
    """a tile where every position is a pair, 16 384 of them, and the same list with every entry doubled"""
    n = 3 * T
    rng = np.random.Generator(np.random.PCG64(7))
    data, cls = split_ref.random_case(rng, n, 1)
    every = np.arange(T, 2 * T, dtype=np.int32)
    device = on_device(data, 0)
    for flags in (0, ref.RUNS):
        check(handle, data, every, cls, flags, 0, device)
        check(handle, data, np.repeat(every, 2), cls, flags, 0, device)


def test_no_cut_anywhere(handle):
    n = 3 * T + 5
    data = np.full(n, ord("x"), dtype=np.uint8)
    positions = [0, 1, T - 1, T, 2 * T + 77, n - 1]
    for flags in ref.ALL_FLAGS:
        check(handle, data, positions, None, flags, 3)
    whole, view = on_device(data, 3)
    st, rec, col, n_records = locate_device(handle, view, n, positions, None, 0)
    assert (st, n_records) == (0, 1) and np.all(rec == 0) and col.tolist() == positions


def test_list_ends_out_of_range(handle):
    n = 2 * T + 9
    rng = np.random.Generator(np.random.PCG64(8))
    data, cls = split_ref.random_case(rng, n, 1)
    device = on_device(data, 0)
    for positions in ([-5, 0, 17, n - 1], [0, T, n - 1, n, n + 3], [-5, -5, -1, T + 1, n, n + 3, (1 << 31) - 1], [-5, -1], [n, n + 3]):
        check(handle, data, positions, cls, 0, 0, device)


@pytest.mark.parametrize("flags", [0, ref.RUNS | ref.BEFORE])
def test_more_tiles_than_one_step_of_the_one_block_passes(handle, flags):
    """1025 tiles, just over 16 MiB: one more than pfac_array_scan and pfac_locate_carry take per step.  Sparse cuts and pairs; the last cut in
    front of the step's edge is carried into the tile behind it"""
    assert api.PFACX_LOCATE_CARRY_STEP == api.PFACX_SPLIT_SCAN_STEP == 1024
    n = 1024 * T + 100
    rng = np.random.Generator(np.random.PCG64(9))
    delimiters = [p for p in np.sort(rng.integers(0, n, size=300)).tolist() if not 1021 * T + 50 <= p < n] + [1021 * T + 49]
    data = text_with(n, delimiters)
    positions = np.sort(np.concatenate([rng.integers(0, n, size=400), [1023 * T + 5, 1024 * T - 1, 1024 * T, 1024 * T + 1, n - 1]]))
    check(handle, data, positions, None, flags, 6)


def test_a_list_that_is_not_sorted_stays_inside_its_arrays(handle):
    """the contract's bounds for a bad list: success, values unspecified, the guard words around both outputs intact (inner() checks them)"""
    n = 3 * T + 5
    rng = np.random.Generator(np.random.PCG64(10))
    data, cls = split_ref.random_case(rng, n, 1)
    whole, view = on_device(data, 0)
    for positions in (rng.integers(-10, n + 10, size=5000), np.arange(n - 1, -1, -97), [2 * T + 1, 5, -3, T, n + 7, 0, T]):
        st, rec, col, n_records = locate_device(handle, view, n, positions, cls, 0)
        assert st == api.STATUS.SUCCESS and n_records == ref.locate(data, [], cls, 0)[2]


@pytest.mark.parametrize("nocase", [False, True])
def test_scan_form(nocase):
    line = b"An AB here\nerror ABC\n\nxyz ab\nLAST abc B\n" if nocase else b"an ab here\nERROR abc\n\nxyz ab\nlast abc b\n"
    data = np.frombuffer(line * 900, dtype=np.uint8).copy()               # more than two tiles
    h = api.PFAC.create()
    h.readPatternFromMemoryEx(PATTERNS, api.PFACX_READ_NOCASE if nocase else 0)
    whole, view = on_device(data, 3)
    n = data.size
    ids_w = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    pos_w = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    _, count_w = h.matchFromDeviceReduce(view.data_ptr(), n, ids_w.data_ptr(), pos_w.data_ptr())
    torch.cuda.synchronize()
    ids_w, pos_w = ids_w.cpu().numpy()[:count_w], pos_w.cpu().numpy()[:count_w]
    assert count_w > 5000
    for cls, flags in ((None, 0), (b"A", ref.BEFORE)):                     # a caseless handle never folds the class
        record, column, _ = ref.locate(data, pos_w, cls, flags)
        for capacity in (0, count_w - 1, count_w):
            ids = torch.full((n,), GUARD, dtype=torch.int32, device="cuda:0")
            pos = torch.full((n,), GUARD, dtype=torch.int32, device="cuda:0")
            rec, col = guarded(capacity), guarded(capacity)
            st, count = h.matchLocatedFromDevice(view.data_ptr(), n, cls, flags, ids.data_ptr(), pos.data_ptr(), rec.data_ptr() + 4 * PAD,
                                                 col.data_ptr() + 4 * PAD, capacity, check=False)
            torch.cuda.synchronize()
            assert count == count_w and st == (api.STATUS.SUCCESS if capacity >= count_w else api.STATUS.OUTPUT_TRUNCATED)
            assert np.array_equal(ids.cpu().numpy()[:count], ids_w) and np.array_equal(pos.cpu().numpy()[:count], pos_w)
            assert np.array_equal(inner(rec, capacity), record[:capacity]) and np.array_equal(inner(col, capacity), column[:capacity])
    # the host form on the GPU platform: the staged-piece path, then the host loop
    host = data.copy()
    ids = np.zeros(n, dtype=np.int32)
    pos = np.zeros(n, dtype=np.int32)
    rec = np.full(count_w, GUARD, dtype=np.int32)
    col = np.full(count_w, GUARD, dtype=np.int32)
    st, count = h.matchLocatedFromHost(host.ctypes.data, n, None, 0, ids.ctypes.data, pos.ctypes.data, rec.ctypes.data, col.ctypes.data, count_w)
    record, column, _ = ref.locate(data, pos_w, None, 0)
    assert (st, count) == (0, count_w) and np.array_equal(pos[:count], pos_w) and np.array_equal(rec, record) and np.array_equal(col, column)
    assert np.array_equal(view.cpu().numpy(), data) and np.array_equal(host, data)
    h.destroy()


def r256(b):
    return (b + 255) & ~255


def scratch_formula(size):
    """the formula of include/pfac_ext.h"""
    t = (size + T - 1) // T
    return r256(8 * (t + 1)) + 2 * r256(4 * t)


def test_scratch_accounting(handle):
    h = api.PFAC.create()
    before = int(h.info().deviceScratchBytes)
    for size in (5 * T + 1, 5 * T + 1, 64):
        data = np.full(size, ord("x"), dtype=np.uint8)
        whole, view = on_device(data, 0)
        st, rec, col, n = locate_device(h, view, size, [0, size - 1], None, 0)
        assert (st, n) == (0, 1) and rec.tolist() == [0, 0] and col.tolist() == [0, size - 1]
        assert int(h.info().deviceScratchBytes) - before == scratch_formula(5 * T + 1), "grown once, by the header's formula; never again"
    h.trim()
    assert int(h.info().deviceScratchBytes) == before
    h.destroy()


def test_optional_pointers_and_the_count_query(handle):
    data = np.frombuffer(b"abc\ndef\n", dtype=np.uint8)
    whole, view = on_device(data, 1)
    st, rec, col, n = locate_device(handle, view, data.size, [1, 5], None, 0, column=False)
    assert (st, n) == (0, 2) and rec.tolist() == [0, 1] and np.all(col == GUARD)
    assert handle.locatePairsFromDevice(view.data_ptr(), data.size, None, 0, None, 0, None, None) == (0, 2)          # numPairs == 0: the count alone
    assert handle.locatePairsFromDevice(view.data_ptr(), 0, None, 0, None, 0, None, None) == (0, 0)
    assert handle.locatePairsFromDevice(view.data_ptr(), data.size, None, 4, None, 0, None, None, check=False)[0] == api.STATUS.INVALID_PARAMETER


def test_device_form_on_a_host_only_handle():
    h = api.PFAC.createHostOnly()
    x = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    st, _ = h.locatePairsFromDevice(x.data_ptr(), 64, None, 0, x.data_ptr(), 2, x.data_ptr() + 64, None, check=False)
    assert st == api.STATUS.LIB_NOT_EXIST
    h.destroy()
