"""PFACX_splitFromDevice (include/pfac_ext.h; scan_split.hip) on the GPU against tests/split_ref.py: the table, every tile, region and 16-byte
edge under every misalignment and flag combination, runs of delimiters across those edges, the density extremes, inputs longer than one grid
pass and than one step of each one-block pass, truncation, positions beyond 2^32, the batch calls over the device offsets as they lie, and the
scratch accounting.  Every call: guard words on both sides of the offsets array, guard bytes around the input, the input unmodified, nothing
written at or behind `capacity`."""

import numpy as np
import pytest
import torch                              # before the library loads its HIP runtime, as in every GPU test module

from pfac_amd import api  # noqa: E402
from tests import split_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

T = api.PFACX_SPLIT_TILE
GUARD = 0xA5A5A5A5A5A5A5A5
GUARD_I64 = int(np.array([GUARD], dtype=np.uint64).view(np.int64)[0])
PAD = 4                                   # guard words on each side of an offsets array
EDGE = 32                                 # guard bytes on each side of the input


@pytest.fixture(scope="module")
def handle():
    assert torch.cuda.is_available(), "GPU tests need a device; there is no CPU fallback to test"
    torch.cuda.set_device(0)
    h = api.PFAC.create()                  # no pattern set: the call needs none
    yield h
    h.destroy()


def on_device(data, mis=0):
    """the bytes at an address that is `mis` mod 16, guard bytes around them -> (the whole buffer, the input's view)"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    whole = torch.full((EDGE + 16 + data.size + EDGE,), 0x0A, dtype=torch.uint8, device="cuda:0")       # the guards are delimiters of most classes here
    view = whole[EDGE + mis:EDGE + mis + data.size]
    if data.size:
        view.copy_(torch.from_numpy(data.copy()))
    assert data.size == 0 or view.data_ptr() % 16 == mis
    return whole, view


def split_device(h, data, cls, flags, capacity, mis=0, null_array=False, device=None):
    """-> (status, segments, longest, the entries the call had room for), every guard and the input checked"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    whole, view = device if device is not None else on_device(data, mis)
    ptr = view.data_ptr() if data.size else whole.data_ptr()
    off = torch.full((capacity + 2 * PAD,), GUARD_I64, dtype=torch.int64, device="cuda:0")
    st, segments, longest = h.splitFromDevice(ptr, data.size, cls, flags, None if null_array else off.data_ptr() + 8 * PAD, capacity, check=False)
    torch.cuda.synchronize()
    got = off.cpu().numpy().view(np.uint64)
    assert np.all(got[:PAD] == GUARD) and np.all(got[PAD + capacity:] == GUARD), "written outside the array"
    back = whole.cpu().numpy()
    lo = EDGE + mis
    assert np.array_equal(back[lo:lo + data.size], data), "the input is never written"
    assert np.all(back[:lo] == 0x0A) and np.all(back[lo + data.size:] == 0x0A)
    return st, segments, longest, got[PAD:PAD + capacity].copy()


def check_against_reference(h, data, cls, flags, mis=0, device=None):
    want, segments, longest = ref.split(data, cls, flags)
    st, n, most, got = split_device(h, data, cls, flags, want.size + 3, mis, device=device)
    assert st == api.STATUS.SUCCESS
    assert (n, most) == (segments, longest), (n, most, segments, longest)
    assert np.array_equal(got[:want.size], want)
    assert np.all(got[want.size:] == GUARD), "nothing behind the closing entry"


@pytest.mark.parametrize("mis", [0, 3])
def test_table(handle, mis):
    for _, data, cls, flags, want, segments, longest in ref.table_cases():
        st, n, most, got = split_device(handle, data, cls, flags, want.size + 2, mis)
        assert st == api.STATUS.SUCCESS
        assert (n, most) == (segments, longest)
        assert np.array_equal(got[:want.size], want) and np.all(got[want.size:] == GUARD)


@pytest.mark.parametrize("n", [1, 15, 16, 17, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1])
def test_tile_edges(handle, n):
    """delimiters at exactly the positions around the first 16-byte load, the first tile's end and the input's end"""
    data = np.full(n, ord("x"), dtype=np.uint8)
    for p in (0, 1, 15, 16, T - 2, T - 1, T, T + 1, n - 2, n - 1):
        if 0 <= p < n:
            data[p] = ord("\n")
    for mis in (0, 1, 7, 15):
        device = on_device(data, mis)
        for flags in ref.ALL_FLAGS:
            check_against_reference(handle, data, None, flags, mis, device)
    check_against_reference(handle, data, b"\n;", 0, 5)                    # ... and through the class table in LDS


def runs_input(n, runs):
    data = np.full(n, ord("x"), dtype=np.uint8)
    for lo, hi in runs:                                                    # [lo, hi], both ends included
        data[lo:hi + 1] = ord(";")
    return data


@pytest.mark.parametrize("name, n, runs", [
    ("across a tile edge and a load edge", 2 * T + 5, [(14, 17), (T - 2, T + 1)]),
    ("a whole tile", 3 * T + 5, [(T - 3, 2 * T + 2)]),
    ("exactly a tile", 3 * T + 5, [(T, 2 * T - 1)]),
    ("to the last byte", T + 9, [(T - 1, T + 8)]),
    ("from the first byte", T + 9, [(0, 20), (T, T)]),
    ("region edges", T + 9, [(4094, 4097), (8191, 8191), (8192, 8192 + 1024)]),
    ("everything", T + 9, [(0, T + 8)]),
])
def test_runs_across_edges(handle, name, n, runs):
    data = runs_input(n, runs)
    for mis in (0, 9):
        device = on_device(data, mis)
        for flags in ref.ALL_FLAGS:
            check_against_reference(handle, data, b";", flags, mis, device)
    data[runs[0][0]] = ord(",")                                            # the same run out of two members of a class
    for flags in (ref.RUNS, ref.RUNS | ref.BEFORE):
        check_against_reference(handle, data, b";,", flags, 2)


def test_density_extremes(handle):
    n = 3 * T + 5
    every = np.full(n, ord("\n"), dtype=np.uint8)
    none = np.full(n, ord("x"), dtype=np.uint8)
    for flags in ref.ALL_FLAGS:
        st, segments, longest, got = split_device(handle, every, None, flags, n + 1, 1)
        assert st == api.STATUS.SUCCESS
        if flags & ref.RUNS:
            assert (segments, longest) == (1, n) and got[:2].tolist() == [0, n] and np.all(got[2:] == GUARD)
        else:
            assert (segments, longest) == (n, 1) and np.array_equal(got, np.arange(n + 1, dtype=np.uint64))
        check_against_reference(handle, every, ref.FULL_CLASS, flags)
        st, segments, longest, got = split_device(handle, none, None, flags, 4)
        assert (st, segments, longest) == (api.STATUS.SUCCESS, 1, n) and got[:2].tolist() == [0, n] and np.all(got[2:] == GUARD)
        check_against_reference(handle, every, ref.EMPTY_CLASS, flags)


def test_more_tiles_than_one_pass_of_anything(handle):
    """more tiles than the grid of the two streaming passes takes at once, than pfac_array_scan takes per step, than pfac_split_longest takes per
    step: random bytes, a class of one member; the longest segment lies across the step of the last of them"""
    grid = 8 * int(handle.info().multiProcessorCount)
    tiles = max(grid, api.PFACX_SPLIT_SCAN_STEP, api.PFACX_SPLIT_LONGEST_STEP) + 3
    n = tiles * T + 5
    rng = np.random.Generator(np.random.PCG64(31))
    data = rng.integers(0, 256, size=n, dtype=np.uint8)
    cls = bytes([int(data[7])])
    lo, hi = (api.PFACX_SPLIT_LONGEST_STEP - 2) * T + 11, (api.PFACX_SPLIT_LONGEST_STEP + 1) * T + 3
    data[lo:hi][data[lo:hi] == cls[0]] ^= 0x55                              # no delimiter in three tiles around that step
    device = on_device(data, 4)
    for flags in (0, ref.RUNS | ref.BEFORE):
        want, segments, longest = ref.split(data, cls, flags)
        assert longest >= hi - lo
        check_against_reference(handle, data, cls, flags, 4, device)


@pytest.mark.parametrize("members", [3, 128])
def test_more_counts_than_one_step_of_the_scan(handle, members):
    n = (api.PFACX_SPLIT_SCAN_STEP + 6) * T + 7
    rng = np.random.Generator(np.random.PCG64(40 + members))
    data, cls = ref.random_case(rng, n, members)
    device = on_device(data, 11)
    for flags in (ref.BEFORE, ref.RUNS):
        check_against_reference(handle, data, cls, flags, 11, device)


@pytest.mark.parametrize("flags", ref.ALL_FLAGS)
def test_truncation(handle, flags):
    rng = np.random.Generator(np.random.PCG64(78))
    data, cls = ref.random_case(rng, 2 * T + 100, 3)
    want, segments, longest = ref.split(data, cls, flags)
    assert segments > 64
    device = on_device(data, 6)
    for capacity in (0, 1, segments // 2, segments, segments + 1):
        st, n, most, got = split_device(handle, data, cls, flags, capacity, 6, null_array=capacity == 0, device=device)
        assert (n, most) == (segments, longest), "the full values whatever the capacity"
        assert st == (api.STATUS.SUCCESS if capacity >= segments + 1 else api.STATUS.OUTPUT_TRUNCATED)
        assert np.array_equal(got, want[:capacity]), "exactly the first `capacity` entries"
    st, n, most = handle.splitFromDevice(device[1].data_ptr(), data.size, cls, flags, None, 0, want_longest=False, check=False)
    assert (st, n, most) == (api.STATUS.OUTPUT_TRUNCATED, segments, 0)


def test_beyond_two_to_the_32(handle):
    if torch.cuda.mem_get_info()[0] < 6 << 30:
        pytest.skip("needs 6 GiB of free device memory")
    n = (1 << 32) + T + 3
    x = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    at = [(1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, n - 2]
    x[torch.tensor(at, device="cuda:0")] = 0x0A
    expected = {
        0: ([0, 1 << 31, (1 << 31) + 1, 1 << 32, (1 << 32) + 1, n - 1, n], 1 << 31),
        ref.RUNS | ref.BEFORE: ([0, (1 << 31) - 1, (1 << 32) - 1, n - 2, n], 1 << 31),
    }
    for flags, (want, longest) in expected.items():
        off = torch.full((len(want) + 2 * PAD,), GUARD_I64, dtype=torch.int64, device="cuda:0")
        st, segments, most = handle.splitFromDevice(x.data_ptr(), n, None, flags, off.data_ptr() + 8 * PAD, len(want), check=False)
        torch.cuda.synchronize()
        got = off.cpu().numpy().view(np.uint64)
        assert st == api.STATUS.SUCCESS and (segments, most) == (len(want) - 1, longest)
        assert got[PAD:PAD + len(want)].tolist() == want
        assert np.all(got[:PAD] == GUARD) and np.all(got[PAD + len(want):] == GUARD)
    assert int(torch.count_nonzero(x)) == len(at) and int(x[torch.tensor(at, device="cuda:0")].sum()) == 10 * len(at), "the input is never written"
    del x
    torch.cuda.empty_cache()


def test_composition_with_the_batch_calls():
    """the device offsets, as they lie, into PFACX_countBatchFromDevice and PFACX_rulesMatchFromDevice; the host forms over the reference's offsets"""
    data, patterns, (rule_off, rule_patterns) = ref.make_log()
    h = api.PFAC.create()
    h.readPatternFromMemory(patterns)
    rules = h.rulesOpen(rule_off, rule_patterns)
    host = api.PFAC.createHostOnly()
    host.readPatternFromMemory(patterns)
    host_rules = host.rulesOpen(rule_off, rule_patterns)
    whole, view = on_device(data, 3)
    for flags in ref.ALL_FLAGS:
        want, segments, _ = ref.split(data, None, flags)
        d_off = torch.full((segments + 1,), GUARD_I64, dtype=torch.int64, device="cuda:0")
        st, n, _ = h.splitFromDevice(view.data_ptr(), data.size, None, flags, d_off.data_ptr(), segments + 1)
        assert n == segments and segments > 100
        # the counts of every pattern in every segment
        first_w, ids_w, counts_w, total_w = host.count_batch_host_array(data, want)
        d_first = torch.zeros(segments + 1, dtype=torch.int64, device="cuda:0")
        d_ids = torch.full((ids_w.size + 1,), -7, dtype=torch.int32, device="cuda:0")
        d_counts = torch.zeros(ids_w.size + 1, dtype=torch.int32, device="cuda:0")
        st, entries, total = h.countBatchFromDevice(view.data_ptr(), data.size, d_off.data_ptr(), segments, 0, d_ids.data_ptr(), d_counts.data_ptr(),
                                                    ids_w.size + 1, d_first.data_ptr())
        torch.cuda.synchronize()
        assert (st, entries, total) == (0, ids_w.size, total_w) and total > 0
        assert np.array_equal(d_first.cpu().numpy().view(np.uint64), first_w.astype(np.uint64))
        assert np.array_equal(d_ids.cpu().numpy()[:entries], ids_w) and np.array_equal(d_counts.cpu().numpy().view(np.uint32)[:entries], counts_w)
        # the rules that fire on each segment
        seg_w, rule_w, rfirst_w = host_rules.match_host_array(data, want)
        d_seg = torch.full((seg_w.size + 1,), -7, dtype=torch.int32, device="cuda:0")
        d_rule = torch.full((seg_w.size + 1,), -7, dtype=torch.int32, device="cuda:0")
        d_rfirst = torch.zeros(segments + 1, dtype=torch.int64, device="cuda:0")
        st, fired = rules.match_device(view.data_ptr(), data.size, d_off.data_ptr(), segments, d_seg.data_ptr(), d_rule.data_ptr(), seg_w.size + 1,
                                       d_rfirst.data_ptr())
        torch.cuda.synchronize()
        assert (st, fired) == (0, seg_w.size) and fired > 0
        assert np.array_equal(d_seg.cpu().numpy()[:fired], seg_w) and np.array_equal(d_rule.cpu().numpy()[:fired], rule_w)
        assert np.array_equal(d_rfirst.cpu().numpy().view(np.uint64), rfirst_w.astype(np.uint64))
        assert np.array_equal(d_off.cpu().numpy().view(np.uint64), want), "the batch calls leave the offsets alone"
    assert np.array_equal(view.cpu().numpy(), data)
    host_rules.close()
    host.destroy()
    rules.close()
    h.destroy()


def r256(b):
    return (b + 255) & ~255


def scratch_formula(size):
    """the formula of include/pfac_ext.h"""
    t = (size + T - 1) // T
    return r256(8 * (t + 1)) + r256(16 * t) + 3 * r256(4 * t) + r256(8)


def test_scratch_accounting_and_other_handle_states(workloads):
    data = np.frombuffer(b"xAyaz\nBa", dtype=np.uint8)
    for read_flags in (None, 0, api.PFACX_READ_NOCASE):                     # no pattern set; a set; a caseless set
        h = api.PFAC.create()
        if read_flags is not None:
            h.readPatternFromFileEx(workloads["c1"].pattern_file, read_flags)
        before = int(h.info().deviceScratchBytes)
        for size in (5 * T + 1, 5 * T + 1, 64):
            big = np.full(size, ord("x"), dtype=np.uint8)
            st, segments, longest, got = split_device(h, big, None, 0, 2)
            assert (st, segments, longest) == (0, 1, size)
            assert int(h.info().deviceScratchBytes) - before == scratch_formula(5 * T + 1), "grown once, by the header's formula; never again"
        # 'A' in the class does not cut at 'a', whatever the handle folds
        st, segments, longest, got = split_device(h, data, b"A", 0, 4, 1)
        assert (st, segments, longest) == (0, 2, 6) and got[:3].tolist() == [0, 2, 8]
        h.trim()
        assert int(h.info().deviceScratchBytes) == before
        h.destroy()
