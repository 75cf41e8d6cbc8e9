"""PFACX_countFromDevice / PFACX_countPairsFromDevice / PFACX_countNonzeroFromDevice / PFACX_countFromHost (GPU platform) against the two references
of tests/count_ref.py: every edge case of the host file, sizes 1, 7 and 4097, a run of one id over several blocks, the nested set, every kernel
variant and mode, set sizes on both sides of the LDS-direct threshold and a 100 000-pattern set, one input above the 32 MiB switch, id lists at
every alignment and length with ids that must be ignored, a stream counted piece by piece, the all-match list's bincount, the non-zero compaction
with truncation, the scratch accounting, the caller's bytes.  All arrays are poisoned and carry guard words on both sides."""

import functools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from pfac_amd import workloads as wl  # noqa: E402
from tests import allmatch_ref as am  # noqa: E402
from tests import count_ref as ref  # noqa: E402
from tests import scale_sets as ss  # noqa: E402
from tests.gpu_helpers import MODES, VARIANTS, make_handle  # noqa: E402
from tests.spans_helpers import pattern_file  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONGEST, ACCUMULATE = api.PFACX_COUNT_LONGEST, api.PFACX_COUNT_ACCUMULATE
DIRECT = api.PFACX_COUNT_LDS_DIRECT         # scan_count.hip: kCountDirect: F + 1 <= DIRECT counts into one LDS counter per id
NZ_BLOCK = 256                              # scan_count.hip: kNzBlock, the entries one block of the non-zero compaction takes
SCAN_BLOCK = 8192                           # scan_passes.h: kScanBlock, the block values one block of the block-value scan takes
GUARD = 16
POISON = 0x5A5A5A5A5A5A5A5A
INVALID = api.STATUS.INVALID_PARAMETER


def as_array(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)


def counts_tensor(f, preset=None):
    arr = np.full(GUARD + f + 1 + GUARD, POISON, dtype=np.uint64)
    if preset is not None:
        arr[GUARD:GUARD + f + 1] = preset
    return torch.from_numpy(arr.view(np.int64)).to("cuda:0")


def read_counts(d, f):
    """counts[0, F] of a counts_tensor; the guard words on both sides must be what they were"""
    torch.cuda.synchronize()
    arr = d.cpu().numpy().view(np.uint64)
    assert np.all(arr[:GUARD] == POISON) and np.all(arr[GUARD + f + 1:] == POISON), "wrote outside counts[0, F]"
    return arr[GUARD:GUARD + f + 1].copy()


def device_counts(h, data, flags=0, in_offset=0, preset=None):
    """countFromDevice -> (counts, total); the input must stay untouched"""
    data = as_array(data)
    n, f = int(data.size), int(h.info().numOfPatterns)
    d_in = torch.zeros(n + in_offset + 64, dtype=torch.uint8, device="cuda:0")
    d_in[in_offset:in_offset + n] = torch.from_numpy(data.copy()).to("cuda:0")
    d = counts_tensor(f, preset)
    st, total = h.countFromDevice(d_in.data_ptr() + in_offset, n, flags, d.data_ptr() + 8 * GUARD, f + 1)
    assert st == 0
    got = read_counts(d, f)
    assert torch.equal(d_in[in_offset:in_offset + n].cpu(), torch.from_numpy(data.copy())), "the caller's input was modified"
    return got, total


def pair_counts(h, ids, flags=0, offset=0, preset=None, num_pairs=None):
    """countPairsFromDevice over an id list that starts `offset` ints into its allocation -> counts"""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    f = int(h.info().numOfPatterns)
    d_ids = torch.from_numpy(np.concatenate([np.full(offset, 1, dtype=np.int32), ids, np.full(8, 1, dtype=np.int32)])).to("cuda:0")
    d = counts_tensor(f, preset)
    assert h.countPairsFromDevice(d_ids.data_ptr() + 4 * offset, ids.size if num_pairs is None else num_pairs, flags, d.data_ptr() + 8 * GUARD, f + 1) == 0
    return read_counts(d, f)


def nonzero(h, counts, capacity=None):
    """countNonzeroFromDevice -> (status, ids, counts, distinct, total); nothing may be written at or behind capacity"""
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    cap = int(counts.size) if capacity is None else capacity
    d_counts = torch.from_numpy(counts.view(np.int64).copy()).to("cuda:0")
    d_ids = torch.full((cap + GUARD,), -5, dtype=torch.int32, device="cuda:0")
    d_out = torch.full((cap + GUARD,), -5, dtype=torch.int64, device="cuda:0")
    st, nd, total = h.countNonzeroFromDevice(d_counts.data_ptr(), counts.size, d_ids.data_ptr(), d_out.data_ptr(), cap)
    torch.cuda.synchronize()
    assert bool((d_ids[cap:] == -5).all()) and bool((d_out[cap:] == -5).all()), "wrote at or behind capacity"
    k = min(nd, cap)
    assert bool((d_ids[k:] == -5).all()) and bool((d_out[k:] == -5).all()), "wrote behind the list"
    return st, d_ids[:k].cpu().numpy(), d_out[:k].cpu().numpy().view(np.uint64), nd, total


def gpu_handle(pf, flags=0, variant=api.PFACX_KERNEL_AUTO, perf=api.PFAC_TIME_DRIVEN, tex=api.PFAC_TEXTURE_OFF):
    h = api.PFAC.create()
    h.setPerfMode(perf)
    h.setTextureMode(tex)
    h.setKernelVariant(variant)
    h.readPatternFromFileEx(pf, flags)
    return h


@functools.lru_cache(maxsize=None)
def prefix_of(pats):
    prefix, chain, _ = am.prefix_table(list(pats))
    return prefix, chain


def check_both_forms(h, data, result, table, what):
    for longest in (False, True):
        got, total = device_counts(h, data, LONGEST if longest else 0)
        ref.same(got, ref.counts_from_result(result, table, longest), f"{what}/longest {longest}")
        assert total == ref.total_of(result, table, longest) == int(got.sum()), f"{what}/longest {longest}: the total"


# ---------------------------------------------------------------- the cases of the host file, small sizes


@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_on_the_device_form_and_the_host_form(workdir, case):
    name, pats, data = case
    nocase = name.startswith("nocase")
    h = gpu_handle(pattern_file(workdir, "count_" + name, pats), api.PFACX_READ_NOCASE if nocase else 0)
    try:
        for longest in (False, True):
            want = ref.counts_py(pats, data, nocase, longest)
            for off in (0, 5):
                got, total = device_counts(h, data, LONGEST if longest else 0, in_offset=off)
                ref.same(got, want, f"{name}/device/longest {longest}/offset {off}")
                assert total == int(want.sum())
            got, total = h.count_host_array(as_array(data), longest)          # the GPU platform: the pipelined host path, counted on the host
            ref.same(got, want, f"{name}/host form/longest {longest}")
            assert total == int(want.sum())
    finally:
        h.destroy()


@pytest.mark.parametrize("n", [1, 7, 4097])
def test_small_sizes(workdir, n):
    pats = [b"ab", b"abc", b"b", b"cab", b"abcab"]
    data = (b"abcab.b" * (n // 7 + 1))[:n]
    h = gpu_handle(pattern_file(workdir, "count_small", pats))
    try:
        for longest in (False, True):
            got, total = device_counts(h, data, LONGEST if longest else 0)
            ref.same(got, ref.counts_py(pats, data, longest=longest), f"{n} bytes/longest {longest}")
            assert total == int(got.sum())
    finally:
        h.destroy()


def test_size_zero_zeroes_or_leaves_alone(workdir):
    h = gpu_handle(pattern_file(workdir, "count_zero", [b"ab", b"cd"]))
    try:
        preset = np.array([9, 9, 9], dtype=np.uint64)
        for flags, want in ((0, [0, 0, 0]), (ACCUMULATE, [9, 9, 9])):
            d = counts_tensor(2, preset)
            assert h.countFromDevice(d.data_ptr(), 0, flags, d.data_ptr() + 8 * GUARD, 3) == (0, 0)
            assert read_counts(d, 2).tolist() == want
    finally:
        h.destroy()


def test_a_run_of_one_id_over_several_blocks(workdir):
    """70 000 pairs of one id: more than one block, every wave's 256 ids one run, an LDS counter in the tens of thousands; then the same with a
    second id every 1000 bytes, and with the run starting off alignment"""
    h = gpu_handle(pattern_file(workdir, "count_run", [b"a", b"b", b"zz"]))
    try:
        data = np.full(70000, ord("a"), dtype=np.uint8)
        for off in (0, 3):
            got, total = device_counts(h, data, in_offset=off)
            assert got.tolist() == [0, 70000, 0, 0] and total == 70000
        data[::1000] = ord("b")
        got, total = device_counts(h, data)
        assert got.tolist() == [0, 69930, 70, 0] and total == 70000
        ids = np.ones(70000, dtype=np.int32)                    # the id list itself: runs that start and end inside a lane's four
        ids[5::7] = 2
        for off in (0, 1):
            assert pair_counts(h, ids, offset=off).tolist() == [0, 60000, 10000, 0]
    finally:
        h.destroy()


def test_nested_set_over_100_kb(workdir):
    """a, aa, ..., a x 8 over runs of a of every length up to 40: chains of depth 8, maxMatchesPerPosition = 8"""
    rng = np.random.Generator(np.random.PCG64(8))
    runs = [b"a" * int(k) + b"b" * int(g) for k, g in zip(rng.integers(0, 41, 5000), rng.integers(1, 3, 5000))]
    data = as_array(b"".join(runs))
    assert 90000 < data.size < 130000
    run_len = np.array([len(r.rstrip(b"b")) for r in runs])
    want = np.array([0] + [int(np.maximum(run_len - k + 1, 0).sum()) for k in range(1, 9)], dtype=np.uint64)      # a^k occurs len - k + 1 times in a run
    h = gpu_handle(pattern_file(workdir, "count_nested", ref.NESTED))
    try:
        assert h.info().maxMatchesPerPosition == 8
        got, total = device_counts(h, data)
        ref.same(got, want, "nested")
        assert total == int(want.sum())
        got, total = device_counts(h, data, LONGEST)
        assert total == int(want[1]) == int(got.sum()), "one longest pair per position that starts an a"
        # ... and against the all-match list: its bincount, its length
        cap = data.size * 8
        d_in = torch.from_numpy(data.copy()).to("cuda:0")
        d_ids, d_pos = (torch.full((cap,), -5, dtype=torch.int32, device="cuda:0") for _ in range(2))
        _, n = h.matchAllFromDevice(d_in.data_ptr(), data.size, d_ids.data_ptr(), d_pos.data_ptr(), cap)
        assert n == int(want.sum())
        ref.same(torch.bincount(d_ids[:n], minlength=9).cpu().numpy(), want, "bincount of PFACX_matchAllFromDevice")
    finally:
        h.destroy()


# ---------------------------------------------------------------- every variant and mode, set sizes, a big input


@pytest.fixture(scope="module")
def c3(workloads, oracle_results):
    return workloads["c3"], oracle_results["c3"], prefix_of(tuple(wl.snort_patterns(3000)))


@pytest.mark.parametrize("perf,tex,mode_name", MODES)
@pytest.mark.parametrize("variant,vname", VARIANTS)
def test_1_mib_every_variant_and_mode(c3, variant, vname, perf, tex, mode_name):
    w, result, table = c3
    assert np.count_nonzero(np.bincount(result[result > 0])) > 100, "the text hits many ids"
    h = make_handle(w.pattern_file, perf, tex, variant)
    try:
        check_both_forms(h, w.data, result, table, f"{vname}/{mode_name}")
    finally:
        h.destroy()


def test_bincount_of_the_all_match_list_equals_the_counts(c3):
    w, result, table = c3
    h = make_handle(w.pattern_file, api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        f, n = int(h.info().numOfPatterns), int(w.data.size)
        cap = n * int(h.info().maxMatchesPerPosition)
        d_in = torch.from_numpy(w.data.copy()).to("cuda:0")
        d_ids, d_pos = (torch.full((cap,), -5, dtype=torch.int32, device="cuda:0") for _ in range(2))
        _, listed = h.matchAllFromDevice(d_in.data_ptr(), n, d_ids.data_ptr(), d_pos.data_ptr(), cap)
        got, total = device_counts(h, w.data)
        assert total == listed, "the total is the length of the all-match list"
        ref.same(got, torch.bincount(d_ids[:listed], minlength=f + 1).cpu().numpy(), "bincount of the all-match list")
        # the all-match list counted as it is: PFACX_COUNT_LONGEST takes every pair for itself alone
        ref.same(pair_counts(h, d_ids[:listed].cpu().numpy(), LONGEST), got, "the all-match ids under PFACX_COUNT_LONGEST")
    finally:
        h.destroy()


SET_SIZES = sorted({1, 63, 64, 65, 4095, 4096, 4097, 16383, 16384, 16385, DIRECT - 2, DIRECT - 1, DIRECT})        # F + 1 == DIRECT is the last direct one


def scale_text(pats):
    """about 1 MiB of the C3 stream with 30 000 patterns of the set planted at random places: it hits many ids, many of them often"""
    data = ss.plain_text((1 << 20) + 11)
    rng = np.random.Generator(np.random.PCG64(len(pats)))
    for k in rng.integers(0, len(pats), 30000):
        p = np.frombuffer(pats[int(k)], dtype=np.uint8)
        at = int(rng.integers(0, data.size - p.size))
        data[at:at + p.size] = p
    return data


@pytest.mark.parametrize("f", SET_SIZES + [ss.S100])
def test_set_sizes_around_the_lds_threshold(f):
    pats = tuple(ss.patterns(ss.S100)[:f])
    pf = ss.pattern_file(ss.S100) if f == ss.S100 else wl.write_pattern_file(ss.scratch_path(f"count_first{f}.pat"), list(pats))
    data = scale_text(pats)
    result = ss.want(pf, data)
    assert np.count_nonzero(np.bincount(result[result > 0])) >= min(f, 4000) // 2 and np.count_nonzero(result) > 15000, "the text hits many ids"
    h = make_handle(pf, api.PFAC_SPACE_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        assert int(h.info().numOfPatterns) == f
        check_both_forms(h, data, result, prefix_of(pats), f"F = {f}")
    finally:
        h.destroy()


def test_big_input_through_the_filter_kernel():
    data, result, density = ss.density_stream(0.10)
    assert data.size == ss.BIG
    table = prefix_of(tuple(ss.patterns(ss.C3)))
    h = make_handle(ss.pattern_file(ss.C3), api.PFAC_SPACE_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        check_both_forms(h, data, result, table, f"{ss.BIG} bytes at density {density:.3f}")
    finally:
        h.destroy()


# ---------------------------------------------------------------- the id list of the caller


def test_id_lists_at_every_alignment_and_length(workdir):
    pats = [b"ab", b"abc", b"abd", b"x", b"abcq"]               # chains: abcq -> abc -> ab
    f = len(pats)
    h = gpu_handle(pattern_file(workdir, "count_pairs", pats))
    try:
        table = prefix_of(tuple(pats))
        junk = [0, -1, f + 1, 2**31 - 1, -2**31]
        rng = np.random.Generator(np.random.PCG64(3))
        for offset in (0, 1, 2, 3):
            for pairs in list(range(10)) + [1023, 1024, 1029, 5000]:
                ids = rng.choice(np.array(list(range(1, f + 1)) + junk, dtype=np.int64), size=pairs).astype(np.int32)
                valid = ids[(ids >= 1) & (ids <= f)]
                preset = rng.integers(0, 1000, f + 1).astype(np.uint64)
                for longest in (False, True):
                    want = ref.counts_from_result(valid, table, longest)
                    flags = LONGEST if longest else 0
                    ref.same(pair_counts(h, ids, flags, offset, preset), want, f"offset {offset}/{pairs} pairs/longest {longest}")
                    got = pair_counts(h, ids, flags | ACCUMULATE, offset, preset)
                    add = want.copy()
                    add[0] = 0
                    ref.same(got, preset + add, f"offset {offset}/{pairs} pairs/longest {longest}/accumulate")
        # no pairs: d_ids may be null
        d = counts_tensor(f, np.full(f + 1, 7, dtype=np.uint64))
        assert h.countPairsFromDevice(None, 0, ACCUMULATE, d.data_ptr() + 8 * GUARD, f + 1) == 0 and read_counts(d, f).tolist() == [7] * (f + 1)
        assert h.countPairsFromDevice(None, 0, 0, d.data_ptr() + 8 * GUARD, f + 1) == 0 and read_counts(d, f).tolist() == [0] * (f + 1)
        assert h.countPairsFromDevice(None, 1, 0, d.data_ptr() + 8 * GUARD, f + 1, check=False) == INVALID
        assert h.countPairsFromDevice(d.data_ptr(), 1 << 31, 0, d.data_ptr() + 8 * GUARD, f + 1, check=False) == INVALID
    finally:
        h.destroy()


def test_accumulate_carries_into_the_high_word_on_the_device(workdir):
    h = gpu_handle(pattern_file(workdir, "count_carry", [b"a", b"aa", b"zz"]))
    try:
        preset = np.array([7, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFFFFFFFFF0], dtype=np.uint64)
        got, total = device_counts(h, b"aaa", ACCUMULATE, preset=preset)
        assert got.tolist() == [7, 0x100000002, 0x100000001, 0xFFFFFFFFFFFFFFF0] and total == 5
    finally:
        h.destroy()


def test_a_stream_counted_piece_by_piece_equals_the_one_buffer_count(c3):
    w, result, table = c3
    data = w.data[:300000]
    result = result.copy()[:300000]
    h = make_handle(w.pattern_file, api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        f, m = int(h.info().numOfPatterns), int(h.info().maxPatternLen)
        whole, total = device_counts(h, data)
        d = counts_tensor(f)
        K = d.data_ptr() + 8 * GUARD
        s = h.streamOpen()
        cuts = [0, 100001, 100003, 300000]                      # the middle piece is shorter than a pattern
        cap = data.size + m
        d_ids, d_pos = (torch.full((cap,), -5, dtype=torch.int32, device="cuda:0") for _ in range(2))
        pairs = 0
        for k, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
            d_piece = torch.from_numpy(data[lo:hi].copy()).to("cuda:0")
            _, n, _ = s.match_device(d_piece.data_ptr(), hi - lo, d_ids.data_ptr(), d_pos.data_ptr(), cap)
            h.countPairsFromDevice(d_ids.data_ptr(), n, ACCUMULATE if k else 0, K, f + 1)
            torch.cuda.synchronize()
            pairs += n
        _, n = s.flush(d_ids.data_ptr(), d_pos.data_ptr(), cap)
        h.countPairsFromDevice(d_ids.data_ptr(), n, ACCUMULATE, K, f + 1)
        s.close()
        ref.same(read_counts(d, f), whole, "three pieces and the flush")
        assert pairs + n == np.count_nonzero(result), "the pieces and the flush report every longest pair once"
    finally:
        h.destroy()


# ---------------------------------------------------------------- the non-zero counts


@pytest.fixture(scope="module")
def bare():
    """the non-zero call needs no pattern set"""
    h = api.PFAC.create()
    yield h
    h.destroy()


def check_nonzero(h, counts, what):
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    ids = np.flatnonzero(counts)
    total = int(counts.sum(dtype=np.uint64))
    st, got_ids, got_counts, nd, tot = nonzero(h, counts)
    assert (st, nd, tot) == (0, ids.size, total), what
    assert np.array_equal(got_ids, ids) and np.array_equal(got_counts, counts[ids]), what
    for cap in sorted({0, max(0, ids.size - 1)}):
        if cap >= ids.size:
            continue
        st, got_ids, got_counts, nd, tot = nonzero(h, counts, cap)
        assert (st, nd, tot) == (api.STATUS.OUTPUT_TRUNCATED, ids.size, total), f"{what}/capacity {cap}"
        assert np.array_equal(got_ids, ids[:cap]) and np.array_equal(got_counts, counts[ids[:cap]]), f"{what}/capacity {cap}"


@pytest.mark.parametrize("n", [1, 2, NZ_BLOCK - 1, NZ_BLOCK, NZ_BLOCK + 1, SCAN_BLOCK + 3, NZ_BLOCK * SCAN_BLOCK + 3, NZ_BLOCK * (2 * SCAN_BLOCK + 1) + 3])
def test_nonzero_counts(bare, n):
    """(the last two sizes: more block values than one block of the block-value scan takes, and more than two)"""
    rng = np.random.Generator(np.random.PCG64(n))
    big = np.uint64(0x100000000)
    check_nonzero(bare, np.zeros(n, dtype=np.uint64), f"{n} zeros")
    check_nonzero(bare, rng.integers(1, 100, n).astype(np.uint64) * big + np.uint64(1), f"{n} non-zero counts above 2^32")
    sparse = np.where(rng.random(n) < 0.3, rng.integers(1, 1 << 40, n), 0).astype(np.uint64)
    sparse[0] = 3                                                 # entry 0 takes part like any other
    sparse[-1] = 5
    check_nonzero(bare, sparse, f"{n} sparse counts")


def test_nonzero_of_a_count_call(c3):
    w, result, table = c3
    h = make_handle(w.pattern_file, api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        got, total = device_counts(h, w.data)
        st, ids, counts, nd, tot = nonzero(h, got)
        assert st == 0 and tot == total and nd == np.count_nonzero(got)
        assert np.array_equal(ids, np.flatnonzero(got)) and np.array_equal(counts, got[ids])
        assert h.countNonzeroFromDevice(None, 0, None, None, 0) == (0, 0, 0), "numCounts == 0"
    finally:
        h.destroy()


# ---------------------------------------------------------------- scratch, errors, the example


def test_scratch_accounting_and_trim(workdir):
    pats = [b"NEEDLE", b"NEE", b"Z"]
    rng = np.random.Generator(np.random.PCG64(4))
    data = rng.integers(97, 123, size=300000, dtype=np.uint8)
    data[rng.random(data.size) < 0.01] = ord("Z")
    data[1000:1006] = np.frombuffer(b"NEEDLE", dtype=np.uint8)
    z = int(np.count_nonzero(data == ord("Z")))                 # (lower-case letters otherwise: NEEDLE occurs once, and NEE inside it)
    want, want_longest = np.array([0, 1, 1, z], dtype=np.uint64), np.array([0, 1, 0, z], dtype=np.uint64)
    h = gpu_handle(pattern_file(workdir, "count_scratch", pats))
    try:
        n, f = data.size, len(pats)
        d_in = torch.from_numpy(data.copy()).to("cuda:0")
        d_ids, d_pos = (torch.full((n,), -5, dtype=torch.int32, device="cuda:0") for _ in range(2))
        h.matchFromDeviceReduce(d_in.data_ptr(), n, d_ids.data_ptr(), d_pos.data_ptr())        # the scan's own scratch is there already
        torch.cuda.synchronize()
        before = h.info().deviceScratchBytes
        ref.same(device_counts(h, data)[0], want, "first call")
        grown = h.info().deviceScratchBytes
        r256 = lambda b: (b + 255) // 256 * 256  # noqa: E731
        assert grown - before == 8 * n + r256(4 * (f + 1)) + r256(8) + 8 * (f + 1), "the pair list, L and its total, the prefix table (pfac_ext.h)"
        ref.same(device_counts(h, data)[0], want, "second call")
        assert h.info().deviceScratchBytes == grown, "a second call of the same shape allocates nothing"
        h.trim()
        assert h.info().deviceScratchBytes < before, "trim gives the scratch back"
        trimmed = h.info().deviceScratchBytes
        ref.same(device_counts(h, data, LONGEST)[0], want_longest, "after trim")
        assert h.info().deviceScratchBytes > trimmed, "the call works again after the trim, on scratch of its own"
        h.trim()
        trimmed = h.info().deviceScratchBytes
        counts = np.arange(5 * NZ_BLOCK + 1, dtype=np.uint64)
        assert nonzero(h, counts)[3] == counts.size - 1
        b = (counts.size + NZ_BLOCK - 1) // NZ_BLOCK
        assert h.info().deviceScratchBytes - trimmed == r256(4 * b) + r256(4 * (b + 1)) + r256(8 * b) + r256(16), "the non-zero call's block values"
    finally:
        h.destroy()


def test_error_rows_on_a_device_handle(workdir):
    h = gpu_handle(pattern_file(workdir, "count_errors", [b"ab", b"cd"]))
    try:
        d_in = torch.from_numpy(np.frombuffer(b"ab.cd.", dtype=np.uint8).copy()).to("cuda:0")
        d = counts_tensor(2)
        I, K = d_in.data_ptr(), d.data_ptr() + 8 * GUARD
        call = lambda *a: h.countFromDevice(*a, check=False)[0]  # noqa: E731
        assert call(I, 6, 0, K, 2) == INVALID and call(I, 1 << 31, 0, K, 3) == INVALID and call(I, 6, 4, K, 3) == INVALID
        assert call(None, 6, 0, K, 3) == INVALID and call(I, 6, 0, None, 3) == INVALID
        assert api.load_library().PFACX_countFromDevice(h._h, I, 6, 0, K, 3, None) == INVALID
        torch.cuda.synchronize()
        assert np.all(d.cpu().numpy().view(np.uint64) == POISON), "a refused call wrote"
        assert h.countFromDevice(I, 6, 0, K, 3) == (0, 2) and read_counts(d, 2).tolist() == [0, 1, 1], "the handle is usable after refused calls"
    finally:
        h.destroy()
    bare = api.PFAC.create()
    try:
        assert bare.countFromDevice(I, 6, 0, K, 3, check=False)[0] == api.STATUS.PATTERNS_NOT_READY
        assert bare.countPairsFromDevice(I, 1, 0, K, 3, check=False) == api.STATUS.PATTERNS_NOT_READY
    finally:
        bare.destroy()


def test_example_program_passes_its_self_check(workdir):
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "count_example"], check=True, stdout=subprocess.PIPE)
    p = subprocess.run([os.path.join(ROOT, "examples", "count_example")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    assert b"self-check passed" in p.stdout
