"""PFACX_countBatchFromDevice / PFACX_countBatchPairsFromDevice / PFACX_countBatchFromHost (GPU platform) against the references of
tests/segcount_ref.py and against the same handle's PFACX_matchAllBatchFromDevice list binned by its segFirst: every case of the host file, sizes 1, 7
and 4097 at two alignments, segments of 0 to 513 pairs, ids on both sides of a window edge and a window that is skipped, the touched list at its
capacity with a small segment of the same block behind it, more segments than the grid has blocks, chains, truncation, hostile device offsets, the
pairs form, every kernel variant and mode, one input above the 32 MiB switch, a 100 000-pattern set, nocase, the scratch accounting.  All arrays are
poisoned and carry guard words on both sides; the input is compared after every call."""

import functools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import allmatch_ref as am  # noqa: E402
from tests import rules_ref  # noqa: E402
from tests import scale_sets as ss  # noqa: E402
from tests import segcount_ref as ref  # noqa: E402
from tests.gpu_helpers import MODES, VARIANTS, make_handle  # noqa: E402
from tests.spans_helpers import pattern_file  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, TOUCHED, BLOCK_PAIRS = api.PFACX_SEGCOUNT_WINDOW, api.PFACX_SEGCOUNT_TOUCHED, api.PFACX_SEGCOUNT_BLOCK_PAIRS
BLOCKS_PER_CU = 4                               # scan_segcount.hip: the grid of a pass is at most this many blocks per compute unit
LONGEST, ACCUMULATE = api.PFACX_COUNT_LONGEST, api.PFACX_COUNT_ACCUMULATE
INVALID, TRUNCATED = api.STATUS.INVALID_PARAMETER, api.STATUS.OUTPUT_TRUNCATED
GUARD = 16
POISON = 0x5A5A5A5A5A5A5A5A
POISON32 = 0x5A5A5A5A


def as_array(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)


def gpu_handle(pf, flags=0, variant=api.PFACX_KERNEL_AUTO, perf=api.PFAC_TIME_DRIVEN, tex=api.PFAC_TEXTURE_OFF):
    h = api.PFAC.create()
    h.setPerfMode(perf)
    h.setTextureMode(tex)
    h.setKernelVariant(variant)
    h.readPatternFromFileEx(pf, flags)
    return h


class Out:
    """the three output arrays of a call on the device, poisoned, GUARD words on both sides of each"""

    def __init__(self, capacity, segs):
        self.capacity, self.segs = capacity, segs
        self.ids = torch.full((GUARD + capacity + GUARD,), -7, dtype=torch.int32, device="cuda:0")
        self.counts = torch.from_numpy(np.full(GUARD + capacity + GUARD, POISON32, dtype=np.uint32).view(np.int32)).to("cuda:0")
        self.first = torch.from_numpy(np.full(GUARD + segs + 1 + GUARD, POISON, dtype=np.uint64).view(np.int64)).to("cuda:0")

    def ptrs(self):
        return self.ids.data_ptr() + 4 * GUARD, self.counts.data_ptr() + 4 * GUARD, self.first.data_ptr() + 8 * GUARD

    def read(self, entries, first_written=True):
        """(segFirst, ids, counts); nothing in front of the arrays, behind the list or behind capacity may have been written"""
        torch.cuda.synchronize()
        ids, counts, first = self.ids.cpu().numpy(), self.counts.cpu().numpy().view(np.uint32), self.first.cpu().numpy().view(np.uint64)
        k = min(entries, self.capacity)
        assert np.all(ids[:GUARD] == -7) and np.all(ids[GUARD + k:] == -7), "ids: wrote outside the list or at or behind capacity"
        assert np.all(counts[:GUARD] == POISON32) and np.all(counts[GUARD + k:] == POISON32), "counts: wrote outside the list or at or behind capacity"
        assert np.all(first[:GUARD] == POISON) and np.all(first[GUARD + self.segs + 1:] == POISON), "wrote outside segFirst"
        if not first_written:
            assert np.all(first == POISON)
        return first[GUARD:GUARD + self.segs + 1].copy(), ids[GUARD:GUARD + k].copy(), counts[GUARD:GUARD + k].copy()


def device_offsets(offsets):
    return None if offsets is None else torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")


def device_list(h, data, offsets, flags=0, capacity=None, in_offset=0):
    """countBatchFromDevice -> (status, (segFirst, ids, counts), entries, total).  capacity None: the count query first, with null arrays, as a
    caller would.  The input must stay untouched"""
    data = as_array(data)
    n = int(data.size)
    d_in = torch.zeros(n + in_offset + 64, dtype=torch.uint8, device="cuda:0")
    d_in[in_offset:in_offset + n] = torch.from_numpy(data.copy()).to("cuda:0")
    segs = 1 if offsets is None else len(offsets) - 1
    d_off = device_offsets(offsets)
    o_ptr = None if d_off is None else d_off.data_ptr()
    if capacity is None:
        query = Out(0, segs)
        st, capacity, total0 = h.countBatchFromDevice(d_in.data_ptr() + in_offset, n, o_ptr, segs, flags, None, None, 0, query.ptrs()[2], check=False)
        assert st in (0, TRUNCATED) and (st == TRUNCATED) == (capacity > 0)
        query.read(0)
    out = Out(capacity, segs)
    I, K, F = out.ptrs()
    st, entries, total = h.countBatchFromDevice(d_in.data_ptr() + in_offset, n, o_ptr, segs, flags, I, K, capacity, F, check=False)
    got = out.read(entries)
    assert torch.equal(d_in[in_offset:in_offset + n].cpu(), torch.from_numpy(data.copy())), "the caller's input was modified"
    return st, got, entries, total


def check_device(h, want, data, offsets, flags, what, **kw):
    st, got, entries, total = device_list(h, data, offsets, flags, **kw)
    assert st == 0 and entries == want[1].size, f"{what}: status {st}, {entries} entries, want {want[1].size}"
    ref.same(got, want, what)
    assert total == int(want[2].sum(dtype=np.uint64)), f"{what}: the total"


def batch_pairs(h, data, offsets):
    """PFACX_matchBatchFromDeviceReduce -> (d_ids, d_segFirst, count) on the device, and the same on the host"""
    data = as_array(data)
    n, segs = int(data.size), len(offsets) - 1
    d_in = torch.from_numpy(data.copy()).to("cuda:0")
    d_off = device_offsets(offsets)
    d_ids = torch.full((n + 8,), -5, dtype=torch.int32, device="cuda:0")
    d_pos = torch.full((n + 8,), -5, dtype=torch.int32, device="cuda:0")
    d_first = torch.full((segs + 1,), -5, dtype=torch.int32, device="cuda:0")
    _, count = h.matchBatchFromDeviceReduce(d_in.data_ptr(), n, d_off.data_ptr(), segs, d_ids.data_ptr(), d_pos.data_ptr(), d_first.data_ptr())
    torch.cuda.synchronize()
    return d_ids, d_first, count


def binned(ids, first, f):
    """the (segFirst, ids, counts) list of an id list cut into segments by first[]: np.unique over segment * (F + 1) + id keys"""
    ids, first = np.asarray(ids, dtype=np.int64), np.asarray(first, dtype=np.int64)
    segs = first.size - 1
    seg = np.searchsorted(first, np.arange(ids.size), side="right") - 1
    u, c = np.unique(seg * (f + 1) + ids, return_counts=True)
    out = np.zeros(segs + 1, dtype=np.uint64)
    out[1:] = np.cumsum(np.bincount(u // (f + 1), minlength=segs))
    return out, (u % (f + 1)).astype(np.int32), c.astype(np.uint32)


def all_batch_binned(h, data, offsets):
    """the same handle's PFACX_matchAllBatchFromDevice list, binned by its d_segFirst"""
    data = as_array(data)
    n, segs, f = int(data.size), len(offsets) - 1, int(h.info().numOfPatterns)
    cap = n * max(1, int(h.info().maxMatchesPerPosition))
    d_in = torch.from_numpy(data.copy()).to("cuda:0")
    d_off = device_offsets(offsets)
    d_ids, d_pos = (torch.full((cap,), -5, dtype=torch.int32, device="cuda:0") for _ in range(2))
    d_first = torch.zeros(segs + 1, dtype=torch.int64, device="cuda:0")
    _, total = h.matchAllBatchFromDevice(d_in.data_ptr(), n, d_off.data_ptr(), segs, d_ids.data_ptr(), d_pos.data_ptr(), cap, d_first.data_ptr())
    torch.cuda.synchronize()
    return binned(d_ids[:total].cpu().numpy(), d_first.cpu().numpy(), f), total


def pairs_list(h, d_ids, num_pairs, d_first, segs, flags=0, capacity=None, ids_offset=0):
    """countBatchPairsFromDevice over device arrays -> (status, (segFirst, ids, counts), entries, total)"""
    p_ptr = None if d_ids is None else d_ids.data_ptr() + 4 * ids_offset
    f_ptr = None if d_first is None else d_first.data_ptr()
    if capacity is None:
        query = Out(0, segs)
        st, capacity, _ = h.countBatchPairsFromDevice(p_ptr, num_pairs, f_ptr, segs, flags, None, None, 0, query.ptrs()[2], check=False)
        assert st in (0, TRUNCATED)
    out = Out(capacity, segs)
    I, K, F = out.ptrs()
    st, entries, total = h.countBatchPairsFromDevice(p_ptr, num_pairs, f_ptr, segs, flags, I, K, capacity, F, check=False)
    return st, out.read(entries), entries, total


@functools.lru_cache(maxsize=None)
def prefix_of(pats):
    prefix, chain, _ = am.prefix_table(list(pats))
    return prefix, chain


# ---------------------------------------------------------------- the cases of the host file, small sizes


@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_on_the_three_forms(workdir, case):
    name, pats, data, offsets = case
    nocase = ref.is_nocase(name)
    h = gpu_handle(pattern_file(workdir, "segcount_" + name.replace("/", "_"), pats), api.PFACX_READ_NOCASE if nocase else 0)
    try:
        for longest in (False, True):
            flags = LONGEST if longest else 0
            want = ref.segcounts_py(pats, data, offsets, nocase, longest)
            for off in (0, 3):                                                  # (3: a misaligned d_input)
                check_device(h, want, data, offsets, flags, f"{name}/device/longest {longest}/offset {off}", in_offset=off)
            first, ids, counts, total = h.count_batch_host_array(as_array(data), offsets, longest)      # the GPU platform: the pipelined batch path
            ref.same((first, ids, counts), want, f"{name}/host form/longest {longest}")
            assert total == int(want[2].sum())
        if len(data):
            got, total = all_batch_binned(h, data, offsets)
            ref.same(got, ref.segcounts_py(pats, data, offsets, nocase), f"{name}/the all-match batch list binned")
            assert device_list(h, data, offsets)[3] == total, "*h_total is *h_num_matched of PFACX_matchAllBatchFromDevice"
            if not nocase:                                                      # (the batch reduce call returns the folded set's pairs too; one is enough)
                d_ids, d_first, count = batch_pairs(h, data, offsets)
                for longest in (False, True):
                    st, got, entries, total = pairs_list(h, d_ids, count, d_first, len(offsets) - 1, LONGEST if longest else 0)
                    assert st == 0
                    ref.same(got, ref.segcounts_py(pats, data, offsets, longest=longest), f"{name}/pairs form/longest {longest}")
    finally:
        h.destroy()


@pytest.mark.parametrize("n", [1, 7, 4097])
def test_small_sizes_at_two_alignments(workdir, n):
    pats = [b"ab", b"abc", b"b", b"cab", b"abcab"]
    data = (b"abcab.b" * (n // 7 + 1))[:n]
    cuts = sorted({0, n} | {min(n, c) for c in (1, 5, 6, 64, 65, 1000, 4096)})
    h = gpu_handle(pattern_file(workdir, "segcount_small", pats))
    try:
        for offsets in (cuts, None):
            for longest in (False, True):
                want = ref.segcounts_py(pats, data, offsets, longest=longest)
                for off in (0, 3):
                    check_device(h, want, data, offsets, LONGEST if longest else 0, f"{n} bytes/longest {longest}/offset {off}", in_offset=off)
    finally:
        h.destroy()


# ---------------------------------------------------------------- trips, windows, the touched list, the grid


def test_segments_of_0_to_513_pairs(workdir):
    """a one-byte pattern over runs of 0, 1, 255, 256, 257 and 513 bytes: the last trip of a segment empty, one pair, one short of full, full, one
    over, two over two trips -- under the nested set too, where every pair walks a chain of up to eight"""
    runs = [0, 1, BLOCK_PAIRS - 1, BLOCK_PAIRS, BLOCK_PAIRS + 1, 2 * BLOCK_PAIRS + 1]
    data, offsets = rules_ref.cut(*[b"a" * k + b".b." for k in runs])
    for name, pats in (("one-byte", [b"a", b"b"]), ("nested", ref.NESTED + [b"b"])):
        h = gpu_handle(pattern_file(workdir, "segcount_trips_" + name, pats))
        try:
            for longest in (False, True):
                want = ref.segcounts_py(pats, data, offsets, longest=longest)
                check_device(h, want, data, offsets, LONGEST if longest else 0, f"trips/{name}/longest {longest}")
            if name == "one-byte":
                assert [ref.pairs_of(want, k) for k in range(len(runs))] == [([(1, k)] if k else []) + [(2, 1)] for k in runs]
        finally:
            h.destroy()


@pytest.mark.parametrize("chain", [False, True], ids=["fixed-width", "with-a-common-prefix"])
def test_ids_on_both_sides_of_a_window_edge(workdir, chain):
    """W + 2 patterns: ids W - 1, W and W + 1 are the last id of window 0 and the first two of window 1.  chain: id 1 is a prefix of every other
    pattern, so the pairs of window 1 also count for an id in front of their window"""
    pats = ref.fixed_set(W + 2, chain)
    edge = b"".join(pats[i - 1] for i in (W + 1, W - 1, W, W + 1))
    data, offsets = rules_ref.cut(pats[5], edge, b"", pats[W] + b" " + pats[W - 1], pats[W - 2] * 3)
    h = gpu_handle(pattern_file(workdir, "segcount_window%d" % chain, pats))
    try:
        assert h.info().maxMatchesPerPosition == (2 if chain else 1)
        for longest in (False, True):
            want = ref.segcounts_py(pats, data, offsets, longest=longest)
            check_device(h, want, data, offsets, LONGEST if longest else 0, f"window edge/longest {longest}")
        want = ref.segcounts_py(pats, data, offsets)
        assert ref.pairs_of(want, 1) == ([(1, 4)] if chain else []) + [(W - 1, 1), (W, 1), (W + 1, 2)]
    finally:
        h.destroy()


@pytest.mark.parametrize("chain", [False, True], ids=["fixed-width", "with-a-common-prefix"])
def test_a_window_without_ids_is_skipped_and_the_order_kept(workdir, chain):
    pats = ref.fixed_set(2 * W + 2, chain)
    seg = b"".join(pats[i - 1] for i in (2 * W + 1, 7, 2 * W, 5, 2 * W + 1))
    data, offsets = rules_ref.cut(seg, pats[W + 3], seg + pats[W + 9])
    h = gpu_handle(pattern_file(workdir, "segcount_skip%d" % chain, pats))
    try:
        want = ref.segcounts_py(pats, data, offsets)
        assert ref.pairs_of(want, 0) == ([(1, 5)] if chain else []) + [(5, 1), (7, 1), (2 * W, 1), (2 * W + 1, 2)]
        check_device(h, want, data, offsets, 0, "windows 0 and 2")
        check_device(h, ref.segcounts_py(pats, data, offsets, longest=True), data, offsets, LONGEST, "windows 0 and 2/longest")
    finally:
        h.destroy()


@pytest.mark.parametrize("touch", [TOUCHED - 1, TOUCHED, TOUCHED + 1], ids=["one-less", "list-full", "one-more"])
def test_touched_list_and_what_it_leaves_behind(workdir, touch):
    """One segment with `touch` distinct ids of window 0 among 5000 segments of 8 bytes; the segment one grid behind it is taken by the SAME block
    and holds one pattern alone: a counter, a bit or a touched count left behind would show in its list"""
    pats = ref.fixed_set(TOUCHED + 8)
    h = gpu_handle(pattern_file(workdir, "segcount_touched", pats))
    try:
        grid = int(h.info().multiProcessorCount) * BLOCKS_PER_CU
        big_at, segs = 17, 5000
        assert big_at + grid < segs
        pieces = [pats[k % 5] + b" " for k in range(segs)]
        pieces[big_at] = b"".join(pats[:touch])
        pieces[big_at + grid] = pats[2] + b" "
        data, offsets = rules_ref.cut(*pieces)
        per_seg = [[k % 5 + 1] for k in range(segs)]                            # the reference in closed form: brute force over 5000 segments is slow
        per_seg[big_at] = list(range(1, touch + 1))
        per_seg[big_at + grid] = [3]
        first = np.zeros(segs + 1, dtype=np.uint64)
        first[1:] = np.cumsum([len(e) for e in per_seg])
        flat = np.array([i for e in per_seg for i in e], dtype=np.int32)
        want = (first, flat, np.ones(flat.size, dtype=np.uint32))
        check = ref.segcounts_py(pats, data[int(offsets[big_at]):int(offsets[big_at + 2])], [0, len(pieces[big_at]), len(pieces[big_at]) + 8])
        assert ref.pairs_of(check, 0) == [(i, 1) for i in range(1, touch + 1)] and ref.pairs_of(check, 1) == [((big_at + 1) % 5 + 1, 1)]
        check_device(h, want, data, offsets, 0, f"{touch} ids touched")
        st, got, entries, total = device_list(h, data, offsets, 0, capacity=big_at + touch // 2)   # truncated inside the big segment: the state is cleaned all the same
        assert (st, entries, total) == (TRUNCATED, flat.size, flat.size)
        ref.same(got, (first, flat[:big_at + touch // 2], want[2][:big_at + touch // 2]), f"{touch} ids touched/truncated")
    finally:
        h.destroy()


def test_more_segments_than_the_grid_has_blocks(workdir):
    pats = ref.NESTED + [b"b"]
    h = gpu_handle(pattern_file(workdir, "segcount_grid", pats))
    try:
        grid = int(h.info().multiProcessorCount) * BLOCKS_PER_CU
        segs = grid + 3
        pieces = [b""] * segs
        pieces[0], pieces[grid], pieces[segs - 1] = b"aaab", b"baaaaaaaaaa", b"a"         # block 0's first and second segment, block 2's second
        data, offsets = rules_ref.cut(*pieces)
        for longest in (False, True):
            small = ref.segcounts_py(pats, data, [0, 4, 15, 16], longest=longest)
            first = np.zeros(segs + 1, dtype=np.uint64)
            first[1:grid + 1], first[grid + 1:segs], first[segs] = small[0][1], small[0][2], small[0][3]
            want = (first, small[1], small[2])
            check_device(h, want, data, offsets, LONGEST if longest else 0, f"{segs} segments, three of them not empty/longest {longest}")
    finally:
        h.destroy()


# ---------------------------------------------------------------- chains


def test_nested_set_over_a_run_cut_at_every_byte(workdir):
    data = b"a" * 40 + b"b" + b"a" * 9
    h = gpu_handle(pattern_file(workdir, "segcount_nested", ref.NESTED))
    try:
        assert h.info().maxMatchesPerPosition == 8
        for offsets in (list(range(len(data) + 1)), [0, 7, 8, 9, 25, 41, 50], [0, 50]):
            for longest in (False, True):
                want = ref.segcounts_py(ref.NESTED, data, offsets, longest=longest)
                check_device(h, want, data, offsets, LONGEST if longest else 0, f"nested/{len(offsets) - 1} segments/longest {longest}")
    finally:
        h.destroy()


def test_siblings_under_a_prefix_and_a_set_without_chains(workdir):
    data, offsets = rules_ref.cut(b"abc abd ab", b" abcabd abx", b"abd", b"ab")
    for pats, most in (([b"ab", b"abc", b"abd"], 2), ([b"abc", b"abd", b"x"], 1)):     # most == 1: the table is never read
        h = gpu_handle(pattern_file(workdir, "segcount_siblings%d" % most, pats))
        try:
            assert h.info().maxMatchesPerPosition == most
            for longest in (False, True):
                want = ref.segcounts_py(pats, data, offsets, longest=longest)
                check_device(h, want, data, offsets, LONGEST if longest else 0, f"siblings/maxChain {most}/longest {longest}")
        finally:
            h.destroy()


# ---------------------------------------------------------------- truncation


def test_truncation_at_every_kind_of_capacity(workdir):
    data, offsets = b"a" * 20 + b"b" + b"a" * 3, [0, 10, 10, 21, 24]
    want = ref.segcounts_py(ref.NESTED, data, offsets)
    n = want[1].size
    assert want[0].tolist() == [0, 8, 8, 16, 19]
    h = gpu_handle(pattern_file(workdir, "segcount_trunc", ref.NESTED))
    try:
        for cap in (0, 1, 5, 8, 16, n - 1, n):                              # 5: inside segment 0; 8 and 16: exactly at a border
            st, got, entries, total = device_list(h, data, offsets, 0, capacity=cap)
            assert (st, entries, total) == (TRUNCATED if cap < n else 0, n, int(want[2].sum())), f"capacity {cap}"
            ref.same(got, (want[0], want[1][:cap], want[2][:cap]), f"capacity {cap}")
    finally:
        h.destroy()


# ---------------------------------------------------------------- hostile device offsets


def test_hostile_device_offsets_are_clamped(workdir):
    """offsets beyond `size`, a first offset that is not 0 and a decreasing pair (an empty segment): success, the guards intact, the list that of the
    clamped offsets.  No match lies across any of the offsets used, so which end a pair is cut at does not matter where segments overlap"""
    pats = [b"ab", b"b", b"abc"]
    data = as_array(b"abc ab b  " * 30)
    n = data.size
    h = gpu_handle(pattern_file(workdir, "segcount_hostile", pats))
    try:
        for hostile, clamped in (([0, 10, n + 100, 2 ** 40], [(0, 10), (10, n), (n, n)]),
                                 ([20, 50, n], [(20, 50), (50, n)]),
                                 ([0, 100, 40, n], [(0, 100), (100, 100), (40, n)]),
                                 ([n, n, n], [(n, n), (n, n)]),
                                 ([2 ** 63, 2 ** 40, n], [(n, n), (n, n)])):
            parts = [ref.segcounts_py(pats, data[a:b].tobytes()) for a, b in clamped]
            want_first = np.concatenate([[0], np.cumsum([p[1].size for p in parts])]).astype(np.uint64)
            want = (want_first, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]))
            st, got, entries, total = device_list(h, data, np.array(hostile, dtype=np.uint64))
            assert st == 0
            ref.same(got, want, f"offsets {hostile}")
    finally:
        h.destroy()


# ---------------------------------------------------------------- the pairs form


def test_pairs_form_ignores_ids_outside_the_set_at_every_alignment(workdir):
    pats = ref.NESTED + [b"b", b"ba"]
    f = len(pats)
    data, offsets = rules_ref.cut(b"aaab", b"", b"baaaaaaaaaa b", b"ba" * 300)
    h = gpu_handle(pattern_file(workdir, "segcount_pairs", pats))
    try:
        d_ids, d_first, count = batch_pairs(h, data, offsets)
        ids = d_ids[:count].cpu().numpy()
        first = d_first.cpu().numpy()
        segs = len(offsets) - 1
        for longest in (False, True):
            flags = LONGEST if longest else 0
            want = ref.segcounts_py(pats, data, offsets, longest=longest)
            st, got, entries, total = pairs_list(h, d_ids, count, d_first, segs, flags)
            assert st == 0 and total == int(want[2].sum())
            ref.same(got, want, f"pairs form/longest {longest}")
            ref.same(device_list(h, data, offsets, flags)[1], got, "the scan form equals the pairs form")
            # ids 0, F + 1 and -1 mixed in at the front of every segment: ignored; the list at every 4-byte alignment of d_pairIds
            junk = np.array([0, f + 1, -1, 2 ** 31 - 1, -(2 ** 31)], dtype=np.int32)
            mixed = np.concatenate([np.concatenate([junk, ids[first[k]:first[k + 1]]]) for k in range(segs)])
            mixed_first = (first + junk.size * np.arange(segs + 1)).astype(np.int32)
            for shift in range(4):
                d_mixed = torch.from_numpy(np.concatenate([np.full(shift, 1, dtype=np.int32), mixed, np.full(8, 1, dtype=np.int32)])).to("cuda:0")
                st, got, entries, total = pairs_list(h, d_mixed, mixed.size, torch.from_numpy(mixed_first).to("cuda:0"), segs, flags, ids_offset=shift)
                assert st == 0
                ref.same(got, want, f"pairs form/junk ids/shift {shift}/longest {longest}")
        # d_segFirstPairs out of range: clamped to [0, numPairs]; a decreasing pair is an empty segment
        wild = torch.tensor([-5, int(first[1]), 2 ** 31 - 1, 3, count + 7], dtype=torch.int32, device="cuda:0")
        st, got, entries, total = pairs_list(h, d_ids, count, wild, 4, LONGEST)
        want = binned(np.concatenate([ids[:first[1]], ids[first[1]:], ids[3:]]), [0, first[1], count, count, 2 * count - 3], f)
        assert st == 0
        ref.same(got, want, "segFirstPairs out of range")
        # one segment without d_segFirstPairs, and no pairs at all
        st, got, entries, total = pairs_list(h, d_ids, count, None, 1, LONGEST)
        ref.same(got, binned(ids, [0, count], f), "segFirstPairs NULL")
        st, got, entries, total = pairs_list(h, None, 0, d_first, segs, 0, capacity=4)
        assert (st, entries, total) == (0, 0, 0) and not got[0].any()
    finally:
        h.destroy()


# ---------------------------------------------------------------- every kernel variant and mode


@pytest.mark.parametrize("mode", MODES, ids=[m[2] for m in MODES])
@pytest.mark.parametrize("variant", VARIANTS, ids=[v[1] for v in VARIANTS])
def test_one_case_in_every_variant_and_mode(workdir, variant, mode):
    pats = [b"ab", b"abc", b"b", b"cab", b"abcab", b"needle", b"nee"]
    data, offsets = rules_ref.cut(b"abcab.b", b"a needle", b"needle nee", b"", b"cabcab" * 20)
    h = make_handle(pattern_file(workdir, "segcount_modes", pats), mode[0], mode[1], variant[0])
    try:
        for longest in (False, True):
            want = ref.segcounts_py(pats, data, offsets, longest=longest)
            check_device(h, want, data, offsets, LONGEST if longest else 0, f"{variant[1]}/{mode[2]}/longest {longest}")
    finally:
        h.destroy()


# ---------------------------------------------------------------- large inputs


def test_an_input_above_the_32_mib_switch(workdir):
    """33 MiB of lowercase filler in 1.5 KiB segments; 300 patterns that start with a capital -- some a prefix of another -- planted at 60 000
    places (wherever they fall: across segment borders too).  The reference: the oracle's longest vector of the whole buffer, cut at the borders
    (segcount_ref.batch_result), pushed up the prefix table"""
    rng = np.random.Generator(np.random.PCG64(2027))
    n, seg_len = (33 << 20) + 1000, 1536
    alnum = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789", dtype=np.uint8)
    stems = sorted({bytes([65 + int(rng.integers(0, 26))]) + rng.choice(alnum, size=int(rng.integers(3, 9))).tobytes() for _ in range(200)})
    pats = sorted(set(stems + [s + rng.choice(alnum, size=int(rng.integers(1, 5))).tobytes() for s in stems[:100]]))
    data = rng.integers(97, 123, size=n, dtype=np.uint8)
    for at in rng.integers(0, n - 32, size=60000):
        p = np.frombuffer(pats[int(rng.integers(0, len(pats)))], dtype=np.uint8)
        data[int(at):int(at) + p.size] = p
    offsets = np.append(np.arange(0, n, seg_len, dtype=np.uint64), np.uint64(n))
    pf = pattern_file(workdir, "segcount_big", pats)
    prefix, chain = prefix_of(tuple(pats))
    from tests.gpu_helpers import oracle_match
    seg_result = ref.batch_result(oracle_match(pf, data, omp=True), offsets, pats, prefix)
    h = gpu_handle(pf)
    try:
        for longest in (False, True):
            want = ref.segcounts_from_result(seg_result, offsets, (prefix, chain), longest)
            assert want[1].size > 20000
            check_device(h, want, data, offsets, LONGEST if longest else 0, f"33 MiB/longest {longest}")
    finally:
        h.destroy()


def test_a_100_000_pattern_set_with_a_few_hundred_segments():
    """thirteen windows of ids; against segcounts_from_result alone (brute force is too slow here)"""
    pats = ss.patterns(ss.S100)
    pf = ss.pattern_file(ss.S100)
    n = 1 << 20
    data = ss.text(ss.S100, n)
    offsets = np.append(np.arange(0, n, 3000, dtype=np.uint64), np.uint64(n))
    assert 300 < offsets.size < 400
    prefix, chain = prefix_of(tuple(pats))
    seg_result = ref.batch_result(ss.want(pf, data), offsets, pats, prefix)
    h = api.PFAC.create()
    try:
        h.setPerfMode(api.PFAC_SPACE_DRIVEN)
        h.readPatternFromFile(pf)
        for longest in (False, True):
            want = ref.segcounts_from_result(seg_result, offsets, (prefix, chain), longest)
            assert np.unique(want[1] // W).size >= 8, "the ids of the list lie in many windows"
            check_device(h, want, data, offsets, LONGEST if longest else 0, f"100 000 patterns/longest {longest}")
    finally:
        h.destroy()


# ---------------------------------------------------------------- nocase, statuses, memory


def test_nocase_counts_the_folded_set_and_leaves_the_input_alone(workdir):
    pats = [b"Needle", b"AB", b"get /admin", b"Nee"]
    data, offsets = rules_ref.cut(b"a NEEDLE in GeT /AdMiN", b" HTTP aB Ab plain ", b"nEeDlEab nEe", b"NEE")
    h = gpu_handle(pattern_file(workdir, "segcount_nocase", pats), api.PFACX_READ_NOCASE)
    try:
        assert h.caseInsensitive() == 1
        for longest in (False, True):
            want = ref.segcounts_py(pats, data, offsets, True, longest)
            check_device(h, want, data, offsets, LONGEST if longest else 0, f"nocase/longest {longest}", in_offset=1)     # (device_list compares the input)
        assert ref.pairs_of(ref.segcounts_py(pats, data, offsets, True), 2) == [(1, 1), (2, 1), (4, 2)]
    finally:
        h.destroy()


def test_statuses_of_the_device_forms(workdir):
    h = gpu_handle(pattern_file(workdir, "segcount_args", [b"ab", b"b"]))
    try:
        d_in = torch.from_numpy(as_array(b"abab").copy()).to("cuda:0")
        d_off = torch.tensor([0, 2, 4], dtype=torch.int64, device="cuda:0")
        d_ids, d_counts = (torch.zeros(8, dtype=torch.int32, device="cuda:0") for _ in range(2))
        d_first = torch.full((3,), 77, dtype=torch.int64, device="cuda:0")
        d_pf = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda:0")
        I, O, D, K, F, P = d_in.data_ptr(), d_off.data_ptr(), d_ids.data_ptr(), d_counts.data_ptr(), d_first.data_ptr(), d_pf.data_ptr()

        def status(*args):
            return h.countBatchFromDevice(*args, check=False)[0]

        assert h.countBatchFromDevice(I, 4, O, 2, 0, D, K, 8, F) == (0, 4, 4)
        assert h.countBatchFromDevice(I, 4, None, 1, LONGEST, D, K, 8, F) == (0, 2, 4)
        assert status(I, 4, O, 2, ACCUMULATE, D, K, 8, F) == INVALID and status(I, 4, O, 2, 4, D, K, 8, F) == INVALID
        assert status(None, 4, O, 2, 0, D, K, 8, F) == INVALID
        assert status(I, 4, O, 2, 0, None, K, 8, F) == INVALID and status(I, 4, O, 2, 0, D, None, 8, F) == INVALID
        assert status(I, 4, O, 2, 0, D, K, 8, None) == INVALID
        assert status(I, 4, None, 2, 0, D, K, 8, F) == INVALID
        assert status(I, 4, O, 0, 0, D, K, 8, F) == INVALID
        assert status(I, 1 << 31, O, 2, 0, D, K, 8, F) == INVALID and status(I, 4, O, 1 << 31, 0, D, K, 8, F) == INVALID
        assert h.countBatchPairsFromDevice(D, 1 << 31, P, 2, 0, D, K, 8, F, check=False)[0] == INVALID
        assert h.countBatchPairsFromDevice(D, 2, P, 2, ACCUMULATE, D, K, 8, F, check=False)[0] == INVALID
        d_first.fill_(77)
        assert h.countBatchFromDevice(I, 0, O, 2, 0, D, K, 8, F) == (0, 0, 0)          # size == 0: nothing counted, segFirst all zero
        torch.cuda.synchronize()
        assert d_first.cpu().tolist() == [0, 0, 0]
    finally:
        h.destroy()
    bare = api.PFAC.create()
    try:
        assert bare.countBatchFromDevice(I, 4, O, 2, 0, D, K, 8, F, check=False)[0] == api.STATUS.PATTERNS_NOT_READY
        assert bare.countBatchPairsFromDevice(D, 2, P, 2, 0, D, K, 8, F, check=False)[0] == api.STATUS.PATTERNS_NOT_READY
    finally:
        bare.destroy()


def round256(b):
    return (b + 255) & ~255


def test_scratch_accounting_and_the_shared_pair_scratch(workdir):
    from tests import count_ref
    pats = [b"ab", b"b", b"abc", b"ab"]
    data = as_array(b"abc ab b " * 100)
    n = data.size
    h = gpu_handle(pattern_file(workdir, "segcount_mem", pats))
    try:
        h.trim()
        scratch0 = int(h.info().deviceScratchBytes)
        n1, n2 = 3, 700
        for segs, last in ((n1, None), (n2, n1)):
            offsets = np.minimum(np.arange(segs + 1, dtype=np.uint64) * 4, n)
            offsets[-1] = n
            check_device(h, ref.segcounts_py(pats, data.tobytes(), offsets), data, offsets, 0, f"{segs} segments")
            scratch = int(h.info().deviceScratchBytes)
            if last is not None:                                            # the same bytes and pairs, more segments: what depends on the segments alone
                assert scratch - before == 4 * (segs - last) + round256(8 * (segs + 1) + 8) - round256(8 * (last + 1) + 8)
            before = scratch
        # the pairs form alone: the entry counts, their scan and the sum -- and the {prefix, chain length} table
        h.trim()
        assert int(h.info().deviceScratchBytes) == scratch0
        d_ids = torch.tensor([4, 4, 3, 2], dtype=torch.int32, device="cuda:0")
        d_first = torch.tensor([0, 2, 4], dtype=torch.int32, device="cuda:0")
        st, got, entries, total = pairs_list(h, d_ids, 4, d_first, 2, LONGEST)
        assert int(h.info().deviceScratchBytes) == scratch0 + round256(8 * 3 + 8)
        st, got, entries, total = pairs_list(h, d_ids, 4, d_first, 2, 0)
        assert int(h.info().deviceScratchBytes) == scratch0 + round256(8 * 3 + 8) + 8 * (len(pats) + 1)
        ref.same(got, ([0, 1, 4], [4, 2, 3, 4], [2, 1, 1, 1]), "pairs form: id 4 (ab) twice; id 3 (abc) counts for 3 and 4, id 2 for itself")
        h.trim()
        assert int(h.info().deviceScratchBytes) == scratch0
        # the rules call and the count call behind it on the same handle, through the same pair scratch
        offsets = [0, 9, 18, n]
        check_device(h, ref.segcounts_py(pats, data.tobytes(), offsets), data, offsets, 0, "after trim")
        rules = [[2, 4], [3]]
        r = h.rulesOpen(*rules_ref.csr(rules))
        d_in = torch.from_numpy(data.copy()).to("cuda:0")
        d_off = device_offsets(offsets)
        d_seg, d_rule = (torch.full((16,), -7, dtype=torch.int32, device="cuda:0") for _ in range(2))
        st, fired = r.match_device(d_in.data_ptr(), n, d_off.data_ptr(), 3, d_seg.data_ptr(), d_rule.data_ptr(), 16, None)
        want = rules_ref.fired_py(pats, rules, data.tobytes(), offsets)
        assert fired == want[0].size and d_seg[:fired].cpu().tolist() == want[0].tolist() and d_rule[:fired].cpu().tolist() == want[1].tolist()
        r.close()
        d_counts = torch.zeros(len(pats) + 1, dtype=torch.int64, device="cuda:0")
        _, added = h.countFromDevice(d_in.data_ptr(), n, 0, d_counts.data_ptr(), len(pats) + 1)
        count_ref.same(d_counts.cpu().numpy().view(np.uint64), count_ref.counts_py(pats, data.tobytes()), "countFromDevice behind it")
        check_device(h, ref.segcounts_py(pats, data.tobytes(), offsets), data, offsets, 0, "and again")
    finally:
        h.destroy()


def test_example_program_prints_the_counts_of_every_line():
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "countbatch_example"], check=True, stdout=subprocess.PIPE)
    p = subprocess.run([os.path.join(ROOT, "examples", "countbatch_example")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().splitlines()
    assert lines[:5] == ["1:", "2: 1\u00d71 2\u00d71 5\u00d73", "3:", "4: 1\u00d71 3\u00d72 4\u00d71", "5: 3\u00d73 4\u00d72 5\u00d71"]
    assert lines[5] == "9 entries, 15 occurrences in 5 lines" and "self-check passed" in lines
