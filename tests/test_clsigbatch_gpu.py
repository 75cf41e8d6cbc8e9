"""PFACX_clsigBatchMatchFromDevice / PFACX_clsigBatchPairsFromDevice / PFACX_clsigBatchMatchFromHost (GPU platform) against the models of
tests/clsig_ref.py run on each segment alone (tests/clsigbatch_ref.py) and against the library's own plain call per segment: the window-edge
table at every pointer offset mod 4 and every segment start mod 4 with both end rules, pair counts around the frame's block with the segment
changing inside a block and at its edge, one-byte segments, runs of empty segments, segment counts around the bounds launch's block, one pairs
list past a single grid pass, a pairs list that does not ascend, offsets no caller should pass, one segment against the plain call, the gapsig
cross-check per segment, truncation with and without the end and segFirst arrays, the refusals, and the seeded random case.  All arrays are
poisoned and carry guard words on both sides; the input and the offsets must stay untouched.  Every comparison is exact."""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import clsig_ref as ref  # noqa: E402
from tests import clsigbatch_ref as bref  # noqa: E402

BLOCK = api.PFACX_CLSIG_BLOCK                   # scan_clsig.hip: kClSigBlock
PER_CU = api.PFACX_CLSIG_BLOCKS_PER_CU          # scan_passes.h: offsetBlocks takes eight blocks per compute unit at most
BOUNDS = api.PFACX_CLSIG_BOUNDS_BLOCK           # scan_clsig.hip: kBoundsBlock
GUARD = 64
POISON = -5
INVALID, TRUNCATED = api.STATUS.INVALID_PARAMETER, api.STATUS.OUTPUT_TRUNCATED


def as_array(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)


def guarded(values, dtype):
    """`values` on the device between GUARD poisoned entries -> (tensor, the address of the first value)"""
    t = torch.full((GUARD + len(values) + GUARD,), POISON, dtype=dtype, device="cuda:0")
    if len(values):
        t[GUARD:GUARD + len(values)] = torch.from_numpy(np.ascontiguousarray(values))
    return t, t.data_ptr() + t.element_size() * GUARD


def device_offsets(offsets):
    """size_t offsets (values up to 2^64 - 1) as the bits of an int64 tensor"""
    return guarded(np.array([int(o) for o in offsets], dtype=np.uint64).view(np.int64), torch.int64)


def device_input(data, in_offset=0):
    """the input as a slice of a larger tensor: its first byte in_offset bytes behind a 256-byte boundary, the tensor ENDS with its last byte"""
    data = as_array(data)
    lead = 16 + in_offset
    host = np.full(lead + data.size, 0x2E, dtype=np.uint8)
    host[lead:] = data
    d = torch.from_numpy(host).to("cuda:0")
    assert d.data_ptr() % 256 == 0
    return d, d.data_ptr() + lead


def check_guards(arrays, cap, clean_from):
    for a in arrays:
        assert bool((a[:GUARD] == POISON).all()) and bool((a[GUARD + cap:] == POISON).all()), "wrote outside the arrays"
        assert bool((a[GUARD + clean_from:GUARD + cap] == POISON).all()), "wrote behind the list"


def run_batch(sg, d_in, address, n, offsets, capacity, pairs=None, with_end=True, with_first=True):
    """the device form, or with pairs = (ids, positions) the pairs form -> (status, (pos, ids, end) written, segFirst or None, the full length)"""
    before = d_in.clone()
    segs = len(offsets) - 1
    d_off, off_ptr = device_offsets(offsets)
    off_before = d_off.clone()
    arrays = [torch.full((GUARD + capacity + GUARD,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(3)]
    ptr = [a.data_ptr() + 4 * GUARD if capacity else None for a in arrays]
    d_first, first_ptr = guarded(np.full(segs + 1, POISON, dtype=np.int64), torch.int64)
    end_ptr, seg_ptr = (ptr[2] if with_end else None), (first_ptr if with_first else None)
    if pairs is None:
        st, total = sg.match_batch_device(address, n, off_ptr, segs, ptr[0], ptr[1], end_ptr, capacity, seg_ptr, check=False)
    else:
        lists = [guarded(np.ascontiguousarray(a, dtype=np.int32), torch.int32) for a in pairs]
        lists_before = [t.clone() for t, _ in lists]
        st, total = sg.batch_pairs_device(address, n, off_ptr, segs, lists[0][1], lists[1][1], len(pairs[0]), ptr[0], ptr[1], end_ptr, capacity, seg_ptr,
                                          check=False)
    torch.cuda.synchronize()
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > capacity), (st, total, capacity)
    k = min(total, capacity)
    check_guards(arrays[:2], capacity, k if pairs is not None else min(capacity, max(k, n)))       # the device form: the scan's list below `size`
    check_guards(arrays[2:], capacity, k if with_end else 0)
    assert bool((d_first[:GUARD] == POISON).all()) and bool((d_first[GUARD + segs + 1:] == POISON).all()), "wrote outside segFirst"
    assert with_first or bool((d_first == POISON).all())
    assert torch.equal(d_in, before) and torch.equal(d_off, off_before), "the caller's input or offsets, or what lies around them, were modified"
    assert pairs is None or all(torch.equal(t, b) for (t, _), b in zip(lists, lists_before)), "the caller's pair list was modified"
    got = tuple(a[GUARD:GUARD + k].cpu().numpy() for a in (arrays[1], arrays[0], arrays[2]))
    return st, got, (d_first[GUARD:GUARD + segs + 1].cpu().numpy().view(np.uint64) if with_first else None), total


def longest_pairs(h, address, n):
    d_ids, d_pos = (torch.full((n,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
    _, count = h.matchFromDeviceReduce(address, n, d_ids.data_ptr(), d_pos.data_ptr())
    torch.cuda.synchronize()
    return d_ids[:count].cpu().numpy(), d_pos[:count].cpu().numpy()


class Opened:
    """a GPU handle with a class-signature object over `sigs` (or the text `lines`)"""

    def __init__(self, sigs, max_len=0, flags=0, lines=None):
        self.sigs, self.flags, self.lines = sigs, flags, lines
        self.h = api.PFAC.create()
        self.sg = self.h.clsigOpenText(ref.text_of(lines), max_len, flags) if lines is not None else self.h.clsigOpen(*ref.csr_of(sigs), max_len, flags)
        self.anchors = self.sg.anchors()
        want, _ = ref.model_anchors(sigs, max_len)
        assert all(g.tolist() == w.tolist() for g, w in zip(self.anchors, want))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.sg.close(check=False)
        self.h.destroy()

    def all_forms(self, data, offsets, want, want_first, what, in_offset=0, host_form=True):
        """the device form, the pairs form over the pairs of the handle's own plain scan, and the host form (the GPU platform: the staged path)"""
        data = as_array(data)
        n, size = int(data.size), int(want[0].size)
        d_in, address = device_input(data, in_offset)
        st, got, first, total = run_batch(self.sg, d_in, address, n, offsets, max(n, size) + 3)
        assert st == 0 and total == size, (what, total, size)
        ref.same(got, want, f"{what}/device")
        assert first.tolist() == [int(f) for f in want_first], f"{what}/device: segFirst"
        st, got, first, total = run_batch(self.sg, d_in, address, n, offsets, size + 3, pairs=longest_pairs(self.h, address, n))
        assert st == 0
        ref.same(got, want, f"{what}/pairs")
        assert first.tolist() == [int(f) for f in want_first], f"{what}/pairs: segFirst"
        if host_form:
            pos, ids, end, first = self.sg.match_batch_host_array(data, offsets)
            ref.same((pos, ids, end), want, f"{what}/host form")
            assert first.tolist() == [int(f) for f in want_first], f"{what}/host form: segFirst"


# ---------------------------------------------------------------- 1. window edges, every alignment


@functools.lru_cache(maxsize=None)
def edge_model(index, flags, lead):
    """computed once, shared by the four pointer offsets"""
    case = bref.EDGE_CASES[index]
    sigs = ref.parse_lines(case[1])
    anchors, _ = ref.model_anchors(sigs, case[2])
    data, offsets = bref.edge_batch(case, lead)
    return bref.batch_model(sigs, data, offsets, anchors, flags, case[1] if lead == 0 else None)


@pytest.mark.parametrize("in_offset", [0, 1, 2, 3])
@pytest.mark.parametrize("index", range(len(bref.EDGE_CASES)), ids=[c[0] for c in bref.EDGE_CASES])
def test_window_edges_at_every_pointer_offset_and_segment_start(index, in_offset):
    case = bref.EDGE_CASES[index]
    name, lines, cut, _, _ = case
    for flags in (0, bref.SHORTEST):
        with Opened(ref.parse_lines(lines), cut, flags, lines) as o:
            for lead in (0, 1, 2, 3):
                data, offsets = bref.edge_batch(case, lead)
                want, want_first = edge_model(index, flags, lead)
                o.all_forms(data, offsets, want, want_first, f"{name}/flags {flags}/pointer {in_offset}/lead {lead}", in_offset, host_form=in_offset == 0)
                by_hand = bref.edge_want(case, flags, lead)
                assert by_hand is None or bref.triples(want) == by_hand
            # the second oracle: the library's own plain device call on each segment alone
            data, offsets = bref.edge_batch(case, in_offset)
            want, _ = edge_model(index, flags, in_offset)
            own = [[], [], []]
            for lo, hi in zip(offsets[:-1].tolist(), offsets[1:].tolist()):
                if hi > lo:
                    d_in, address = device_input(data[lo:hi], (in_offset + lo) % 4)
                    arrays = [torch.full((hi - lo + 8,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(3)]
                    _, total = o.sg.match_device(address, hi - lo, *[a.data_ptr() for a in arrays], hi - lo + 8)
                    torch.cuda.synchronize()
                    for col, a, shift in zip(own, (arrays[1], arrays[0], arrays[2]), (lo, 0, lo)):
                        col += (a[:total].cpu().numpy() + shift).tolist()
            ref.same(own, want, f"{name}/flags {flags}: the plain call per segment")


# ---------------------------------------------------------------- 2. the segment search and segFirst


def run_case(o, n, offsets, what, in_offset=0):
    want, want_first = bref.run_want(offsets)
    o.all_forms(b"a" * n, offsets, want, want_first, what, in_offset, host_form=False)
    return want


@pytest.mark.parametrize("pairs", [BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1])
def test_pair_counts_around_one_block_with_the_segment_changing_inside_a_block_and_at_its_edge(pairs):
    with Opened(ref.parse_lines(bref.RUN_LINES), lines=bref.RUN_LINES) as o:
        run_case(o, pairs, [0, pairs], f"{pairs} pairs in one segment")
        run_case(o, pairs, [0, 100, pairs], f"{pairs} pairs, a cut inside the first block")
        run_case(o, pairs, [0, min(BLOCK, pairs), pairs], f"{pairs} pairs, a cut at the block's edge")
        run_case(o, pairs, [0, BLOCK - 1, min(BLOCK, pairs), min(BLOCK + 1, pairs), pairs], f"{pairs} pairs, one-byte segments around the edge")
        want = run_case(o, pairs, [0, 0, 0, 7, 19, 19, 19, 19, 20, 22, pairs, pairs, pairs], f"{pairs} pairs, runs of empty segments")
        assert want[0].size == pairs - 5


@pytest.mark.parametrize("segments", [BOUNDS - 2, BOUNDS - 1, BOUNDS, BOUNDS + 1])
def test_one_pair_per_one_byte_segment_and_segment_counts_around_the_bounds_block(segments):
    """numSegments + 1 offsets: BOUNDS - 1, BOUNDS, BOUNDS + 1 and BOUNDS + 2 entries; seven of the segments are empty, the others hold the one
    byte of a one-byte anchor: one entry each, and segFirst counts them"""
    lines = ["a[0-9]?", "ab"]
    n = segments - 7
    cuts = np.arange(n + 1)
    offsets = np.concatenate([[0, 0], cuts[:n // 2 + 1], [n // 2] * 3, cuts[n // 2 + 1:], [n, n]])
    assert offsets.size == segments + 1 and np.all(np.diff(offsets) >= 0)
    lengths = np.diff(offsets)
    pos = offsets[:-1][lengths == 1]
    want = (pos.astype(np.int32), np.ones(n, np.int32), (pos + 1).astype(np.int32))
    want_first = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    with Opened(ref.parse_lines(lines), lines=lines) as o:
        o.all_forms(b"a" * n, offsets, want, want_first, f"{segments} segments", in_offset=1, host_form=segments == BOUNDS)


def test_one_pairs_list_past_a_single_grid_pass_and_a_list_that_does_not_ascend():
    """every pair decides on its own, so a list that names each position of a 4 KiB input many times gives each entry that many times"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pairs, n = PER_CU * cus * BLOCK + 1, 4096
    offsets = np.concatenate([np.arange(0, n, 61), [n]])
    with Opened(ref.parse_lines(bref.RUN_LINES)) as o:
        d_in, address = device_input(np.full(n, 0x61, dtype=np.uint8))
        pair_pos = (np.arange(pairs, dtype=np.int64) * n // pairs).astype(np.int32)
        hi = offsets[np.searchsorted(offsets, pair_pos, side="right")]              # the end of each pair's segment
        keep = pair_pos <= hi - 2
        st, (pos, ids, end), first, total = run_batch(o.sg, d_in, address, n, offsets, pairs, pairs=(np.ones(pairs, dtype=np.int32), pair_pos))
        assert st == 0 and total == int(keep.sum())
        assert np.array_equal(pos, pair_pos[keep]) and bool((ids == 1).all()) and np.array_equal(end, np.minimum(pair_pos[keep] + 3, hi[keep]))
        assert first.tolist() == np.searchsorted(pair_pos[keep], offsets, side="left").tolist()
        # the same pairs back to front, a thousand of them: each pair's entries are right, in the list's order
        back, hi_back = pair_pos[::-1][:1000].copy(), hi[::-1][:1000]
        keep = back <= hi_back - 2
        st, (pos, ids, end), _, total = run_batch(o.sg, d_in, address, n, offsets, 1000, pairs=(np.ones(1000, dtype=np.int32), back))
        assert st == 0 and total == int(keep.sum())
        assert np.array_equal(pos, back[keep]) and np.array_equal(end, np.minimum(back[keep] + 3, hi_back[keep]))


# ---------------------------------------------------------------- 3. offsets no caller should pass


@pytest.mark.parametrize("what,make", bref.HOSTILE, ids=[w for w, _ in bref.HOSTILE])
def test_hostile_device_offsets_give_the_list_of_the_clamped_ones(what, make):
    lines = ["k=[0-9]{1,5}", "(?<![0-9])[0-9]{1,2}k(?![0-9])"]
    data = b"k=12 k=345 k=6789 k=1 12k=5 k=77k"
    n = len(data)
    hostile = make(n)
    clamped = bref.clamp_offsets([min(int(v), 2 ** 62) for v in hostile], n)
    with Opened(ref.parse_lines(lines), lines=lines) as o:
        want, want_first = bref.batch_model(o.sigs, data, clamped, o.anchors, 0, lines)
        assert want[0].size >= 3
        for in_offset in (0, 3):
            d_in, address = device_input(data, in_offset)
            st, got, first, total = run_batch(o.sg, d_in, address, n, hostile, n + 3)
            assert st == 0
            ref.same(got, want, f"{what}/device")
            assert first.tolist() == want_first.tolist()
            st, got, first, total = run_batch(o.sg, d_in, address, n, hostile, n + 3, pairs=longest_pairs(o.h, address, n))
            ref.same(got, want, f"{what}/pairs")
            assert first.tolist() == want_first.tolist()
        offs = np.array(hostile, dtype=np.uint64)
        buf = as_array(data).copy()
        st, _ = o.sg.match_batch_host(buf.ctypes.data, n, offs.ctypes.data, offs.size - 1, None, None, None, 0, check=False)
        assert st == INVALID, "the host form refuses the same array"


# ---------------------------------------------------------------- 4. equalities, capacity, refusals


def test_one_segment_is_the_plain_call():
    for name, lines, data, cut, flags in ref.CASES[:12]:
        with Opened(ref.parse_lines(lines), cut, flags, lines) as o:
            n = len(data)
            d_in, address = device_input(data, 1)
            arrays = [torch.full((n + 8,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(3)]
            _, total = o.sg.match_device(address, n, *[a.data_ptr() for a in arrays], n + 8)
            torch.cuda.synchronize()
            plain = tuple(a[:total].cpu().numpy() for a in (arrays[1], arrays[0], arrays[2]))
            o.all_forms(data, [0, n], plain, [0, total], name, 1)


def test_the_gapsig_cross_check_segment_by_segment():
    from tests import gapsig_ref
    gap_lines = ["4D 5A {2-6} 50 45 00", "E8 ?? ?? [0-8] 5? C3", "61 62 {0-3} ?A 63 64 {1-2} 65"]
    cls_lines = ["MZ.{2,6}PE\\x00", "\\xe8.{2}.{0,8}[P-_]\\xc3", "ab.{0,3}[\\x0a\\x1a*:JZjz\\x8a\\x9a\\xaa\\xba\\xca\\xda\\xea\\xfa]cd.{1,2}e"]
    data = np.random.default_rng(11).integers(0, 256, 3000, dtype=np.uint8)
    gapsig_ref.embed(gapsig_ref.parse_lines(gap_lines), data, 5, per_sig=6)
    cuts = np.sort(np.random.default_rng(12).choice(np.arange(1, 3000), size=40, replace=False))
    offsets = np.concatenate([[0], cuts, [3000]])
    d_in, address = device_input(data, 2)
    h = api.PFAC.create()
    try:
        per_segment = []
        with h.gapsigOpenText(gapsig_ref.text_of(gap_lines)) as gs:
            arrays = [torch.full((3000,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(3)]
            for lo, hi in zip(offsets[:-1].tolist(), offsets[1:].tolist()):
                _, total = gs.match_device(address + lo, hi - lo, *[a.data_ptr() for a in arrays], 3000)
                torch.cuda.synchronize()
                ids, pos, end = (a[:total].cpu().numpy() for a in arrays)
                per_segment += zip(ids.tolist(), (pos + lo).tolist(), (end + lo).tolist())
        with h.clsigOpenText(ref.text_of(cls_lines), 0, ref.SHORTEST) as sg:
            st, got, _, _ = run_batch(sg, d_in, address, 3000, offsets, 3000)
        assert st == 0 and len(per_segment) >= 6 and bref.triples(got) == sorted(per_segment)
    finally:
        h.destroy()


def test_truncation_with_and_without_the_end_and_seg_first_arrays_and_the_refusals():
    case = next(c for c in bref.EDGE_CASES if c[0] == "full-boundary-classes")
    data, offsets = bref.edge_batch(case, 1)
    n = int(data.size)
    with Opened(ref.parse_lines(case[1]), lines=case[1]) as o:
        want, want_first = bref.batch_model(o.sigs, data, offsets, o.anchors, 0)
        total = int(want[0].size)
        assert total == 6
        d_in, address = device_input(data)
        pairs = longest_pairs(o.h, address, n)
        for cap in (0, 1, total - 1, total):
            for with_end in (True, False):
                for with_first in (True, False):
                    st, got, first, full = run_batch(o.sg, d_in, address, n, offsets, cap, pairs, with_end, with_first)
                    assert (st, full) == (TRUNCATED if cap < total else 0, total)
                    ref.same(got[:2], tuple(w[:cap] for w in want[:2]), f"pairs/capacity {cap}")
                    assert not with_end or got[2].tolist() == want[2][:cap].tolist()
                    assert not with_first or first.tolist() == want_first.tolist(), "segFirst names entries past capacity too"
        for with_end, with_first in ((False, True), (True, False), (False, False)):
            st, got, first, full = run_batch(o.sg, d_in, address, n, offsets, n + 3, None, with_end, with_first)
            assert st == 0 and full == total
            ref.same(got[:2], want[:2], "device/without an array")
        # no pairs at all: segFirst is all zero
        st, got, first, full = run_batch(o.sg, d_in, address, n, offsets, 4, pairs=(np.zeros(0, np.int32), np.zeros(0, np.int32)))
        assert (st, full) == (0, 0) and first.tolist() == [0] * len(offsets)
        d_none, none_address = device_input(b"." * n)
        st, got, first, full = run_batch(o.sg, d_none, none_address, n, offsets, n)
        assert (st, full) == (0, 0) and first.tolist() == [0] * len(offsets)
        # the refusals: nothing is written
        d_off, off_ptr = device_offsets(offsets)
        segs = len(offsets) - 1
        t = torch.full((6 * n,), POISON, dtype=torch.int32, device="cuda:0")
        base = t.data_ptr()
        free = [base + 8 * n, base + 12 * n, base + 16 * n]
        calls = [
            o.sg.match_batch_device(address, n, off_ptr, segs, *free, n - 1, None, check=False),
            o.sg.match_batch_device(address, n, None, segs, *free, n, None, check=False),
            o.sg.match_batch_device(address, n, off_ptr, 0, *free, n, None, check=False),
            o.sg.match_batch_device(address, n, off_ptr, 2 ** 31 - 1, *free, n, None, check=False),
            o.sg.match_batch_device(address, 1 << 31, off_ptr, segs, *free, 1 << 31, None, check=False),
            o.sg.match_batch_device(address, n, off_ptr, segs, None, free[1], None, n, None, check=False),
            o.sg.batch_pairs_device(address, n, None, segs, base, base + 4 * n, 4, *free, n, None, check=False),
            o.sg.batch_pairs_device(address, n, off_ptr, segs, base, base + 4 * n, 4, None, None, None, 1, None, check=False),
            o.sg.batch_pairs_device(address, n, off_ptr, segs, base, base + 4 * n, 4, base + 8, free[1], free[2], n, None, check=False),
            o.sg.batch_pairs_device(address, n, off_ptr, segs, base, base + 4 * n, 4, free[0], free[1], base + 4 * n + 12, n, None, check=False),
        ]
        torch.cuda.synchronize()
        assert [st for st, _ in calls] == [INVALID] * len(calls)
        assert bool((t == POISON).all())
        assert o.sg.match_batch_device(address, 0, off_ptr, 0, None, None, None, 0, None, check=False) == (INVALID, 0), "null arrays"
        assert o.sg.match_batch_device(address, 0, off_ptr, 0, *free, 0, None, check=False) == (0, 0), "size 0"


# ---------------------------------------------------------------- 5. the seeded random case


def test_200_random_signatures_over_64_kib_cut_at_seeded_offsets():
    sigs, data, offsets = bref.random_batch()
    with Opened(sigs) as o:
        flat, _ = ref.fast_list(sigs, data, o.anchors)
        want, want_first = bref.batch_model(sigs, data, offsets, o.anchors, fast=True)
        lost, freed = bref.crossing_figures(flat, want)
        print({"segments": offsets.size - 1, "flat": int(flat[0].size), "batch": int(want[0].size), "lost": lost, "freed": freed})
        assert lost >= 20, "crossings: entries of the flat list that the batch list must not have"
        assert freed >= 5, "boundary classes freed by a segment edge: entries the flat list cannot have"
        o.all_forms(data, offsets, want, want_first, "random, cut", in_offset=1)
        assert bref.triples(flat) != bref.triples(want), "the flat list fails this comparison"
