"""PFACX_groupsMatchFromDevice / PFACX_groupsPairsFromDevice / PFACX_groupsMatchFromHost (GPU platform) against the reference of tests/groups_ref.py:
every case of the table at two input alignments, random cases in every kernel variant and mode, the block and wave edges of the pass, more pairs
than one grid pass takes with several hundred thousand segments, one segment over many blocks, ALL with truncation, one input above the 32 MiB
switch, a 100 000-pattern set, the pairs form over the reduce list, over a hostile list and over the pairs of a flows call, the accounting.  All
arrays are poisoned and carry guard words on both sides."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import allmatch_ref as am  # noqa: E402
from tests import groups_ref as ref  # noqa: E402
from tests import scale_sets as ss  # noqa: E402
from tests.gpu_helpers import MODES, VARIANTS, make_handle  # noqa: E402
from tests.spans_helpers import pattern_file  # noqa: E402
from tests.test_count_gpu import prefix_of, scale_text  # noqa: E402  (cached for the session: the prefix table of 100 000 patterns is built once)
from tests.test_groups_host import small_random_case, u64  # noqa: E402

ALL = api.PFACX_GROUPS_ALL
BLOCK = api.PFACX_GROUPS_BLOCK              # scan_groups.hip: kGroupsBlock
GUARD = 64
POISON = -5
INVALID, TRUNCATED = api.STATUS.INVALID_PARAMETER, api.STATUS.OUTPUT_TRUNCATED


def as_array(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)


def gpu_handle(pf, flags=0, variant=api.PFACX_KERNEL_AUTO, perf=api.PFAC_TIME_DRIVEN, tex=api.PFAC_TEXTURE_OFF):
    h = api.PFAC.create()
    h.setPerfMode(perf)
    h.setTextureMode(tex)
    h.setKernelVariant(variant)
    h.readPatternFromFileEx(pf, flags)
    return h


def dev64(values):
    """64-bit words on the device (torch has no uint64 arithmetic: the bits travel as int64)"""
    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")


def poisoned(count, dtype):
    return torch.full((GUARD + count + GUARD,), POISON, dtype=dtype, device="cuda:0")


def inner(t, count, width):
    return t.data_ptr() + width * GUARD if count or width == 8 else None


def outputs(capacity, segments):
    return poisoned(capacity, torch.int32), poisoned(capacity, torch.int32), poisoned(segments + 1, torch.int64), poisoned(segments, torch.int64)


def collect(st, total, capacity, segments, d_ids, d_pos, d_first, d_hit, on_device=False):
    """the guards, then (pos, ids, segFirst, segGroups) of what was written"""
    torch.cuda.synchronize()
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > capacity), (st, total, capacity)
    k = min(total, capacity)
    for a, n in ((d_ids, capacity), (d_pos, capacity), (d_first, segments + 1), (d_hit, segments)):
        assert bool((a[:GUARD] == POISON).all()) and bool((a[GUARD + n:] == POISON).all()), "wrote outside the arrays"
    for a in (d_ids, d_pos):
        assert bool((a[GUARD + k:GUARD + capacity] == POISON).all()), "wrote behind the list"
    pos, ids = d_pos[GUARD:GUARD + k], d_ids[GUARD:GUARD + k]
    first, hit = d_first[GUARD:GUARD + segments + 1].cpu().numpy().view(np.uint64), d_hit[GUARD:GUARD + segments].cpu().numpy().view(np.uint64)
    return (pos, ids, first, hit) if on_device else (pos.cpu().numpy(), ids.cpu().numpy(), first, hit)


def device_groups(g, data, offsets, seg_masks, flags, in_offset=0, capacity=None, on_device=False):
    """match_device -> (status, (pos, ids, segFirst, segGroups), the full length).  capacity=None: the count query with null arrays first, then
    arrays of exactly that length.  Nothing outside what the contract names may be written, and the input must stay untouched"""
    data = as_array(data)
    n = int(data.size)
    d_in = torch.zeros(n + in_offset + 64, dtype=torch.uint8, device="cuda:0")
    src = torch.from_numpy(data.copy()).to("cuda:0")
    d_in[in_offset:in_offset + n] = src
    segments = 1 if offsets is None else len(offsets) - 1
    d_off = None if offsets is None else dev64(offsets)
    d_sm = None if seg_masks is None else dev64(u64(seg_masks))
    optr, mptr = (None if t is None else t.data_ptr() for t in (d_off, d_sm))
    if capacity is None:
        st, capacity = g.match_device(d_in.data_ptr() + in_offset, n, optr, segments, mptr, flags, None, None, 0, None, None, check=False)
        assert st == (TRUNCATED if capacity else 0)
    d_ids, d_pos, d_first, d_hit = outputs(capacity, segments)
    st, total = g.match_device(d_in.data_ptr() + in_offset, n, optr, segments, mptr, flags, inner(d_ids, capacity, 4), inner(d_pos, capacity, 4), capacity,
                               inner(d_first, 1, 8), inner(d_hit, 1, 8), check=False)
    got = collect(st, total, capacity, segments, d_ids, d_pos, d_first, d_hit, on_device)
    assert torch.equal(d_in[in_offset:in_offset + n], src), "the caller's input was modified"
    assert bool((d_in[:in_offset] == 0).all()) and bool((d_in[in_offset + n:] == 0).all())
    return st, got, total


def device_pairs(g, pair_ids, pair_pos, seg_first_pairs, segments, seg_masks, flags, capacity):
    """pairs_device over a pair list on the host -> (status, (pos, ids, segFirst, segGroups), the full length); the caller's lists stay as they were"""
    d_pi, d_pp = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to("cuda:0") for a in (pair_ids, pair_pos))
    d_sf = None if seg_first_pairs is None else torch.from_numpy(np.ascontiguousarray(seg_first_pairs, dtype=np.int32)).to("cuda:0")
    d_sm = None if seg_masks is None else dev64(u64(seg_masks))
    d_ids, d_pos, d_first, d_hit = outputs(capacity, segments)
    st, total = g.pairs_device(d_pi.data_ptr(), d_pp.data_ptr(), len(pair_ids), None if d_sf is None else d_sf.data_ptr(), segments,
                               None if d_sm is None else d_sm.data_ptr(), flags, inner(d_ids, capacity, 4), inner(d_pos, capacity, 4), capacity,
                               inner(d_first, 1, 8), inner(d_hit, 1, 8), check=False)
    got = collect(st, total, capacity, segments, d_ids, d_pos, d_first, d_hit)
    assert np.array_equal(d_pi.cpu().numpy(), pair_ids) and np.array_equal(d_pp.cpu().numpy(), pair_pos), "the caller's pair list was modified"
    if d_sf is not None:
        assert np.array_equal(d_sf.cpu().numpy(), seg_first_pairs)
    return st, got, total


# ---------------------------------------------------------------- the table, random cases


@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_on_the_device_form_and_the_host_form(workdir, case):
    name, pats, masks, data, offsets, seg_masks, nocase = case
    h = gpu_handle(pattern_file(workdir, "groups_gpu_" + name, pats), api.PFACX_READ_NOCASE if nocase else 0)
    cpu = api.PFAC.createHostOnly()
    try:
        cpu.readPatternFromFileEx(pattern_file(workdir, "groups_gpu_" + name, pats), api.PFACX_READ_NOCASE if nocase else 0)
        g = h.groupsOpen(u64(masks))
        for flags in (0, ALL):
            want = ref.groups_ref(pats, masks, data, offsets, seg_masks, bool(flags), nocase)
            for in_offset in (0, 3):
                st, got, total = device_groups(g, data, offsets, seg_masks, flags, in_offset)
                assert st == 0 and total == want[0].size
                ref.same(got, want, f"{name}/flags {flags}/input at +{in_offset}")
            args = (as_array(data), u64(masks), offsets, None if seg_masks is None else u64(seg_masks), bool(flags))
            on_gpu = h.match_groups_host_array(*args)                                      # the host form on the GPU platform ...
            ref.same(on_gpu, want, f"{name}/flags {flags}: the host form on the GPU platform")
            ref.same(on_gpu, cpu.match_groups_host_array(*args), f"{name}/flags {flags}: ... equals the CPU platform's")
        if name == "foo-foobar-masks-1-2-3-0":
            got = device_groups(g, data, offsets, seg_masks, 0)[1]
            shortcut = ref.longest_filter(pats, masks, data, offsets, seg_masks)
            assert got[0].tolist() == [0] + shortcut[0].tolist(), "filter the longest pairs: foo at 0, under foobar of group 1, would be lost"
        g.close()
    finally:
        cpu.destroy()
        h.destroy()


@pytest.mark.parametrize("perf,tex,mode_name", MODES, ids=[m[2] for m in MODES])
@pytest.mark.parametrize("variant,vname", VARIANTS, ids=[v[1] for v in VARIANTS])
def test_random_cases_every_variant_and_mode(workdir, variant, vname, perf, tex, mode_name):
    for seed in (3, 8, 14, 22):
        pats, masks, data, offsets, seg_masks = small_random_case(seed)
        lists, folded = ref.segment_lists(pats, data, offsets)
        m = ref.resolve_masks(folded, masks)
        h = make_handle(pattern_file(workdir, f"groups_gpu_random{seed}", pats), perf, tex, variant)
        try:
            g = h.groupsOpen(u64(masks))
            for flags in (0, ALL):
                want = ref.filter_lists(lists, m, seg_masks, bool(flags))
                st, got, total = device_groups(g, data, offsets, seg_masks, flags)
                assert st == 0 and total == want[0].size
                ref.same(got, want, f"seed {seed}/{vname}/{mode_name}/flags {flags}")
        finally:
            h.destroy()                                                                     # (with the table open)


# ---------------------------------------------------------------- the edges of the pass: pattern a, mask 1, n bytes of a


def run_of_a(workdir):
    h = gpu_handle(pattern_file(workdir, "groups_gpu_a", [b"a"]))
    return h, h.groupsOpen(u64([0, 1]))


def want_of_a(offsets, seg_masks):
    """one pair per byte; a segment is reported iff bit 0 of its mask is set"""
    on = [1 if seg_masks is None else int(seg_masks[k]) & 1 for k in range(len(offsets) - 1)]
    keep = np.concatenate([np.full(int(offsets[k + 1] - offsets[k]), on[k], dtype=bool) for k in range(len(on))]) if on else np.zeros(0, dtype=bool)
    pos = np.flatnonzero(keep).astype(np.int32)
    first = np.concatenate([[0], np.cumsum([int(offsets[k + 1] - offsets[k]) * on[k] for k in range(len(on))])]).astype(np.uint64)
    hit = np.array([on[k] if offsets[k + 1] > offsets[k] else 0 for k in range(len(on))], dtype=np.uint64)
    return pos, np.ones(pos.size, dtype=np.int32), first, hit


@pytest.mark.parametrize("pairs", [63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1])
def test_pair_counts_and_segment_cuts_around_the_wave_and_the_block(workdir, pairs):
    h, g = run_of_a(workdir)
    try:
        n = pairs + 130 if pairs < 100 else pairs + 300
        data = b"a" * n
        cuts = [[0, n]] + [[0, c, n] for c in (63, 64, 65, 255, 256, 257) if c < n] + [[0, 0, 63, 63, 64, 65, 65, 65, 65, n, n]] + [list(range(n + 1))]
        for offsets in cuts + [[0, pairs, n]]:
            for sm in (None, [(k % 3 != 1) * 1 for k in range(len(offsets) - 1)]):
                for flags in (0, ALL):
                    st, got, total = device_groups(g, data, offsets, sm, flags)
                    ref.same(got, want_of_a(offsets, sm), f"{pairs} pairs/{len(offsets) - 1} segments/masks {sm is not None}/flags {flags}")
        st, got, total = device_groups(g, b"a" * pairs, None, None, 0)                     # exactly `pairs` pairs, one segment, no array
        assert total == pairs and got[2].tolist() == [0, pairs] and got[3].tolist() == [1]
    finally:
        h.destroy()


def test_more_pairs_than_one_grid_pass_takes_in_several_hundred_thousand_segments(workdir):
    h, g = run_of_a(workdir)
    try:
        n = (1 << 20) + 77
        assert n > 8 * BLOCK * int(h.info().multiProcessorCount), "more pairs than blocks x 256: a block walks its pairs in several trips"
        rng = np.random.Generator(np.random.PCG64(5))
        steps = rng.integers(1, 4, size=n)                                                  # segments of 1 to 3 bytes, an empty one now and then
        steps[rng.integers(0, n, size=2000)] = 0
        offsets = np.concatenate([[0], np.cumsum(steps)])
        offsets = np.concatenate([offsets[offsets < n], [n, n, n]]).astype(np.uint64)
        segments = offsets.size - 1
        assert segments > 300000
        sm = np.where(np.arange(segments) % 3 == 2, 0, 1 + 2 * (np.arange(segments) % 5)).astype(np.uint64)    # every third segment sees nothing
        st, got, total = device_groups(g, np.full(n, ord("a"), dtype=np.uint8), offsets, sm, 0, on_device=True)
        want = want_of_a(offsets, sm)
        assert st == 0 and total == want[0].size
        assert torch.equal(got[0].cpu(), torch.from_numpy(want[0])) and bool((got[1] == 1).all())
        ref.same((None, None, got[2], got[3]), want, "segFirst with its empty runs, segGroups through the atomics")
    finally:
        h.destroy()


def test_one_segment_over_many_blocks_collects_the_groups_of_hits_far_apart(workdir):
    pats = [b"a", b"xyz", b"xyzw", b"q"]
    masks = [0, 1, 1 << 40, 1 << 63, 1 << 7]
    n = 300000
    data = np.full(n, ord("a"), dtype=np.uint8)
    data[5:9] = np.frombuffer(b"xyzw", dtype=np.uint8)                                      # xyzw: group 63, and its prefix xyz: group 40
    data[n - 2] = ord("q")                                                                  # group 7, a thousand blocks away
    h = gpu_handle(pattern_file(workdir, "groups_gpu_far", pats))
    try:
        g = h.groupsOpen(u64(masks))
        st, got, total = device_groups(g, data, [0, 3, n - 1, n], [ref.ALL_BITS, (1 << 40) | (1 << 7) | 1, 1 << 7], 0, on_device=True)
        assert got[3].tolist() == [1, (1 << 40) | (1 << 7) | 1, 0], "the OR of a segment that spans many waves and blocks; xyzw's own bit is not enabled"
        assert got[2].tolist() == [0, 3, n - 4, n - 4] and total == n - 4                   # segment 1: [3, n - 1) without 6, 7, 8 (y, z, w); a at n - 1 is not enabled
        assert got[1][5].item() == 2 and got[0][5].item() == 5, "xyz, the longest ENABLED pattern at 5"
    finally:
        h.destroy()


def test_all_with_truncation_keeps_segfirst_seggroups_and_the_count_complete(workdir):
    name, pats, masks, data, offsets, seg_masks, nocase = ref.CASES[9]                     # nested a, two segments, every other group
    data, offsets = data * 60, [0, 5, 12 * 60]
    h = gpu_handle(pattern_file(workdir, "groups_gpu_trunc", pats))
    try:
        g = h.groupsOpen(u64(masks))
        want = ref.groups_ref(pats, masks, data, offsets, seg_masks, True)
        total = want[0].size
        assert total > len(data)
        for capacity in (0, 1, BLOCK + 1, total - 1, total):
            st, got, n = device_groups(g, data, offsets, seg_masks, ALL, capacity=capacity)
            assert n == total and st == (TRUNCATED if capacity < total else 0)
            ref.same(got, (want[0][:capacity], want[1][:capacity], want[2], want[3]), f"capacity {capacity}")
    finally:
        h.destroy()


# ---------------------------------------------------------------- big inputs, big sets


def id_masks(count):
    """masks derived from the id: a bit below 32, one above, and for every 7th id none"""
    ids = np.arange(count + 1, dtype=np.uint64)
    m = (np.uint64(1) << (ids % np.uint64(29))) | (np.uint64(1) << (np.uint64(33) + ids % np.uint64(30)))
    m[ids % np.uint64(7) == 0] = 0
    m[0] = 0
    return m


def check_against_result(h, pats, data, result, offsets, seg_masks, what):
    prefix, chain = prefix_of(tuple(pats))
    lengths = [0] + [len(p) for p in pats]
    masks = id_masks(len(pats))
    clipped = ref.clip_to_segments(result, offsets, prefix, lengths)
    pair_pos = np.flatnonzero(clipped > 0)
    bounds = np.searchsorted(pair_pos, np.asarray(offsets, dtype=np.int64))
    g = h.groupsOpen(masks)
    for flags in (0, ALL):
        want = ref.groups_from_pairs(pair_pos, clipped[pair_pos], bounds, len(offsets) - 1, prefix, ref.resolve_masks(pats, masks), seg_masks, bool(flags))
        st, got, total = device_groups(g, data, offsets, seg_masks, flags, on_device=True)
        assert st == 0 and total == want[0].size, (what, flags, total, want[0].size)
        assert torch.equal(got[0].cpu(), torch.from_numpy(want[0])) and torch.equal(got[1].cpu(), torch.from_numpy(want[1])), f"{what}/flags {flags}"
        ref.same((None, None, got[2], got[3]), want, f"{what}/flags {flags}")
    g.close()
    return want


def test_big_input_through_the_filter_kernel():
    data, result, density = ss.density_stream(0.10)
    assert data.size == ss.BIG
    pats = ss.patterns(ss.C3)
    n = int(data.size)
    h = make_handle(ss.pattern_file(ss.C3), api.PFAC_SPACE_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        want = check_against_result(h, pats, data, result, [0, 1 << 20, (33 << 20) + 5, n - 3, n], [ref.ALL_BITS, 0xFFFF, ref.ALL_BITS >> 32 << 32, 1], f"{n} bytes")
        assert want[0].size > 1000
    finally:
        h.destroy()


def test_a_100_000_pattern_set_against_the_filtered_all_match_batch_list():
    pats = tuple(ss.patterns(ss.S100))
    data = scale_text(pats)
    pf = ss.pattern_file(ss.S100)
    n = int(data.size)
    offsets = np.arange(0, n + 1500, 1500, dtype=np.uint64)
    offsets[-1] = n
    segments = offsets.size - 1
    seg_masks = np.where(np.arange(segments) % 4 == 0, np.uint64(ref.ALL_BITS), np.uint64(0x0000FFFF0000FF0F)).astype(np.uint64)
    h = make_handle(pf, api.PFAC_SPACE_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        want = check_against_result(h, pats, data, ss.want(pf, data), offsets, seg_masks, "S100")
        assert want[0].size > 1000
        # the do-it-yourself path in torch: the all-match batch list, gather of masks, gather of segment masks, AND, masked select
        masks = id_masks(len(pats))
        cap = n * max(1, int(h.info().maxMatchesPerPosition))
        d_in, d_off = torch.from_numpy(data.copy()).to("cuda:0"), dev64(offsets)
        d_ids, d_pos = (torch.full((cap,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
        d_first = torch.zeros(segments + 1, dtype=torch.int64, device="cuda:0")
        _, count = h.matchAllBatchFromDevice(d_in.data_ptr(), n, d_off.data_ptr(), segments, d_ids.data_ptr(), d_pos.data_ptr(), cap, d_first.data_ptr())
        torch.cuda.synchronize()
        ids, pos = d_ids[:count].long(), d_pos[:count]
        seg = torch.searchsorted(d_first[1:].contiguous(), torch.arange(count, device="cuda:0"), right=True)
        keep = (dev64(masks)[ids] & dev64(seg_masks)[seg]) != 0
        g = h.groupsOpen(masks)
        st, got, total = device_groups(g, data, offsets, seg_masks, ALL, on_device=True)
        assert total == int(keep.sum()) and torch.equal(got[0], pos[keep]) and torch.equal(got[1].long(), ids[keep])
    finally:
        h.destroy()


# ---------------------------------------------------------------- the pairs form


PAIR_PATS = [b"foo", b"foobar", b"bar", b"o", b"foob"]
PAIR_MASKS = [0, 1, 2, 4, 1 << 35, 1 << 63]


def test_pairs_form_over_the_batch_reduce_list_equals_the_scanning_form(workdir):
    data = as_array(b"foo bar foobar,foobarx foo o oo foob|bar foo" * 30)
    n = int(data.size)
    offsets = np.array([0, 5, 13, 14, 14, 100, n], dtype=np.uint64)
    seg_masks = [1, 2 | 4, ref.ALL_BITS, 1, (1 << 35) | (1 << 63), 3]
    h = gpu_handle(pattern_file(workdir, "groups_gpu_pairs", PAIR_PATS))
    try:
        g = h.groupsOpen(u64(PAIR_MASKS))
        d_in, d_off = torch.from_numpy(data.copy()).to("cuda:0"), dev64(offsets)
        d_ids, d_pos = (torch.full((n,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
        d_seg = torch.full((offsets.size,), POISON, dtype=torch.int32, device="cuda:0")
        _, count = h.matchBatchFromDeviceReduce(d_in.data_ptr(), n, d_off.data_ptr(), offsets.size - 1, d_ids.data_ptr(), d_pos.data_ptr(), d_seg.data_ptr())
        torch.cuda.synchronize()
        pair_ids, pair_pos, seg_first = d_ids[:count].cpu().numpy(), d_pos[:count].cpu().numpy(), d_seg.cpu().numpy()
        for flags in (0, ALL):
            want = ref.groups_ref(PAIR_PATS, PAIR_MASKS, data.tobytes(), offsets, seg_masks, bool(flags))
            st, scanned, total = device_groups(g, data, offsets, seg_masks, flags)
            ref.same(scanned, want, f"the scanning form/flags {flags}")
            st, got, t2 = device_pairs(g, pair_ids, pair_pos, seg_first, offsets.size - 1, seg_masks, flags, total + 3)
            assert (st, t2) == (0, total)
            ref.same(got, scanned, f"the pairs form over the batch reduce list/flags {flags}")
            assert device_pairs(g, pair_ids, pair_pos, seg_first, offsets.size - 1, seg_masks, flags, 0)[::2] == (TRUNCATED, total)   # the count query
            st, got, t2 = device_pairs(g, pair_ids, pair_pos, seg_first, offsets.size - 1, seg_masks, flags, total - 1)
            assert (st, t2) == (TRUNCATED, total)
            ref.same(got, (want[0][:total - 1], want[1][:total - 1], want[2], want[3]), "capacity = the length minus 1")
        # one segment of all pairs, no array
        want = ref.groups_from_pairs(pair_pos, pair_ids, None, 1, am.prefix_table(PAIR_PATS)[0], PAIR_MASKS, [5], True)
        ref.same(device_pairs(g, pair_ids, pair_pos, None, 1, [5], ALL, count * 3)[1], want, "numSegments == 1 without an array")
    finally:
        h.destroy()


def test_pairs_form_ignores_or_clamps_what_a_hostile_list_holds(workdir):
    f = len(PAIR_PATS)
    pair_ids = np.array([2, 0, -1, f + 1, 5, 2, 1 << 30, 3, 2, 4, -(1 << 31), 2, 5, 1, 2], dtype=np.int32)
    pair_pos = np.array([7, 1, 2, 3, -9, 5, 6, (1 << 31) - 1, 8, -(1 << 31), 10, 11, 12, 13, 14], dtype=np.int32)
    count = pair_ids.size
    # entries below 0 and above numPairs, a decreasing pair (9 -> 4: segment 4 is empty), pairs before the first and behind the last bound
    seg_first = np.array([-5, 1, 1, 9, 4, 12, count + 7, 13], dtype=np.int32)
    seg_first[0] = 1                                                                        # pair 0 lies before the first bound
    hostile = [np.array([-5, 1, 1, 9, 4, 12, count + 7, 13], dtype=np.int32), seg_first, np.array([3, 2, 1, 0], dtype=np.int32),
               np.array([count + 1, -1], dtype=np.int32), np.array([0, 14], dtype=np.int32)]
    prefix = am.prefix_table(PAIR_PATS)[0]
    h = gpu_handle(pattern_file(workdir, "groups_gpu_hostile", PAIR_PATS))
    try:
        g = h.groupsOpen(u64(PAIR_MASKS))
        for sf in hostile:
            segments = sf.size - 1
            sm = [ref.ALL_BITS, 1, 2 | (1 << 63), 0, ref.ALL_BITS, 1 << 35, 7][:segments]
            for flags in (0, ALL):
                want = ref.groups_from_pairs(pair_pos, pair_ids, sf, segments, prefix, PAIR_MASKS, sm, bool(flags))
                st, got, total = device_pairs(g, pair_ids, pair_pos, sf, segments, sm, flags, 3 * count)
                assert (st, total) == (0, want[0].size)
                ref.same(got, want, f"bounds {sf.tolist()}/flags {flags}")
        assert ref.bounds_of(hostile[0], count).tolist() == [0, 1, 1, 9, 9, 12, count, count]
    finally:
        h.destroy()


def test_pairs_form_over_the_pairs_of_a_flows_call_gives_per_flow_groups(workdir):
    pats = [b"needle", b"nee", b"dle", b"hay"]
    masks = [0, 1, 2, 4, 1 << 50]
    h = gpu_handle(pattern_file(workdir, "groups_gpu_flows", pats))
    try:
        g = h.groupsOpen(u64(masks))
        fl = h.flowsOpen(3)
        M = int(h.info().maxPatternLen)
        prefix = am.prefix_table(pats)[0]
        flows = np.array([0, 1, 2], dtype=np.uint32)
        seen = 0
        for buf in (b"hay nee" + b"needle ne" + b"xxx", b"dle hay" + b"edle nee" + b"needle"):
            cuts = np.array([0, 7, 16, len(buf)] if seen == 0 else [0, 7, 15, len(buf)], dtype=np.uintp)
            data = as_array(buf)
            n = int(data.size)
            cap = n + 3 * (M - 1)
            d_in = torch.from_numpy(data.copy()).to("cuda:0")
            d_ids, d_pos = (torch.full((cap,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
            d_first = torch.full((4,), POISON, dtype=torch.int32, device="cuda:0")
            offs = np.zeros(3, np.uint64)
            _, k = fl.match_device(d_in.data_ptr(), n, cuts.ctypes.data, flows.ctypes.data, 3, d_ids.data_ptr(), d_pos.data_ptr(), cap, d_first.data_ptr(),
                                   offs.ctypes.data)
            torch.cuda.synchronize()
            pair_ids, pair_pos, first = d_ids[:k].cpu().numpy(), d_pos[:k].cpu().numpy(), d_first.cpu().numpy()
            if seen:
                assert (pair_pos < 0).any(), "the second call reports matches that began in the carried bytes"
            sm = [1 | 2 | 4, 2 | (1 << 50), ref.ALL_BITS]
            for flags in (0, ALL):
                want = ref.groups_from_pairs(pair_pos, pair_ids, first, 3, prefix, masks, sm, bool(flags))
                st, got, total = device_pairs(g, pair_ids, pair_pos, first, 3, sm, flags, 3 * max(1, k))
                assert (st, total) == (0, want[0].size)
                ref.same(got, want, f"flows call {seen}/flags {flags}")
            seen += 1
        fl.close()
    finally:
        h.destroy()


def test_pairs_form_refuses_overlapping_arrays(workdir):
    h = gpu_handle(pattern_file(workdir, "groups_gpu_overlap", PAIR_PATS))
    try:
        g = h.groupsOpen(u64(PAIR_MASKS))
        a = torch.ones(64, dtype=torch.int32, device="cuda:0")
        b = torch.ones(64, dtype=torch.int32, device="cuda:0")
        c = torch.full((64,), POISON, dtype=torch.int32, device="cuda:0")
        for ids, pos in ((a.data_ptr(), c.data_ptr()), (c.data_ptr(), b.data_ptr() + 4 * 31), (b.data_ptr() + 4, c.data_ptr()), (c.data_ptr(), a.data_ptr())):
            assert g.pairs_device(a.data_ptr(), b.data_ptr(), 32, None, 1, None, 0, ids, pos, 32, None, None, check=False)[0] == INVALID
        assert g.pairs_device(a.data_ptr(), b.data_ptr(), 32, None, 1, None, 0, a.data_ptr() + 4 * 32, b.data_ptr() + 4 * 32, 32, None, None,
                              check=False) == (0, 32)                                       # behind the lists: no overlap
        torch.cuda.synchronize()
        assert bool((c == POISON).all()) and bool((a[:32] == 1).all())
    finally:
        h.destroy()


# ---------------------------------------------------------------- accounting


def test_table_and_scratch_accounting(workdir):
    h = gpu_handle(pattern_file(workdir, "groups_gpu_bytes", PAIR_PATS))
    try:
        tables = h.info().deviceTableBytes
        g = h.groupsOpen(u64(PAIR_MASKS))
        assert h.info().deviceTableBytes == tables, "the mask table is made by the first device call"
        before = h.info().deviceScratchBytes
        data = b"foobar foo bar" * 50
        device_groups(g, data, [0, 100, len(data)], [1, 2], ALL)
        assert h.info().deviceTableBytes == tables + 8 * (len(PAIR_PATS) + 1)
        grown = h.info().deviceScratchBytes
        assert grown > before
        device_groups(g, data, [0, 100, len(data)], [1, 2], ALL)
        assert h.info().deviceScratchBytes == grown, "a second call of the same shape allocates nothing"
        h.trim()
        assert h.info().deviceScratchBytes <= before and h.info().deviceTableBytes == tables + 8 * (len(PAIR_PATS) + 1), "trim keeps the mask table"
        trimmed = h.info().deviceScratchBytes
        want = ref.groups_ref(PAIR_PATS, PAIR_MASKS, data, [0, 100, len(data)], [1, 2], True)
        ref.same(device_groups(g, data, [0, 100, len(data)], [1, 2], ALL)[1], want, "the call works again after the trim")
        h.trim()
        assert h.info().deviceScratchBytes == trimmed, "the scratch returns to its value after trim"
        g.close()
        assert h.info().deviceTableBytes == tables, "close frees the mask table"
    finally:
        h.destroy()
