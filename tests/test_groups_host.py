"""PFACX_groupsOpen / PFACX_groupsMatchFromHost / PFACX_groupsClose on the CPU platforms (host-only handles: no device needed) against the reference
of tests/groups_ref.py: every case of the table in both modes, seeded random cases, both identities of the contract, truncation, every status row,
the generation rule, destroy with an open table, the device forms on a host-only handle."""

import numpy as np
import pytest

from pfac_amd import api
from tests import groups_ref as ref
from tests.groups_ref import test_the_reference_agrees_with_the_lists_worked_out_by_hand  # noqa: F401  (runs here: groups_ref.py is not collected)
from tests.spans_helpers import pattern_file, random_case

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
INVALID, NOT_READY, NOT_EXIST, TRUNCATED, BAD_HANDLE = (api.STATUS.INVALID_PARAMETER, api.STATUS.PATTERNS_NOT_READY, api.STATUS.LIB_NOT_EXIST,
                                                        api.STATUS.OUTPUT_TRUNCATED, api.STATUS.INVALID_HANDLE)
ALL = api.PFACX_GROUPS_ALL
GUARD = 16
POISON64 = 0xDEADDEADDEADDEAD


def host_handle(pf, platform=api.PFAC_PLATFORM_CPU, flags=0):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    h.readPatternFromFileEx(pf, flags)
    return h


def u64(values):
    return np.array([int(v) for v in values], dtype=np.uint64)


def host_groups(g, data, offsets, seg_masks, flags, capacity=None):
    """match_host into poisoned arrays of exactly `capacity` entries (default: the full length, from a count query that is checked too) with GUARD
    poisoned words on both sides of every array -> (status, (pos, ids, segFirst, segGroups), the full length); nothing outside what the contract
    names may change, nor the input"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    n = buf.size
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uintp)
    segments = 1 if off is None else off.size - 1
    sm = None if seg_masks is None else u64(seg_masks)
    optr = None if off is None else off.ctypes.data
    mptr = None if sm is None else sm.ctypes.data
    iptr = buf.ctypes.data if n else np.zeros(1, dtype=np.uint8).ctypes.data
    if capacity is None:                                                                    # the count query: null arrays
        _, capacity = g.match_host(iptr, n, optr, segments, mptr, flags, None, None, 0, None, None, check=False)
    ids, pos = (np.full(GUARD + capacity + GUARD, -7, dtype=np.int32) for _ in range(2))
    first = np.full(GUARD + segments + 1 + GUARD, POISON64, dtype=np.uint64)
    hit = np.full(GUARD + segments + GUARD, POISON64, dtype=np.uint64)
    st, total = g.match_host(iptr, n, optr, segments, mptr, flags, ids.ctypes.data + 4 * GUARD, pos.ctypes.data + 4 * GUARD, capacity,
                             first.ctypes.data + 8 * GUARD, hit.ctypes.data + 8 * GUARD, check=False)
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > capacity), (st, total, capacity)
    k = min(total, capacity)
    for a in (ids, pos):
        assert np.all(a[:GUARD] == -7) and np.all(a[GUARD + capacity:] == -7), "wrote outside the pair arrays"
        assert np.all(a[GUARD + k:GUARD + capacity] == -7), "wrote behind the list"
    for a, m in ((first, segments + 1), (hit, segments)):
        assert np.all(a[:GUARD] == POISON64) and np.all(a[GUARD + m:] == POISON64), "wrote outside segFirst / segGroups"
    assert buf.tobytes() == bytes(data), "the caller's input was modified"
    return st, (pos[GUARD:GUARD + k].copy(), ids[GUARD:GUARD + k].copy(), first[GUARD:GUARD + segments + 1].copy(), hit[GUARD:GUARD + segments].copy()), total


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_equals_the_reference(workdir, case, platform, pname):
    name, pats, masks, data, offsets, seg_masks, nocase = case
    h = host_handle(pattern_file(workdir, "groups_" + name, pats), platform, api.PFACX_READ_NOCASE if nocase else 0)
    try:
        g = h.groupsOpen(u64(masks))
        for flags in (0, ALL):
            want = ref.groups_ref(pats, masks, data, offsets, seg_masks, bool(flags), nocase)
            st, got, total = host_groups(g, data, offsets, seg_masks, flags)
            assert st == 0 and total == want[0].size
            ref.same(got, want, f"{name}/{pname}/flags {flags}")
            if name in ref.WANT:
                ids, pos, first = ref.WANT[name][flags]
                ref.same(got, (pos, ids, first, ref.WANT[name][2]), f"{name}/{pname}/flags {flags}: against the list worked out by hand")
            conv = h.match_groups_host_array(np.frombuffer(data, dtype=np.uint8), u64(masks), offsets, None if seg_masks is None else u64(seg_masks), bool(flags))
            ref.same(conv, want, f"{name}/match_groups_host_array")
        g.close()
    finally:
        h.destroy()


def test_the_longest_enabled_pattern_is_not_a_filter_over_the_longest_pairs(workdir):
    """the shortcut "scan with the union set and filter the longest pairs" loses `foo` at the positions where `foobar`, of another group, is longest"""
    name, pats, masks, data, offsets, seg_masks, nocase = ref.CASES[0]
    h = host_handle(pattern_file(workdir, "groups_shortcut", pats))
    try:
        g = h.groupsOpen(u64(masks))
        st, got, total = host_groups(g, data, offsets, seg_masks, 0)
        shortcut = ref.longest_filter(pats, masks, data, offsets, seg_masks)
        assert got[0].tolist() == [0, 7, 10, 20, 27] and got[1].tolist() == [1, 1, 2, 2, 1]
        assert shortcut[0].tolist() == [7, 10, 20, 27], "filter the longest pairs: foo at 0, under foobar of group 1, is lost"
        assert total == shortcut[0].size + 1
    finally:
        h.destroy()


def small_random_case(seed):
    """the alphabet and pattern generator of tests/spans_helpers.py over an input the brute-force reference walks in milliseconds; masks with a bias
    to few bits (and some zeros), random cuts with empty segments"""
    pats, data = random_case(seed)
    rng = np.random.Generator(np.random.PCG64(77000 + seed))
    data = data[:int(rng.integers(1, 401))]
    few = lambda: int(np.bitwise_or.reduce(np.uint64(1) << rng.integers(0, 64, size=int(rng.integers(0, 3))).astype(np.uint64), initial=np.uint64(0)))  # noqa: E731
    masks = [0] + [few() if rng.random() < 0.8 else int(rng.integers(0, 1 << 63)) * 2 + 1 for _ in pats]
    cuts = np.sort(rng.integers(0, data.size + 1, size=int(rng.integers(0, 12))))
    offsets = [0] + cuts.tolist() + [int(data.size)]
    seg_masks = [few() | few() | few() if rng.random() < 0.7 else ref.ALL_BITS for _ in range(len(offsets) - 1)]
    return pats, masks, data, offsets, seg_masks


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("block", range(6))
def test_random_cases_equal_the_reference(workdir, block, platform, pname):
    for seed in range(block * 30, block * 30 + 30):
        pats, masks, data, offsets, seg_masks = small_random_case(seed)
        lists, folded = ref.segment_lists(pats, data, offsets)
        m = ref.resolve_masks(folded, masks)
        h = host_handle(pattern_file(workdir, f"groups_random{seed}", pats), platform)
        try:
            g = h.groupsOpen(u64(masks))
            for flags in (0, ALL):
                for sm in (seg_masks, None):
                    want = ref.filter_lists(lists, m, sm, bool(flags))
                    st, got, total = host_groups(g, data.tobytes(), offsets, sm, flags)
                    assert st == 0 and total == want[0].size
                    ref.same(got, want, f"seed {seed}/{pname}/flags {flags}/masks {sm is not None}")
        finally:
            h.destroy()                                                                     # (with the table open)


@pytest.mark.parametrize("platform,pname", PLATFORMS)
def test_all_bits_everywhere_gives_the_lists_of_the_calls_without_groups(workdir, platform, pname):
    pats = ref.NESTED + [b"needle", b"nee", b"dle"]
    data = (b"b" + b"a" * 11 + b" needle nee " + b"a" * 5) * 40
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    offsets = np.array([0, 0, 7, 300, 301, 640, buf.size, buf.size], dtype=np.uintp)
    h = host_handle(pattern_file(workdir, "groups_identity", pats), platform)
    try:
        g = h.groupsOpen(np.full(len(pats) + 1, ref.ALL_BITS, dtype=np.uint64))
        for sm in (None, [ref.ALL_BITS] * (offsets.size - 1)):
            st, got, total = host_groups(g, data, offsets, sm, ALL)
            per = [h.match_all_host_array(buf[offsets[k]:offsets[k + 1]]) for k in range(offsets.size - 1)]
            want = (np.concatenate([p[0] + int(offsets[k]) for k, p in enumerate(per)]), np.concatenate([p[1] for p in per]))
            ref.same(got[:2], want, "ALL under all bits is the all-match list of every segment")
            assert got[2].tolist() == np.concatenate([[0], np.cumsum([p[0].size for p in per])]).tolist()
            full = np.full(buf.size, -7, dtype=np.int32)
            h.matchBatchFromHost(buf.ctypes.data, buf.size, offsets.ctypes.data, offsets.size - 1, full.ctypes.data)
            st, got, total = host_groups(g, data, offsets, sm, 0)
            ref.same(got[:2], (np.flatnonzero(full > 0), full[full > 0]), "flags 0 under all bits is the longest list of the batch")
        st, got, total = host_groups(g, data, None, None, 0)                               # one segment: the plain compacted call
        ids, pos = (np.full(buf.size, -7, dtype=np.int32) for _ in range(2))
        _, n = h.matchFromHostReduce(buf.ctypes.data, buf.size, ids.ctypes.data, pos.ctypes.data)
        ref.same(got[:2], (pos[:n], ids[:n]), "flags 0, one segment, all bits: the list of PFAC_matchFromHostReduce")
    finally:
        h.destroy()


def test_truncation_writes_the_first_capacity_pairs_and_keeps_segfirst_and_seggroups_complete(workdir):
    name, pats, masks, data, offsets, seg_masks, nocase = ref.CASES[9]                     # nested a, two segments, every other group
    h = host_handle(pattern_file(workdir, "groups_trunc", pats))
    try:
        g = h.groupsOpen(u64(masks))
        for flags in (0, ALL):
            want = ref.groups_ref(pats, masks, data, offsets, seg_masks, bool(flags))
            total = want[0].size
            assert total > 3
            for capacity in (0, 1, total - 1, total, total + 5):
                st, got, n = host_groups(g, data, offsets, seg_masks, flags, capacity)
                assert n == total and st == (TRUNCATED if capacity < total else 0)
                k = min(capacity, total)
                ref.same(got, (want[0][:k], want[1][:k], want[2], want[3]), f"flags {flags}/capacity {capacity}")
    finally:
        h.destroy()


def test_every_status_of_the_contract(workdir):
    pats = [b"foo", b"foobar"]
    h = host_handle(pattern_file(workdir, "groups_status", pats))
    empty = api.PFAC.createHostOnly()
    try:
        assert empty.groupsOpen(u64([0, 1, 2]), check=False).status == NOT_READY
        assert h.groupsOpen(u64([0, 1]), check=False).status == INVALID                    # numMasks < F + 1
        assert h._lib.PFACX_groupsOpen(h._h, None, 3, None) == INVALID
        assert h._lib.PFACX_groupsOpen(None, None, 3, None) == BAD_HANDLE
        assert h._lib.PFACX_groupsClose(None) == BAD_HANDLE
        g = h.groupsOpen(u64([0, 1, 2, 99, 99]))                                            # more masks than patterns: the rest is ignored
        buf = np.frombuffer(b"foobar foo", dtype=np.uint8).copy()
        off = np.array([0, 6, 10], dtype=np.uintp)
        ids, pos = (np.full(16, -7, dtype=np.int32) for _ in range(2))
        n, big = buf.size, 1 << 31
        args = dict(h_input=buf.ctypes.data, size=n, h_offsets=off.ctypes.data, num_segments=2, h_seg_masks=None, flags=0, h_ids=ids.ctypes.data,
                    h_pos=pos.ctypes.data, capacity=16, h_seg_first=None, h_seg_groups=None)

        def call(**changed):
            return g.match_host(**dict(args, **changed), check=False)

        assert call() == (0, 2)
        assert call(size=big)[0] == INVALID
        assert call(num_segments=big)[0] == INVALID
        assert call(flags=2)[0] == INVALID and call(flags=ALL | 4)[0] == INVALID
        assert call(h_input=None)[0] == INVALID
        assert call(h_ids=None)[0] == INVALID and call(h_pos=None)[0] == INVALID
        assert call(h_ids=None, h_pos=None, capacity=0) == (TRUNCATED, 2)                   # the count query
        assert call(h_offsets=None)[0] == INVALID                                           # offsets == NULL with numSegments != 1
        assert call(h_offsets=None, num_segments=1) == (0, 2)
        assert call(num_segments=0)[0] == INVALID                                           # numSegments == 0 with size > 0
        assert g._lib.PFACX_groupsMatchFromHost(g._g, buf.ctypes.data, n, off.ctypes.data, 2, None, 0, ids.ctypes.data, pos.ctypes.data, 16, None, None,
                                                None) == INVALID
        assert g._lib.PFACX_groupsMatchFromHost(None, buf.ctypes.data, n, off.ctypes.data, 2, None, 0, None, None, 0, None, None, None) == BAD_HANDLE
        for bad in ([1, 6, 10], [0, 7, 6], [0, 6, 9]):                                      # host offsets are validated
            assert call(h_offsets=np.array(bad, dtype=np.uintp).ctypes.data)[0] == INVALID
        # size == 0: success, 0 pairs, segFirst and segGroups zeroed where given
        first, hit = np.full(3, ref.ALL_BITS, dtype=np.uint64), np.full(2, ref.ALL_BITS, dtype=np.uint64)
        zero = np.zeros(3, dtype=np.uintp)
        assert call(size=0, h_offsets=zero.ctypes.data, h_seg_first=first.ctypes.data, h_seg_groups=hit.ctypes.data) == (0, 0)
        assert not first.any() and not hit.any()
        assert call(size=0, num_segments=0, h_offsets=None)[0] == INVALID                   # (offsets == NULL with numSegments != 1 comes first)
        assert call(size=0, num_segments=0) == (0, 0)
        # a device form on a host-only handle; opening on one has worked
        assert g.match_device(buf.ctypes.data, n, None, 1, None, 0, None, None, 0, None, None, check=False)[0] == NOT_EXIST
        assert g.pairs_device(ids.ctypes.data, pos.ctypes.data, 2, None, 1, None, 0, None, None, 0, None, None, check=False)[0] == NOT_EXIST
        assert g.pairs_device(ids.ctypes.data, pos.ctypes.data, big, None, 1, None, 0, None, None, 0, None, None, check=False)[0] == INVALID
        assert g.pairs_device(ids.ctypes.data, pos.ctypes.data, 8, None, 1, None, 0, ids.ctypes.data + 16, pos.ctypes.data, 4, None, None,
                              check=False)[0] == INVALID                                    # output over input
        # another pattern set: every match call is refused, close works
        h.readPatternFromFileEx(pattern_file(workdir, "groups_status2", [b"bar"]), 0)
        assert call()[0] == INVALID
        assert g.match_device(buf.ctypes.data, n, None, 1, None, 0, None, None, 0, None, None, check=False)[0] in (INVALID, NOT_EXIST)
        assert g.close(check=False) == 0
        assert h._lib.PFACX_groupsClose(g._g) == BAD_HANDLE
        g2 = h.groupsOpen(u64([0, 4]))
        st, total = g2.match_host(buf.ctypes.data, n, None, 1, None, 0, ids.ctypes.data, pos.ctypes.data, 16, None, None)
        assert (st, total) == (0, 1) and (int(ids[0]), int(pos[0])) == (1, 3)
    finally:
        empty.destroy()
        h.destroy()                                                                         # with g2 open: PFAC_destroy closes it
