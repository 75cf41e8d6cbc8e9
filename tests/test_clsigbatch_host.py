"""PFACX_clsigBatchMatchFromHost on the CPU platforms (host-only handles: no device needed) against two oracles that share nothing with it: the
models of tests/clsig_ref.py run on each segment's bytes alone and shifted (tests/clsigbatch_ref.py), and the library's own plain call per
segment.  The window-edge table at every segment start mod 4 with both end rules and the lists worked out by hand, one segment against the plain
call, runs of empty segments, offsets the host form refuses, every refusal, truncation with and without the end and segFirst arrays, the set of
the gapsig cross-check segment by segment, and the seeded random case with its two counts asserted.  Every comparison is exact."""

import numpy as np
import pytest

from pfac_amd import api
from tests import clsig_ref as ref
from tests import clsigbatch_ref as bref

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
INVALID, NOT_EXIST, TRUNCATED, BAD_HANDLE = (api.STATUS.INVALID_PARAMETER, api.STATUS.LIB_NOT_EXIST, api.STATUS.OUTPUT_TRUNCATED,
                                             api.STATUS.INVALID_HANDLE)
GUARD = 16
POISON64 = 2 ** 64 - 7


def host_handle(platform=api.PFAC_PLATFORM_CPU):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    return h


def host_batch(sg, data, offsets, capacity=None, with_end=True, with_first=True):
    """match_batch_host into poisoned arrays of `capacity` entries (default: the full length, asked for first) with GUARD poisoned entries on both
    sides of each, segFirst included -> (status, (pos, ids, end) written, segFirst, the full length); nothing else may change, nor the inputs"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    offs_before, n, segs = offs.copy(), buf.size, offs.size - 1
    if capacity is None:
        st, capacity = sg.match_batch_host(buf.ctypes.data, n, offs.ctypes.data, segs, None, None, None, 0, check=False)
        assert st in (0, TRUNCATED) and (st == TRUNCATED) == (capacity > 0)
    ids, pos, end = (np.full(GUARD + capacity + GUARD, -7, dtype=np.int32) for _ in range(3))
    first = np.full(GUARD + segs + 1 + GUARD, POISON64, dtype=np.uint64)
    st, total = sg.match_batch_host(buf.ctypes.data, n, offs.ctypes.data, segs, ids.ctypes.data + 4 * GUARD, pos.ctypes.data + 4 * GUARD,
                                    end.ctypes.data + 4 * GUARD if with_end else None, capacity,
                                    first.ctypes.data + 8 * GUARD if with_first else None, check=False)
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > capacity)
    k = min(total, capacity)
    for a in (ids, pos, end):
        assert np.all(a[:GUARD] == -7) and np.all(a[GUARD + capacity:] == -7), "wrote outside the arrays"
        assert np.all(a[GUARD + k:GUARD + capacity] == -7), "wrote behind the list"
    assert with_end or np.all(end == -7)
    assert np.all(first[:GUARD] == POISON64) and np.all(first[GUARD + segs + 1:] == POISON64), "wrote outside segFirst"
    assert with_first or np.all(first == POISON64)
    assert buf.tobytes() == bytes(data) and np.array_equal(offs, offs_before), "the caller's input or offsets were modified"
    return st, tuple(a[GUARD:GUARD + k].copy() for a in (pos, ids, end)), first[GUARD:GUARD + segs + 1].copy(), total


def plain_per_segment(sg, data, offsets):
    """the second oracle: the library's own plain host call on each segment's bytes alone, shifted"""
    raw, cols, first = bytes(data), [[], [], []], []
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        first.append(len(cols[0]))
        if hi > lo:
            pos, ids, end = sg.match_host_array(np.frombuffer(raw[int(lo):int(hi)], dtype=np.uint8))
            cols[0] += (pos + int(lo)).tolist()
            cols[1] += ids.tolist()
            cols[2] += (end + int(lo)).tolist()
    first.append(len(cols[0]))
    return tuple(np.array(c, dtype=np.int32) for c in cols), np.array(first, dtype=np.uint64)


# ---------------------------------------------------------------- 1. window edges


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("case", bref.EDGE_CASES, ids=[c[0] for c in bref.EDGE_CASES])
def test_window_edges_against_the_models_and_the_plain_call_per_segment(case, platform, pname):
    name, lines, cut, _, _ = case
    sigs = ref.parse_lines(lines)
    for flags in (0, bref.SHORTEST):
        h = host_handle(platform)
        try:
            with h.clsigOpenText(ref.text_of(lines), cut, flags) as sg:
                anchors = sg.anchors()
                for lead in (0, 1, 2, 3):
                    data, offsets = bref.edge_batch(case, lead)
                    want, want_first = bref.batch_model(sigs, data, offsets, anchors, flags, lines if lead == 0 else None)
                    st, got, first, total = host_batch(sg, data, offsets)
                    assert st == 0 and total == want[0].size
                    ref.same(got, want, f"{name}/flags {flags}/lead {lead}: against the models per segment")
                    assert first.tolist() == want_first.tolist()
                    own, own_first = plain_per_segment(sg, data, offsets)
                    ref.same(got, own, f"{name}/flags {flags}/lead {lead}: against the plain call per segment")
                    assert first.tolist() == own_first.tolist()
                    by_hand = bref.edge_want(case, flags, lead)
                    assert by_hand is None or bref.triples(got) == by_hand, f"{name}/flags {flags}/lead {lead}: against the list worked out by hand"
        finally:
            h.destroy()


def test_the_flat_call_differs_on_every_edge_case():
    """what the feature is for: without segments, the same bytes give another list"""
    for case in bref.EDGE_CASES:
        name, lines, cut, _, _ = case
        h = host_handle()
        try:
            with h.clsigOpenText(ref.text_of(lines), cut, 0) as sg:
                data, offsets = bref.edge_batch(case)
                _, got, _, _ = host_batch(sg, data, offsets)
                assert bref.triples(sg.match_host_array(data)) != bref.triples(got), name
        finally:
            h.destroy()


# ---------------------------------------------------------------- 2. empty segments and segFirst


def test_runs_of_empty_segments_at_the_front_in_the_middle_and_at_the_end():
    data = b"a" * 40
    offsets = [0] * 5 + [7] + [19] * 4 + [20, 22] + [40] * 6
    h = host_handle()
    try:
        with h.clsigOpenText(ref.text_of(bref.RUN_LINES)) as sg:
            want, want_first = bref.run_want(offsets)
            st, got, first, total = host_batch(sg, data, offsets)
            assert st == 0
            ref.same(got, want, "empty segments")
            assert first.tolist() == want_first.tolist()
    finally:
        h.destroy()


# ---------------------------------------------------------------- 3. offsets the host form refuses


@pytest.mark.parametrize("what,make", bref.HOSTILE, ids=[w for w, _ in bref.HOSTILE])
def test_the_host_form_refuses_offsets_a_device_form_clamps(what, make):
    data = np.frombuffer(b"k=12 k=345 k=6789 k=1", dtype=np.uint8).copy()
    h = host_handle()
    try:
        with h.clsigOpenText(b"k=[0-9]{1,5}\n") as sg:
            offs = np.array(make(data.size), dtype=np.uint64)
            out = np.full(64, -7, dtype=np.int32)
            first = np.full(offs.size, POISON64, dtype=np.uint64)
            st, _ = sg.match_batch_host(data.ctypes.data, data.size, offs.ctypes.data, offs.size - 1, out.ctypes.data, out.ctypes.data, None, 8,
                                        first.ctypes.data, check=False)
            assert st == INVALID and np.all(out == -7) and np.all(first == POISON64)
    finally:
        h.destroy()


# ---------------------------------------------------------------- 4. equalities, capacity, refusals


@pytest.mark.parametrize("flags", [0, bref.SHORTEST])
def test_one_segment_is_the_plain_call(flags):
    for name, lines, data, cut, _ in ref.CASES:
        h = host_handle()
        try:
            with h.clsigOpenText(ref.text_of(lines), cut, flags) as sg:
                st, got, first, total = host_batch(sg, data, [0, len(data)])
                ref.same(got, sg.match_host_array(np.frombuffer(data, dtype=np.uint8)), name)
                assert first.tolist() == [0, total]
        finally:
            h.destroy()


def test_the_gapsig_cross_check_segment_by_segment():
    """full classes (??), nibble classes (5?, ?A) and gaps through PFACX_gapsig* on each segment alone: (id, start, end) equal as sets with
    SHORTEST_END, which is the gapsig meaning of the end"""
    from tests import gapsig_ref
    gap_lines = ["4D 5A {2-6} 50 45 00", "E8 ?? ?? [0-8] 5? C3", "61 62 {0-3} ?A 63 64 {1-2} 65"]
    cls_lines = ["MZ.{2,6}PE\\x00", "\\xe8.{2}.{0,8}[P-_]\\xc3", "ab.{0,3}[\\x0a\\x1a*:JZjz\\x8a\\x9a\\xaa\\xba\\xca\\xda\\xea\\xfa]cd.{1,2}e"]
    data = np.random.default_rng(11).integers(0, 256, 3000, dtype=np.uint8)
    gapsig_ref.embed(gapsig_ref.parse_lines(gap_lines), data, 5, per_sig=6)
    cuts = np.sort(np.random.default_rng(12).choice(np.arange(1, 3000), size=150, replace=False))
    offsets = np.concatenate([[0], cuts, [3000]])
    h = host_handle()
    try:
        per_segment = []
        with h.gapsigOpenText(gapsig_ref.text_of(gap_lines)) as gs:
            whole = gs.match_host_array(data)
            for lo, hi in zip(offsets[:-1], offsets[1:]):
                pos, ids, end = gs.match_host_array(data[lo:hi])
                per_segment += zip(ids.tolist(), (pos + lo).tolist(), (end + lo).tolist())
        with h.clsigOpenText(ref.text_of(cls_lines), 0, ref.SHORTEST) as sg:
            _, got, _, _ = host_batch(sg, data, offsets)
        assert bref.triples(got) == sorted(per_segment)
        assert 6 <= len(per_segment) < whole[0].size, "some instances are cut, some are left"
    finally:
        h.destroy()


def test_truncation_with_and_without_the_end_and_seg_first_arrays():
    case = next(c for c in bref.EDGE_CASES if c[0] == "full-boundary-classes")
    data, offsets = bref.edge_batch(case, 1)
    h = host_handle()
    try:
        with h.clsigOpenText(ref.text_of(case[1])) as sg:
            _, want, want_first, total = host_batch(sg, data, offsets)
            assert total == 6 and want_first[-1] == 6
            for cap in (0, 1, total - 1, total, total + 2):
                for with_end in (True, False):
                    for with_first in (True, False):
                        st, got, first, full = host_batch(sg, data, offsets, cap, with_end, with_first)
                        assert (st, full) == (TRUNCATED if cap < total else 0, total)
                        ref.same(got[:2], tuple(w[:cap] for w in want[:2]), f"capacity {cap}")
                        assert not with_end or got[2].tolist() == want[2][:cap].tolist()
                        assert not with_first or first.tolist() == want_first.tolist(), "segFirst names entries past capacity too"
    finally:
        h.destroy()


def test_every_refusal_of_the_host_form_and_the_device_forms_on_a_host_only_handle():
    h = host_handle()
    buf = np.frombuffer(b"ab12cd", dtype=np.uint8).copy()
    out = np.zeros(8, dtype=np.int32)
    offs = np.array([0, 3, 6], dtype=np.uint64)
    try:
        sg = h.clsigOpenText(b"ab[0-9]{0,3}cd\n")
        args = (out.ctypes.data, out.ctypes.data, out.ctypes.data)
        o = offs.ctypes.data
        assert sg.match_batch_host(buf.ctypes.data, 6, o, 2, None, None, None, 0) == (0, 0), "the signature crosses the cut"
        assert sg.match_batch_host(buf.ctypes.data, 6, o + 8, 1, None, None, None, 0, check=False)[0] == INVALID, "offsets[0] != 0"
        assert sg.match_batch_host(buf.ctypes.data, 0, o, 2, None, None, None, 0) == (0, 0), "size 0: nothing is looked at"
        assert sg.match_batch_host(buf.ctypes.data, 0, o, 0, None, None, None, 0) == (0, 0), "size 0 with no segment"
        assert sg.match_batch_host(buf.ctypes.data, 6, o, 0, None, None, None, 0, check=False)[0] == INVALID, "no segment for six bytes"
        assert sg.match_batch_host(buf.ctypes.data, 6, None, 2, None, None, None, 0, check=False)[0] == INVALID, "null offsets"
        assert sg.match_batch_host(buf.ctypes.data, 6, o, 2 ** 31 - 1, None, None, None, 0, check=False)[0] == INVALID
        assert sg.match_batch_host(None, 6, o, 2, *args, 8, check=False)[0] == INVALID
        assert sg.match_batch_host(buf.ctypes.data, 1 << 31, o, 2, *args, 8, check=False)[0] == INVALID
        assert sg.match_batch_host(buf.ctypes.data, 6, o, 2, None, None, None, 1, check=False)[0] == INVALID, "capacity without arrays"
        one = np.array([0, 6], dtype=np.uint64)
        assert sg.match_batch_host(buf.ctypes.data, 6, one.ctypes.data, 1, None, None, None, 0, check=False) == (TRUNCATED, 1)
        assert sg.match_batch_device(buf.ctypes.data, 6, o, 2, *args, 8, check=False)[0] == NOT_EXIST
        assert sg.batch_pairs_device(buf.ctypes.data, 6, o, 2, out.ctypes.data, out.ctypes.data, 1, None, None, None, 0, check=False)[0] == NOT_EXIST
        assert sg.match_batch_device(buf.ctypes.data, 6, None, 2, *args, 8, check=False)[0] == INVALID
        assert sg.match_batch_device(buf.ctypes.data, 6, o, 0, *args, 8, check=False)[0] == INVALID
        assert sg.match_batch_device(buf.ctypes.data, 6, o, 2, *args, 5, check=False)[0] == INVALID, "the device form needs capacity >= size"
        assert sg.batch_pairs_device(buf.ctypes.data, 6, o, 2 ** 31 - 1, out.ctypes.data, out.ctypes.data, 1, None, None, None, 0, check=False)[0] == INVALID
        assert sg.batch_pairs_device(buf.ctypes.data, 6, o, 2, out.ctypes.data, out.ctypes.data, 2 ** 31, None, None, None, 0, check=False)[0] == INVALID
        assert sg.batch_pairs_device(buf.ctypes.data, 6, o, 2, out.ctypes.data, out.ctypes.data, 4, out.ctypes.data + 8, out.ctypes.data + 16, None, 4,
                                     check=False)[0] == INVALID, "output arrays that overlap the pair arrays"
        null = (None, buf.ctypes.data, 6, o, 2, None, None, None, 0, None, None)
        assert sg._lib.PFACX_clsigBatchMatchFromHost(*null) == BAD_HANDLE and sg._lib.PFACX_clsigBatchMatchFromDevice(*null) == BAD_HANDLE
        assert sg._lib.PFACX_clsigBatchMatchFromHost(sg._c, buf.ctypes.data, 6, o, 2, None, None, None, 0, None, None) == INVALID, "no place for the length"
        h.readPatternFromMemory(b"other\n")                       # the object goes stale
        assert sg.match_batch_host(buf.ctypes.data, 6, o, 2, None, None, None, 0, check=False)[0] == INVALID
        assert sg.close() == 0
    finally:
        h.destroy()


# ---------------------------------------------------------------- 5. the seeded random case


def test_200_random_signatures_over_64_kib_cut_at_seeded_offsets():
    sigs, data, offsets = bref.random_batch()
    h = host_handle(api.PFAC_PLATFORM_CPU_OMP)
    try:
        with h.clsigOpen(*ref.csr_of(sigs)) as sg:
            anchors = sg.anchors()
            flat, _ = ref.fast_list(sigs, data, anchors)
            want, want_first = bref.batch_model(sigs, data, offsets, anchors, fast=True)
            lost, freed = bref.crossing_figures(flat, want)
            print({"segments": offsets.size - 1, "flat": int(flat[0].size), "batch": int(want[0].size), "lost": lost, "freed": freed})
            assert lost >= 20, "crossings: entries of the flat list that the batch list must not have"
            assert freed >= 5, "boundary classes freed by a segment edge: entries the flat list cannot have"
            st, got, first, total = host_batch(sg, data, offsets)
            assert st == 0
            ref.same(got, want, "the random case, cut")
            assert first.tolist() == want_first.tolist()
            ref.same(sg.match_host_array(data), flat, "the flat call is what it was")
            assert bref.triples(flat) != bref.triples(got)
    finally:
        h.destroy()
