"""The cases of tests/batch_edges.py sit where their names say (group width, trip, grid pass, pair index, block count), their expected vectors
are what the brute force and the oracle give on every segment alone, and PFACX_matchBatchFromHost on the CPU platforms returns them.  No
device needed."""
import os
import re

import numpy as np
import pytest

from pfac_amd import api
from tests import batch_edges as be
from tests.nocase_ref import fold, fold_array, write_patterns
from tests.segcount_ref import brute_seg_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]


def small_tables():
    return be.full_tables() + [t for t in be.pair_tables() if t.name != "many-blocks"]


def large_tables():
    return [be.pair_case("many-blocks"), be.grid_pass(256)]


def always_sampled(case):
    """the segments of a large table that the sample must hold: those around its drops"""
    if case.name != "many-blocks":
        return ()
    whole = np.flatnonzero(brute_seg_result(be.DROP, case.data.tobytes(), [0, case.data.size]))
    return [be.segment_of(case, int(whole[i])) + d for i in be.MANY_DROPS for d in (-1, 0, 1)]


def test_constants_name_the_kernels_constants():
    assert (api.PFACX_BATCH_BLOCK, api.PFACX_BATCH_SEGS_PER_TRIP, api.PFACX_BATCH_MAX_GROUP_LOG2) == (256, 8, 6)
    src = open(os.path.join(ROOT, "pfac_amd", "csrc", "scan_batch.hip")).read()
    assert int(re.search(r"constexpr int kBatchBlock = (\d+);", src).group(1)) == api.PFACX_BATCH_BLOCK
    assert int(re.search(r"constexpr int kSegsPerTrip = (\d+);", src).group(1)) == api.PFACX_BATCH_SEGS_PER_TRIP
    assert int(re.search(r"while \(groupLog2 < (\d+) &&", src).group(1)) == api.PFACX_BATCH_MAX_GROUP_LOG2
    assert f"gridCap(c, {be.GRID_PER_CU})" in src and f"dim3({be.SCAN_BLOCKS})" in src


def test_the_model_of_the_group_width():
    assert [be.group_log2(n * 100, 100, 70) for n in (0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 68, 69, 5000)] == [0, 0, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 6, 6, 6]
    assert be.group_log2(1000, 10, 4) == 2 and be.group_log2(1000, 10, 2) == 0          # the zone, where it is shorter than the mean segment
    assert be.segments_per_pass(256, 6) == 256 * 16 * 4 * 8 and be.segments_per_pass(64, 0) == 64 * 16 * 256 * 8


def test_width_tables_reach_their_group_width_with_every_special_length():
    for log2 in range(7):
        case = be.width_case(log2)
        assert be.case_group_log2(case) == log2, case.name
        lens = set(be.segment_lengths(case).tolist())
        walk = be.MAX_WALK["arun"]
        assert walk == 69 and {0, 1, walk - 1, walk, walk + 1}.issubset(lens), case.name
        assert any(n < (1 << log2) for n in lens) and any(2.9 * walk <= n <= 3.1 * walk for n in lens), case.name
        assert case.data.size < (16 << 10)
        want = be.reference(case)
        assert np.all(want[case.data == ord("a")] != 0), "every `a` matches"
        ends = case.offsets[1:][be.segment_lengths(case) > 0].astype(np.int64)
        assert np.all(want[ends - 1] == (case.data[ends - 1] == ord("a"))), "the last position of a segment holds the 1-byte pattern"
    long_zone = be.width6_long_zone()
    assert be.case_group_log2(long_zone) == 6 and be.MAX_WALK["longzone"] > 64
    lens = be.segment_lengths(long_zone)
    assert np.all(lens > 3 * 64) and min(lens.min(), be.MAX_WALK["longzone"]) // 64 >= 3, "three strides of a 64-lane group and more"
    want = be.reference(long_zone)
    assert np.count_nonzero(want > len(be.ARUN)) >= 6 and np.count_nonzero((want > 0) & (want <= len(be.ARUN))) > 800


def test_trip_tables_cover_1_to_17_segments():
    for n in range(1, 18):
        case = be.trip_case(n)
        assert len(case.offsets) - 1 == n and be.case_group_log2(case) in (2, 3), case.name
        lens = be.segment_lengths(case)
        assert lens.min() >= 5 and lens.max() <= 9 and np.all(case.data == ord("a"))
    lens = be.segment_lengths(be.empties()).tolist()
    assert lens[0] == 0 and lens[-1] == 0 and [0] * 9 == lens[3:12] and lens[11:15] == [0, 12, 0, 12]
    assert be.SEGS_PER_TRIP == 8


def test_long_slot_cuts_report_the_longest_prefix_that_fits():
    case = be.long_slots()
    want = be.reference(case)
    _, marks = be.long_slots_marks()
    assert sorted(j for _, j in marks) == sorted(2 * list(range(201)))
    for i, (at, j) in enumerate(marks):
        whole_behind = i < 201 and j == 0         # cut after 0 bytes with the rest behind the cut: all of P at the head of the next segment
        assert want[at] == (len(be.NESTED) if whole_behind else be.longest_prefix_id(j)), (at, j)
        if j:
            assert case.data[at] == ord("Z") and be.segment_of(case, at) == be.segment_of(case, at + j - 1) != be.segment_of(case, at + j)
    assert np.count_nonzero(want) == sum(1 for _, j in marks if j >= 2) + sum(1 for _, j in marks[:201] if j == 0), "P's first byte starts every match"
    assert be.P.count(be.P[:1]) == 1 and len(be.P) == 200 and be.P[:1].lower() not in be.P[1:]
    assert len(be.NOCASE_CUTS) == 50 and be.nocase_case().nocase


def test_pair_tables_hold_the_counts_and_drops_they_claim():
    for case in be.pair_tables():
        count, drops = be.CLAIMED[case.name]
        whole = brute_seg_result(be.DROP, case.data.tobytes(), [0, case.data.size])
        pairs = np.flatnonzero(whole)
        assert pairs.size == count, case.name
        dropped = np.flatnonzero(be.reference(case)[pairs] == 0)
        assert dropped.tolist() == drops, case.name
        assert np.array_equal(be.reference(case)[pairs] != 0, whole[pairs] == 3), case.name
    assert be.CLAIMED["pairs-513"][1] == [0, 63, 64, 255, 256, 512] and be.CLAIMED["pairs-64"][1] == [0, 63] and be.CLAIMED["pairs-1"][1] == [0]
    many = be.pair_case("many-blocks")
    blocks = (be.CLAIMED["many-blocks"][0] + be.BLOCK - 1) // be.BLOCK
    assert blocks > be.SCAN_BLOCKS and be.MANY_DROPS[0] < be.BLOCK and be.MANY_DROPS[1] // be.BLOCK >= 1025 and many.data.size < (1 << 20)
    on = be.pair_case("pair-on-offset")
    at = set(np.flatnonzero(be.reference(on)).tolist())
    assert len(at & set(on.offsets.astype(np.int64).tolist())) == 40 and np.count_nonzero(be.segment_lengths(on) == 0) >= 5
    assert len(be.pair_case("no-pairs").offsets) - 1 == 20


@pytest.mark.parametrize("cus", [256, 64])
def test_grid_pass_exceeds_one_pass_of_the_grid(cus):
    case = be.grid_pass(cus)
    nseg = len(case.offsets) - 1
    assert be.case_group_log2(case) == 6
    assert nseg == be.segments_per_pass(cus, 6) + 9 > be.segments_per_pass(cus, 6) and np.all(be.segment_lengths(case) == 70)
    whole = brute_seg_result(be.SETS["grid"], case.data[:70 * 300].tobytes(), [0, 70 * 300])
    assert np.count_nonzero(whole == 1) >= 290, "the scan over the concatenation reports the 70-byte pattern across the segment ends"
    segments = be.sample_segments(case, 220)
    assert segments.size >= 200 and nseg - 1 in segments and be.segments_per_pass(cus, 6) in segments
    for k, want in be.brute_on_segments(case, segments):
        assert np.array_equal(be.reference(case)[70 * k:70 * k + 70], want), k


def test_constructed_vectors_equal_the_brute_force():
    for case in be.pair_tables():
        if case.name == "many-blocks":
            segments = be.sample_segments(case, 240, always=always_sampled(case))
            assert segments.size >= 200
            for k, want in be.brute_on_segments(case, segments):
                assert np.array_equal(be.reference(case)[int(case.offsets[k]):int(case.offsets[k + 1])], want), k
        else:
            assert np.array_equal(be.reference(case), brute_seg_result(be.DROP, case.data.tobytes(), case.offsets)), case.name


def _oracle(case, workdir):
    from oracle import binding as ob
    pats = be.SETS[case.set]
    if case.nocase:                               # the definition of a caseless set: the folded set over the folded input
        return ob.Oracle(write_patterns(os.path.join(workdir, "batch_edges_folded.pat"), [fold(p) for p in pats]), hashed=False)
    return ob.Oracle(be.pattern_file(case.set), hashed=False)


def test_oracle_on_every_segment_equals_the_reference(workdir):
    for case in small_tables() + large_tables():
        o = _oracle(case, workdir)
        data = fold_array(case.data) if case.nocase else case.data
        want = be.reference(case)
        segments = be.sample_segments(case, 240, always=always_sampled(case))
        assert segments.size >= min(200, len(case.offsets) - 1)
        try:
            for k in segments:
                s, e = int(case.offsets[k]), int(case.offsets[k + 1])
                if e > s:
                    assert np.array_equal(o.match(np.ascontiguousarray(data[s:e])), want[s:e]), f"{case.name}: segment {k}"
        finally:
            o.close()


def _handle(case, platform):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    if case.nocase:
        h.readPatternFromFileEx(be.pattern_file(case.set), api.PFACX_READ_NOCASE)
    else:
        h.readPatternFromFile(be.pattern_file(case.set))
    return h


@pytest.mark.parametrize("platform,pname", PLATFORMS)
def test_batch_from_host_on_the_cpu_platforms_equals_the_reference(monkeypatch, platform, pname):
    monkeypatch.setenv("OMP_NUM_THREADS", "4")
    for case in small_tables() + large_tables():
        h = _handle(case, platform)
        try:
            got = h.match_batch_host_array(case.data, case.offsets)
        finally:
            h.destroy()
        want = be.reference(case)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{case.name}/{pname}: {bad.size} mismatches, first at {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"
