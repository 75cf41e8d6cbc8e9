"""The fixtures of tests/test_filter_edges_gpu.py (tests/filter_edges.py), checked without a device: the constants of the model against the
defaults in the kernel's sources, the model of the launch plan for every size the GPU file uses, the level-1 hit counts that put a chunk on
either side of the kernel's buffer sizes and of its dense threshold, which filter instance each pattern set gets, and that the oracle finds what
was planted.

The three sets that the cases were planned around -- "qq", "long", "q" -- all carry a tail table in LDS (the VETO = 1 instance); the set without
one, which gets the plain window walker, is "min3", the set of 3-byte patterns that case A needs for the smallest margin anyway."""
import os
import re

import numpy as np
import pytest

from tests import filter_edges as fe
from tests import tiled_edges as te
from tests.filter_model import level1_model, reduce_filter_model, tail_entries

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pfac_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.mark.parametrize("name", sorted(fe.SOURCES))
def test_model_constants_are_the_defaults_in_the_sources(name):
    """a retune of the kernel fails here: the sizes of the GPU file are derived from these constants and would otherwise quietly stop
    meeting the kernel's edges"""
    path, pattern = fe.SOURCES[name]
    found = re.findall(pattern, _source(path))
    assert len(found) == 1, f"{name}: {len(found)} definitions match in {path}"
    assert int(found[0]) == getattr(fe, name), f"{name}: {path} says {found[0]}, tests/filter_edges.py {getattr(fe, name)}"


def test_model_restates_the_launchers_arithmetic():
    """the expressions plan() restates, as they stand in the sources"""
    module, kernel, common = _source("scan_module.hip"), _source("scan_filter.hip"), _source("scan_common.h")
    for text, where in (("const size_t margin = (size_t)c->fa.maxPatternLen + 64 + kWalkHalo;", module),
                        ("return end > first ? (end - first) / kChunkBytesHost * kChunkBytesHost : 0;", module),
                        ("const size_t head = (16u - (reinterpret_cast<uintptr_t>(in) & 15u)) & 15u;", module),
                        ("constexpr size_t kChunkBytesHost = (size_t)pfac::kChunkTiles * 1024;", common),
                        ("constexpr size_t kLdsPerCu = 160 * 1024;", common),
                        ("constexpr int kWavesPerBlock = kBlockThreads / 64;", common),
                        ("static constexpr int kWriters = REDUCE ? 0 : PFAC_WRITERS;", kernel),
                        ("static constexpr int kScanners = kWavesPerBlock - kWriters;", kernel),
                        ("size_t blocks = (numChunks + scanners - 1) / scanners;", kernel),
                        ("const uint32_t parts = gridDim.x < kParts ? gridDim.x : kParts;", kernel),
                        ("constexpr uint32_t kTicketBatch = kWriters ? 1u : (kFrontOn ? (1u << kFront) : 1u);", kernel),
                        ("const bool dense = !REDUCE && freshChunk && total > kDenseHits && a.denseList != nullptr;", kernel)):
        assert text in where, text
    assert (fe.CHUNK, fe.kSpanChunks, fe.GRANULE, fe.BATCH, fe.SCANNERS_FULL, fe.SCANNERS_REDUCE) == (2048, 4, 64, 16, 13, 16)
    assert fe.margin(600) == 792 and fe.margin(3) == 195
    # by hand: a pointer 5 bytes behind a 16-byte address: 11 positions in front of the first aligned byte
    assert fe.plan(5, 11 + 2048 + 792, 600, False) == (11, 2048, 1, 1, 1)
    assert fe.plan(5, 11 + 2048 + 792 - 1, 600, False) == (11, 0, 0, 0, 0)
    assert fe.plan(0, 14 * 2048 + 792 + 2047, 600, False) == (0, 14 * 2048, 14, 2, 2)
    assert fe.plan(0, 17 * 2048 + 195, 3, True) == (0, 17 * 2048, 17, 2, 2)
    assert fe.plan(15, 7, 600, False) == (1, 0, 0, 0, 0) and fe.plan(0, 3, 3, True)[2] == 0
    assert fe.plan(0, 2048 * 5000 + 792, 600, False)[3:] == (fe.RESIDENT, 2)


def test_pattern_sets_and_the_instance_each_gets():
    """HAS_SHORT: the set has patterns of one or two bytes.  VETO = 1: it has a tail table in LDS (launchChained: every walker but the forced stage
    walker); without one the register-window walker runs plain."""
    assert fe.SETS["long"] == [p for p in te.SETS["qq"] if len(p) >= 3] and len(fe.SETS["long"]) == len(te.SETS["qq"]) - 2
    assert all(len(p) == 3 for p in fe.MIN3) and len(set(fe.MIN3)) == len(fe.MIN3)
    assert fe.MAX_LEN == {"q": 600, "qq": 600, "long": 600, "min3": 3}
    shape = {}
    for name, pats in fe.SETS.items():
        h = fe.host_handle(name)
        info = h.info()
        assert info.numOfPatterns == len(pats) and info.maxPatternLen == fe.MAX_LEN[name] and info.filterTailGlobalEntries == 0
        assert len(tail_entries(h)) == info.filterTailEntries
        shape[name] = (bool(info.filterHasShort), info.filterTailEntries > 0)
    assert shape == {"q": (True, True), "qq": (True, True), "long": (False, True), "min3": (False, False)}
    assert open(fe.pattern_file("qq"), "rb").read() == open(te.pattern_file("qq"), "rb").read()
    assert fe.WALK_PATTERN in fe.SETS["qq"] and fe.WALK_PATTERN in fe.SETS["long"] and len(fe.WALK_PATTERN) == 5
    assert all(p in fe.SETS[name] for p in fe._HANDOUT for name in ("q", "qq", "long"))


def test_fillers():
    """The quiet filler passes neither kernel's level 1 anywhere under "qq", "long" and "min3".  tiled_edges' `0123` passes nowhere under "long" and
    "min3"; under "qq" the full-result kernel's level 1 lets `11` + another byte through (a collision in the bitmap) and nothing else: sparse.
    A chunk of `q` is dense under "qq"; every chunk is dense under "q"."""
    rng = np.random.Generator(np.random.PCG64(1))
    quiet, filler = fe._quiet(rng, 64 * 1024), te._filler(rng, 64 * 1024)
    for name in ("qq", "long", "min3"):
        h = fe.host_handle(name)
        assert not level1_model(h, quiet).any() and not reduce_filter_model(h, quiet)[0].any(), name
        assert not reduce_filter_model(h, filler)[0].any(), name
    for name in ("long", "min3"):
        assert not level1_model(fe.host_handle(name), filler).any(), name
    hits = level1_model(fe.host_handle("qq"), filler)[:-2]
    ones = (filler[:-2] == ord("1")) & (filler[1:-1] == ord("1")) & (filler[2:] != ord("1"))
    assert np.array_equal(hits, ones) and 0 < hits.sum() * 16 < hits.size
    per_chunk = hits[:31 * fe.CHUNK].reshape(-1, fe.CHUNK).sum(axis=1)
    assert per_chunk.max() < fe.PFAC_DENSE_HITS // 4
    run = np.concatenate([np.full(fe.CHUNK, fe.Q, dtype=np.uint8), quiet[:8]])
    assert level1_model(fe.host_handle("qq"), run)[:fe.CHUNK].sum() == fe.CHUNK - 1 > fe.PFAC_DENSE_HITS
    for in_off in fe.IN_OFFS:
        for chunks in fe.DENSE_SET_CHUNKS:
            per_chunk = fe.chunk_hits(fe.host_handle("q"), 600, fe.handout(in_off, chunks), in_off, False)
            assert per_chunk.size == chunks and per_chunk.min() > fe.PFAC_DENSE_HITS, (in_off, chunks, per_chunk.min())
            assert fe.stats_of("q", fe.handout(in_off, chunks), in_off, False) == (0, chunks)
    assert set(fe.DENSE_SET_CHUNKS) <= set(fe.FULL_CHUNKS)


# blocks and parts of the hand-out's sizes, by hand: ceil(chunks / 13) blocks of the full-result kernel, ceil(chunks / 16) of the compacted-output one
FULL_PLAN = {1: (1, 1), 2: (1, 1), 3: (1, 1), 4: (1, 1), 5: (1, 1), 12: (1, 1), 13: (1, 1), 14: (2, 2), 26: (2, 2), 27: (3, 2), 63: (5, 2), 64: (5, 2),
             65: (5, 2), 68: (6, 2), 69: (6, 2), 127: (10, 2), 129: (10, 2), 193: (15, 2)}
REDUCE_PLAN = {1: (1, 1), 15: (1, 1), 16: (1, 1), 17: (2, 2), 32: (2, 2), 33: (3, 3), 511: (32, 32), 512: (32, 32), 513: (33, 32), 528: (33, 32), 529: (34, 32)}


def test_plan_of_every_size_the_gpu_file_uses():
    assert fe.FULL_CHUNKS == tuple(sorted(FULL_PLAN)) and fe.REDUCE_CHUNKS == tuple(sorted(REDUCE_PLAN))
    for in_off in fe.IN_OFFS:
        head = fe.head16(in_off)
        for reduce, table in ((False, FULL_PLAN), (True, REDUCE_PLAN)):
            for chunks, (blocks, parts) in table.items():
                n = fe.handout(in_off, chunks).size
                assert fe.plan(in_off, n, 600, reduce) == (head, fe.CHUNK * chunks, chunks, blocks, parts), (in_off, chunks, reduce)
    for name in fe.A_SETS:                                             # A: k chunks, k - 1 for d = -1, whichever kernel
        for in_off in range(16):
            for k in fe.A_K:
                for d in fe.A_D:
                    n = fe.size_for(in_off, k, fe.MAX_LEN[name], d)
                    for reduce in (False, True):
                        head, main_len, chunks, blocks, parts = fe.plan(in_off, n, fe.MAX_LEN[name], reduce)
                        assert (head, chunks, blocks, parts) == ((16 - in_off) % 16, k - (d < 0), min(1, k - (d < 0)), min(1, k - (d < 0)))
                        assert n - (head + main_len) == fe.margin(fe.MAX_LEN[name]) + (d if d >= 0 else fe.CHUNK - 1)      # the tail
    assert fe.A_D == (-1, 0, 1, 1024, 2047)
    # parts = min(gridDim, kParts) loses nothing because a launch has a block for every part that owns a piece: ceil(chunks / scanners) blocks, and a
    # granule holds more chunks than a block has scanners (with parts FIXED at kParts the kernel computes the same: a part without a block owns no piece)
    assert fe.SCANNERS_FULL <= fe.GRANULE and fe.SCANNERS_REDUCE <= fe.BATCH
    for chunks in range(1, 3 * fe.GRANULE * fe.PFAC_REDUCE_PARTS):
        for reduce, granule, most in ((False, fe.GRANULE, fe.PFAC_WORK_PARTS), (True, fe.BATCH, fe.PFAC_REDUCE_PARTS)):
            assert fe.plan(0, fe.size_for(0, chunks, 600), 600, reduce)[4] >= min(-(-chunks // granule), most)
    for case, (chunks, _, _) in fe.DENSE_CASES.items():
        for in_off in fe.IN_OFFS:
            assert fe.plan(in_off, fe.dense_case(in_off, case).size, 600, False)[2] == chunks
    for data, _ in (fe.hit_chunks("qq"), fe.hit_chunks("long"), fe.hit_chunks("qq", True), fe.walk_chunks()):
        assert fe.plan(0, data.size, 600, False)[2] == fe.plan(0, data.size, 600, True)[2] == (data.size - 792) // fe.CHUNK >= 15
    assert fe.plan(0, fe.WALKS_N, 600, False)[2:] == (113, 9, 2) and fe.WALKS_N < 240 * 1024


@pytest.mark.parametrize("in_off", [0, 1, 9, 15])
def test_seam_inputs(in_off):
    """what case A plants lies where its docstring says, and the oracle reports it on exactly these bytes"""
    long_a, p600, lb40 = te.pattern_id(te.LONG_A), te.pattern_id(te.P600), te.pattern_id(te.LONG_B[:40])
    head = fe.head16(in_off)
    for k in fe.A_K:
        for d in fe.A_D:
            main_end = head + fe.CHUNK * (k - (d < 0 and k > 1))
            for v in range(fe.A_VARIANTS):
                data = fe.seam("qq", in_off, k, d, v)
                n = data.size
                assert n == head + fe.CHUNK * k + 792 + d
                want = fe.want(data, "qq")
                if v < 3:
                    assert want[main_end - (1, 0, 60)[v]] == long_a
                else:
                    assert want[main_end - 450] == p600 and main_end - 450 >= head
                assert want[(0, max(head - 1, 0), head, 0)[v]] == lb40
                assert want[n - 600] == p600 and want[n - 30] == 0
                whole = np.concatenate([data, np.frombuffer(b"ABCDEFGH", dtype=np.uint8)])
                assert fe.want(whole, "qq")[n - 30] == te.pattern_id(te.TAIL_CUT)
                assert np.count_nonzero(want[main_end + fe.SEAM_CLEAR:n - 600]) >= (d > 600)          # matches among the bounded walks
                small = fe.seam("min3", in_off, k, d, v)
                m = small.size
                want3 = fe.want(small, "min3")
                assert m == head + fe.CHUNK * k + 195 + d and want3[m - 3] == 3 and want3[m - 2] == 0
                whole = np.concatenate([small, np.frombuffer(b"A", dtype=np.uint8)])
                assert fe.want(whole, "min3")[m - 2] == 4
                assert np.count_nonzero(want3) > 10 and np.count_nonzero(fe.want(fe.seam("long", in_off, k, d, v), "long")) > 10


def test_handout_inputs():
    for in_off in fe.IN_OFFS:
        for chunks in (1, fe.GRANULE + 1, 2 * fe.GRANULE + 1):
            data = fe.handout(in_off, chunks)
            plants = fe.handout_plants(in_off, chunks)
            head = fe.head16(in_off)
            assert len(plants) == chunks and all(head + fe.CHUNK * c <= at < head + fe.CHUNK * (c + 1) - 40 for c, (at, _) in enumerate(plants))
            assert len({at % fe.CHUNK for at, _ in plants}) == len(plants) or chunks > 64
            for name in ("qq", "long"):
                want = fe.want(data, name)
                assert all(want[at] == fe.SETS[name].index(p) + 1 for at, p in plants)
                assert want[data.size - 300] == fe.SETS[name].index(te.LONG_B) + 1
                level1, dense = fe.stats_of(name, data, in_off, False)
                assert dense == 0 and level1 >= chunks


@pytest.mark.parametrize("in_off", fe.IN_OFFS)
def test_boundary_walks_straddle_the_chunks_of_a_filter_launch(in_off):
    data, planted = fe.boundary_walks(in_off)
    head = fe.head16(in_off)
    assert data.size == fe.WALKS_N and len(planted) == len([s for s in te.plant_specs() if s[2] is not None]) + 1
    want = fe.want(data, "qq")
    assert all(want[at] == pid for at, pid in planted)
    sizes = {te.pattern_id(p): len(p) for p in te.PATTERNS}
    crossing = [(at, sizes[pid]) for at, pid in planted[:-1]]
    # every plant lies across a boundary of the launch's own grid (a short one: up to it) ...
    assert all(at - head <= -(-(at - head) // fe.CHUNK) * fe.CHUNK < at - head + max(size, 72) for at, size in crossing)
    deep = [(at, size) for at, size in crossing if size >= 200]
    ends = sorted((at - head + size - 1) % fe.CHUNK for at, size in deep)
    assert len(deep) == 18 and all(ends.count(e) >= 2 for e in te.END_BEHIND)        # ... ending 127, 128, 129 bytes behind it: the stage walker's kWalkHalo
    assert te.END_BEHIND == (fe.kWalkHalo - 1, fe.kWalkHalo, fe.kWalkHalo + 1)
    starts = {-(at - head) % fe.CHUNK for at, size in crossing if size == 60}
    assert set(range(0, 72, 7)) <= starts                                            # LONG_A itself: every seventh offset of the 72
    boundaries = {-(-(at - head) // fe.CHUNK) for at, _ in crossing}
    # span boundaries, on either side of the one between the parts' first granules (every boundary up to the last has a plant: a whole pattern or a near miss)
    assert sum(b % fe.kSpanChunks == 0 for b in boundaries) >= 10 and min(boundaries) <= 2 and max(boundaries) > fe.GRANULE + fe.kSpanChunks and len(boundaries) >= 50


@pytest.mark.parametrize("case", sorted(fe.DENSE_CASES))
def test_dense_cases_have_exactly_the_intended_dense_chunks(case):
    for in_off in fe.IN_OFFS:
        data = fe.dense_case(in_off, case)
        hits = fe.chunk_hits(fe.host_handle("qq"), 600, data, in_off, False)
        assert tuple(np.flatnonzero(hits > fe.PFAC_DENSE_HITS).tolist()) == fe.dense_chunks_of(case), (case, in_off, hits.tolist())
        assert fe.stats_of("qq", data, in_off, False)[1] == len(fe.dense_chunks_of(case))
    counts = {case: len(fe.dense_chunks_of(case)) for case in fe.DENSE_CASES}
    assert counts["first"] == counts["last"] == 1 and counts["stage"] == fe.kDenseStage and counts["stage+1"] == fe.kDenseStage + 1
    assert fe.DENSE_CASES["partial-span"][0] % fe.kSpanChunks != 0 and fe.dense_chunks_of("part-1") == (fe.GRANULE,)
    if case == "across-the-end":
        data = fe.dense_case(5, case)
        main_end = fe.head16(5) + fe.CHUNK * fe.DENSE_CASES[case][0]
        want = fe.want(data, "qq")
        assert np.all(want[main_end - fe.CROSS[0]:main_end + fe.CROSS[1] - 1] == 1) and want[main_end + fe.CROSS[1] - 1] == 0


@pytest.mark.parametrize("name,reduce", [("qq", False), ("long", False), ("qq", True)])
def test_threshold_chunks_have_exactly_the_intended_level_1_hits(name, reduce):
    """D.  One chunk each with PFAC_LIST_CAP - 1 .. PFAC_DENSE_HITS hits, between chunks with none.  (Under "long" no byte passes the compacted-output
    kernel's level 1 in a run: its list rounds are reached under "qq".)"""
    assert fe.HIT_TARGETS == (127, 128, 129, 255, 257, 1023, 1024)
    data, at = fe.hit_chunks(name, reduce)
    hits = fe.chunk_hits(fe.host_handle(name), 600, data, 0, reduce)
    for target, c in at.items():
        assert hits[c] == target and hits[c - 1] == 0 and hits[c + 1] == 0
    assert hits.sum() == sum(fe.HIT_TARGETS) and fe.stats_of(name, data, 0, reduce) == (sum(fe.HIT_TARGETS), 0)
    if name == "qq":
        assert np.count_nonzero(fe.want(data, "qq")) > sum(fe.HIT_TARGETS) * 3 // 4          # `q` runs: nearly every hit is a match, and walks


def test_walk_chunks_hold_exactly_the_intended_matches():
    assert fe.WALK_COUNTS == (1, 15, 16, 17, 63, 64, 65, 129, 300)
    data, at = fe.walk_chunks()
    for name in ("qq", "long"):
        want = fe.want(data, name)
        per_chunk = np.count_nonzero(want[:len(at) * 2 * fe.CHUNK + fe.CHUNK].reshape(-1, fe.CHUNK), axis=1)
        assert {count: int(per_chunk[c]) for count, c in at.items()} == {count: count for count in at}
        assert per_chunk.sum() == sum(fe.WALK_COUNTS)
        assert np.all(want[want != 0] == fe.SETS[name].index(fe.WALK_PATTERN) + 1)
        hits = fe.chunk_hits(fe.host_handle(name), 600, data, 0, False)
        assert all(hits[c] >= count for count, c in at.items()) and hits[at[300]] > 2 * fe.PFAC_LIST_CAP


def test_builders_are_deterministic():
    for build, cached in ((lambda: fe.seam("qq", 7, 2, 1, 3), fe.seam), (lambda: fe.handout(5, 14), fe.handout), (lambda: fe.hit_chunks("qq")[0], fe.hit_chunks),
                          (lambda: fe.dense_case(15, "stage+1"), fe.dense_case)):
        first = build().copy()
        cached.cache_clear()
        fe.handout.cache_clear()
        assert np.array_equal(build(), first)
