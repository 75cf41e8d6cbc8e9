"""pfac_scan_filter (scan_filter.hip) at its chunk, span, grid and input-end edges: the kernel of every large call, here under
PFACX_KERNEL_FILTER on inputs of a few KiB to 1 MiB.  The launcher gives it the whole 2 KiB chunks between the first 16-byte aligned input byte
and maxPatternLen + 64 + kWalkHalo bytes before the end (scan_module.hip: headPositions, filterLength); the positions in front and behind are walked
with bounds by the same launch (ScanArgs::endsIn).  Chunks are handed out in order: spans of 4 chunks claimed by writer waves, granules of 16 spans
dealt to min(gridDim, 2) parts (full result); batches of 16 chunks claimed by the scanning waves, over up to 32 parts (compacted output).  A wave lists
128 level-1 hits at a time, queues 64 walks, stages 16 pairs (compacted output) and 8 dense chunk numbers (full result: a chunk with more than
1024 hits goes to the tiled kernel behind the launch).

Every expected value is the oracle's result on exactly the bytes the call was given (tests/filter_edges.py: want).  Every call has poisoned result
buffers whose surroundings must stay as they were, and the device memory around the input holds bytes that would complete a match.

That a call reached the kernel, with the plan the test assumes, is asserted through PFACX_getScanStats: level1Hits is the kernel's sum of the hits it
LISTED -- a dense chunk lists nothing (`listed` in scan_filter.hip), the bounded walks of the ends are not filtered -- so it equals the model's hits
(tests/filter_model.py) over the non-dense chunks of [head, head + main_len) of the launch's own grid and of no other; denseChunks equals the model's
count on that grid, with an aligned and with a misaligned input (tests/filter_edges.py: expected_stats follows the launcher's grid, where
test_chunks_on_either_side_of_the_dense_threshold models the aligned one only).  Which instance ran (walker, veto, the compacted-output kernel's two
walks per lane) is asserted on handles whose walker is forced, so that a session under PFAC_TEST_WALKER asserts the same; TEX is what the handle's
texture mode says, HAS_SHORT what the set's compiled filter says (tests/test_filter_edges_host.py pins it per set)."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import filter_edges as fe  # noqa: E402
from tests.gpu_helpers import MODES, STAGE, VARIANTS, VETO, assert_pairs, assert_same, device_match, device_reduce, make_handle  # noqa: E402

FILTER = api.PFACX_KERNEL_FILTER
WINDOW = api.PFACX_WALKER_WINDOW << 8
TEX_MODES = [MODES[1], MODES[2]]                 # dense-buffer (TEX), hash-global (no TEX): throughout
OTHER_MODES = [MODES[0], MODES[3]]               # once per group: the filter kernel walks the chained table in both perf modes
ZERO_STATS = ("walkerRounds", "laneSteps", "walksStarted", "level1Hits", "ladderCandidates", "denseChunks", "walksPerLane", "stageModeWaves", "veto")


@pytest.fixture(scope="module")
def handles():
    """handle(set name, variant, mode): one handle per combination for the whole file, as a caller keeps one across calls of every size"""
    made = {}

    def handle(name, variant, mode):
        key = (name, variant, mode[2])
        if key not in made:
            made[key] = make_handle(fe.pattern_file(name), mode[0], mode[1], variant)
        return made[key]

    yield handle
    for h in made.values():
        h.destroy()


def check_full(h, name, data, what, in_off=0, out_off=0, **around):
    """a full-result call against the oracle, and its launch against the model of the plan"""
    assert_same(device_match(h, data, in_off, out_off, **around), fe.want(data, name), what)
    if fe.plan(in_off, data.size, fe.MAX_LEN[name], False)[2]:
        st = h.scanStats()
        assert (st["level1Hits"], st["denseChunks"], st["walksPerLane"]) == fe.stats_of(name, data, in_off, False) + (1,), (what, st)


def check_reduce(h, name, data, what, in_off=0, **around):
    """a compacted-output call: the oracle's non-zero results in position order, none twice; its launch against the model"""
    assert_pairs(device_reduce(h, data, in_off, **around), fe.want(data, name), what + "/compacted")
    if fe.plan(in_off, data.size, fe.MAX_LEN[name], True)[2]:
        st = h.scanStats()
        assert (st["level1Hits"], st["denseChunks"], st["walksPerLane"], st["veto"]) == (fe.stats_of(name, data, in_off, True)[0], 0, 2, 0), (what, st)


# ------------------------------------------------------------------------------------------------------------------------------- A

@pytest.mark.parametrize("in_off", range(16))
def test_end_of_the_main_part_at_every_misalignment(handles, in_off):
    """A.  n = head + 2048 k + margin + d for k = 1, 2 and d = -1 (k = 1: the last size without a filter launch), 0, 1, 1024, 2047 (the longest
    tail), under "qq", "long" (maxPatternLen 600) and "min3" (3: the smallest margin); the input in_off bytes and the result 0..3 ints behind a 16-byte
    address.  Four variants of every input: LONG_A from main_end - 1, main_end, main_end - 60, P600 from the last chunk into the tail;
    a pattern at 0, at head - 1, on the first aligned byte; all of them: P600 ending exactly at n with the rest of TAIL_CUT behind the input, `q`
    in front of it.  Full result and compacted output, with and without buffer loads.
    On a fresh handle the one size below a chunk leaves the statistics of the filter kernel all zero: no launch."""
    for name in fe.A_SETS:
        for k in fe.A_K:
            for d in fe.A_D:
                for v in range(fe.A_VARIANTS):
                    data = fe.seam(name, in_off, k, d, v)
                    for mode in TEX_MODES:
                        h = handles(name, FILTER, mode)
                        what = f"{name}/{mode[2]}/in +{in_off}/k {k}/d {d}/variant {v}"
                        for out_off in range(4):
                            check_full(h, name, data, f"{what}/out +{out_off}", in_off, out_off, **fe.A_AROUND)
                        check_reduce(h, name, data, what, in_off, **fe.A_AROUND)
        mode = MODES[in_off % 4]
        fresh = make_handle(fe.pattern_file(name), mode[0], mode[1], FILTER)
        try:
            data = fe.seam(name, in_off, 1, -1, in_off % fe.A_VARIANTS)
            assert fe.plan(in_off, data.size, fe.MAX_LEN[name], False)[2] == 0 and fe.plan(in_off, data.size + 1, fe.MAX_LEN[name], False)[2] == 1
            check_full(fresh, name, data, f"{name}/fresh/in +{in_off}", in_off, 1, **fe.A_AROUND)
            check_reduce(fresh, name, data, f"{name}/fresh/in +{in_off}", in_off, **fe.A_AROUND)
            st = fresh.scanStats()
            assert all(st[key] == 0 for key in ZERO_STATS), st
            one_more = fe.seam(name, in_off, 1, 0, 0)
            check_full(fresh, name, one_more, f"{name}/fresh/in +{in_off}/one chunk", in_off, 0, **fe.A_AROUND)
            assert fresh.scanStats()["walksPerLane"] == 1 and fresh.scanStats()["walkerRounds"] > 0
        finally:
            fresh.destroy()


def test_end_of_the_main_part_in_the_other_table_modes(handles):
    for name in fe.A_SETS:
        for mode in OTHER_MODES:
            for in_off, k, d, v in ((0, 1, 0, 0), (3, 2, 2047, 1), (8, 1, 1, 2), (13, 2, -1, 3)):
                data = fe.seam(name, in_off, k, d, v)
                what = f"{name}/{mode[2]}/in +{in_off}/k {k}/d {d}/variant {v}"
                check_full(handles(name, FILTER, mode), name, data, what, in_off, v, **fe.A_AROUND)
                check_reduce(handles(name, FILTER, mode), name, data, what, in_off, **fe.A_AROUND)


# --------------------------------------------------------------------------------------------------------------------- the instances

INSTANCES = [("min3", WINDOW, api.PFACX_WALKER_WINDOW, 0, False), ("long", WINDOW, api.PFACX_WALKER_WINDOW, 1, False), ("qq", VETO, api.PFACX_WALKER_WINDOW, 1, True),
             ("min3", VETO, api.PFACX_WALKER_WINDOW, 0, False), ("qq", STAGE, api.PFACX_WALKER_STAGE, 0, True), ("long", STAGE, api.PFACX_WALKER_STAGE, 0, False)]


@pytest.mark.parametrize("name,variant,walker,veto,has_short", INSTANCES)
def test_every_instance_is_reached(handles, name, variant, walker, veto, has_short):
    """The walker forced (a launch under PFACX_WALKER_AUTO takes what the handle's previous launch voted for): the plain window walker ("min3": no tail
    table), VETO = 1 ("long", "qq": a tail table in LDS), the stage walker; HAS_SHORT on ("qq") and off; with and without buffer loads; and the
    compacted-output kernel of the same handles -- on one chunk and on the hand-out's largest size."""
    for mode in TEX_MODES:
        h = handles(name, FILTER | variant, mode)
        assert bool(h.info().filterHasShort) == has_short and (h.info().filterTailEntries > 0) == (name != "min3")
        for in_off, chunks in ((0, 1), (5, 3 * fe.GRANULE + 1)):
            data = fe.handout(in_off, chunks)
            what = f"{name}/{mode[2]}/in +{in_off}/{chunks} chunks"
            check_full(h, name, data, what, in_off, 3, front=fe.Q, behind=b"q" * 8)
            st = h.scanStats()
            assert (st["walker"], st["veto"]) == (walker, veto), (what, st)
            check_reduce(h, name, data, what, in_off, front=fe.Q, behind=b"q" * 8)


# ------------------------------------------------------------------------------------------------------------------------------- B

@pytest.mark.parametrize("chunks", fe.FULL_CHUNKS)
def test_hand_out_of_the_full_result_kernel(handles, chunks):
    """B.  1 .. kSpanChunks + 1 chunks (one chunk, the partial last span), scanners - 1 .. + 1 and 2 scanners (+ 1) (one, two, three blocks; parts =
    min(gridDim, 2); the third block serves part 0 again), granule - 1 .. + 1 (chunk 64: the first piece part 1 ever gets), granule + span (+ 1),
    2 granules -+ 1, 3 granules + 1.  Every chunk holds one match at an offset of its own: a chunk nobody took keeps its poison."""
    for in_off in fe.IN_OFFS:
        data = fe.handout(in_off, chunks)
        for name in ("qq", "long"):
            for mode in TEX_MODES:
                for out_off in (0, 3):
                    check_full(handles(name, FILTER, mode), name, data, f"{name}/{mode[2]}/{chunks} chunks/+{in_off},+{out_off}", in_off, out_off, front=fe.Q, behind=b"q" * 8)


@pytest.mark.parametrize("chunks", fe.REDUCE_CHUNKS)
def test_hand_out_of_the_compacted_output_kernel(handles, chunks):
    """B.  1 chunk, batch - 1 .. + 1 (a batch: the 16 chunks a wave claims per atomic), 2 batches (+ 1), PFAC_REDUCE_PARTS batches - 1 .. + 1 (33 blocks:
    the 33rd serves part 0 again) and a batch more: a chunk taken twice has its pair twice."""
    for in_off in fe.IN_OFFS:
        data = fe.handout(in_off, chunks)
        for name in ("qq", "long"):
            for mode in TEX_MODES:
                check_reduce(handles(name, FILTER, mode), name, data, f"{name}/{mode[2]}/{chunks} chunks/+{in_off}", in_off, front=fe.Q, behind=b"q" * 8)


@pytest.mark.parametrize("in_off", fe.IN_OFFS)
def test_walks_across_the_boundaries_of_chunks_spans_and_granules(handles, in_off):
    """B.  tiled_edges' plants across every chunk boundary of the launch's own grid up to the 109th: span boundaries and the granule boundary at
    128 KiB, where a walk's chunk and the next belong to different blocks.  60-byte matches, near misses and prefix-patterns at every offset 0..71,
    the 200- and 600-byte patterns from 1..199 bytes in front of a chunk's end and ending 127, 128 and 129 bytes behind it (the stage walker's
    kWalkHalo), P600 ending with the input.  Every walker, and the compacted output; at in_off 0 in all four table modes."""
    data, _ = fe.boundary_walks(in_off)
    for name in ("qq", "long"):
        for mode in (MODES if in_off == 0 else TEX_MODES):
            for variant, variant_name in VARIANTS[:3]:
                h = handles(name, variant, mode)
                what = f"{name}/{variant_name}/{mode[2]}/+{in_off}"
                check_full(h, name, data, what, in_off, in_off % 4, front=fe.Q, behind=b"ABCDEFGH")
                if variant_name == "filter-stage":
                    assert h.scanStats()["walker"] == api.PFACX_WALKER_STAGE, what
                if variant_name == "filter-veto":
                    assert h.scanStats()["veto"] == 1, what
            check_reduce(handles(name, FILTER, mode), name, data, f"{name}/{mode[2]}/+{in_off}", in_off, front=fe.Q, behind=b"ABCDEFGH")


# ------------------------------------------------------------------------------------------------------------------------------- C

@pytest.mark.parametrize("case", sorted(fe.DENSE_CASES))
def test_dense_chunks_at_the_edges_of_the_hand_out(handles, case):
    """C.  `q` runs under "qq" make dense: the first chunk, the last of the main part, the chunks of a partial last span, chunk 64, kDenseStage and
    kDenseStage + 1 chunks, every chunk, and the last chunk with a run that goes on into the bounded walks behind main_end.  check_full compares
    denseChunks with the model's count on the launch's grid."""
    for in_off in fe.IN_OFFS:
        data = fe.dense_case(in_off, case)
        assert fe.stats_of("qq", data, in_off, False)[1] == len(fe.dense_chunks_of(case))
        for mode in TEX_MODES:
            for out_off in (0, 3):
                check_full(handles("qq", FILTER, mode), "qq", data, f"{case}/{mode[2]}/+{in_off},+{out_off}", in_off, out_off, front=fe.Q, behind=b"q" * 8)
    for mode in OTHER_MODES:
        check_full(handles("qq", FILTER, mode), "qq", fe.dense_case(5, case), f"{case}/{mode[2]}/+5,+1", 5, 1, front=fe.Q, behind=b"q" * 8)


@pytest.mark.parametrize("chunks", fe.DENSE_SET_CHUNKS)
def test_hand_out_when_every_chunk_is_dense(handles, chunks):
    """C.  The "q" set: every chunk goes on the dense list, the tiled kernel's list mode does all of the main part (level1Hits 0, denseChunks = chunks)."""
    for in_off in fe.IN_OFFS:
        data = fe.handout(in_off, chunks)
        assert fe.stats_of("q", data, in_off, False) == (0, chunks)
        for mode in TEX_MODES:
            for out_off in (0, 3):
                check_full(handles("q", FILTER, mode), "q", data, f"q/{mode[2]}/{chunks} chunks/+{in_off},+{out_off}", in_off, out_off, front=fe.Q, behind=b"q" * 8)
            check_reduce(handles("q", FILTER, mode), "q", data, f"q/{mode[2]}/{chunks} chunks/+{in_off}", in_off, front=fe.Q, behind=b"q" * 8)


@pytest.mark.parametrize("perf,tex,mode_name", TEX_MODES)
def test_the_two_dense_counter_words_alternate(perf, tex, mode_name):
    """C.  Launches count their dense chunks in two words in turn, and each word is zeroed by the launch after the one that used it: dense, sparse,
    dense, dense (and sparse, dense again) on ONE handle, each call's count and result right."""
    h = make_handle(fe.pattern_file("qq"), perf, tex, FILTER)
    try:
        for call, case in enumerate(("stage+1", None, "all", "partial-span", None, "stage")):
            data = fe.dense_case(0, case) if case else fe.handout(0, fe.kSpanChunks + 1)
            check_full(h, "qq", data, f"{mode_name}/call {call}: {case or 'sparse'}")
            assert h.scanStats()["denseChunks"] == (len(fe.dense_chunks_of(case)) if case else 0)
    finally:
        h.destroy()


# ------------------------------------------------------------------------------------------------------------------------------- D

@pytest.mark.parametrize("name", ["qq", "long"])
def test_chunks_on_either_side_of_the_list_rounds_and_the_dense_threshold(handles, name):
    """D.  Chunks with exactly PFAC_LIST_CAP - 1, PFAC_LIST_CAP, + 1 level-1 hits (one list round | two), 2 PFAC_LIST_CAP -+ 1 (two | three),
    PFAC_DENSE_HITS - 1 and PFAC_DENSE_HITS (eight rounds; one hit more would be dense), each among chunks without a hit.  Under "qq" the hits are `q`
    runs -- a match and a walk each: the 64-entry queue overflows, batches wait for room --, under "long" a byte that no pattern holds: the list alone.
    The compacted-output kernel has a level 1 of its own: "qq" again with the counts set by ITS model."""
    data, _ = fe.hit_chunks(name)
    assert fe.stats_of(name, data, 0, False) == (sum(fe.HIT_TARGETS), 0)
    for mode in MODES:
        for variant, variant_name in VARIANTS[:3]:
            check_full(handles(name, variant, mode), name, data, f"{name}/{variant_name}/{mode[2]}", front=fe.Q, behind=b"q" * 8)
        check_reduce(handles(name, FILTER, mode), name, data, f"{name}/{mode[2]}", front=fe.Q, behind=b"q" * 8)
    if name == "qq":
        data, _ = fe.hit_chunks("qq", True)
        assert fe.stats_of("qq", data, 0, True) == (sum(fe.HIT_TARGETS), 0)
        for mode in MODES:
            check_reduce(handles("qq", FILTER, mode), "qq", data, f"qq/{mode[2]}/its own level 1", front=fe.Q, behind=b"q" * 8)
            check_full(handles("qq", FILTER, mode), "qq", data, f"qq/{mode[2]}/the compacted kernel's counts", front=fe.Q, behind=b"q" * 8)


@pytest.mark.parametrize("name", ["qq", "long"])
def test_chunks_on_either_side_of_the_walk_queue_and_the_pair_staging(handles, name):
    """D.  Chunks with 1, kReduceCap - 1 .. + 1, PFAC_QUEUE_CAP - 1 .. + 1, 2 PFAC_QUEUE_CAP + 1 and 300 whole patterns of one length, six bytes apart:
    walks that start together end together -- the queue fills and overflows, ladder batches wait for room (PFAC_APPEND_MIN, PFAC_MERGE_MIN), and in the
    compacted output a ballot of up to kReduceCap finished walks is staged, a larger one goes out directly.  Pairs come back in position order, none twice."""
    data, _ = fe.walk_chunks()
    for mode in MODES:
        for variant, variant_name in VARIANTS[:3]:
            h = handles(name, variant, mode)
            check_full(h, name, data, f"{name}/{variant_name}/{mode[2]}", front=fe.Q, behind=b"q" * 8)
            assert h.scanStats()["walksStarted"] >= sum(fe.WALK_COUNTS)
        check_reduce(handles(name, FILTER, mode), name, data, f"{name}/{mode[2]}", front=fe.Q, behind=b"q" * 8)
        assert handles(name, FILTER, mode).scanStats()["walksStarted"] >= sum(fe.WALK_COUNTS)


# ------------------------------------------------------------------------------------------------------------------------------- E

@pytest.mark.parametrize("seed", range(16))
def test_fuzzed_pattern_sets_through_the_filter_kernel(workdir, seed):
    """E.  The generator of test_fuzzed_pattern_sets_over_tiny_alphabets (tiny alphabets, 1- and 2-byte patterns on odd seeds, bytes 0x00 and 0xFF,
    almost every position walks or its chunk is dense), at least five chunks of main part, aligned and 7 bytes behind a 16-byte address, full and
    compacted, with and without buffer loads; level1Hits and denseChunks against the model of the set's own tables."""
    from oracle import binding as ob
    pf, data = fe.fuzz_input(workdir, seed)
    o = ob.Oracle(pf, hashed=False)
    want = o.match(data)
    o.close()
    host = api.PFAC.createHostOnly()
    host.readPatternFromFile(pf)
    max_len = host.info().maxPatternLen
    expected = {(in_off, reduce): fe.expected_stats(host, max_len, data, in_off, reduce) for in_off in (0, 7) for reduce in (False, True)}
    host.destroy()
    assert fe.plan(7, data.size, max_len, False)[2] >= fe.FUZZ_MIN_CHUNKS
    for mode in TEX_MODES:
        h = make_handle(pf, mode[0], mode[1], FILTER)
        try:
            for in_off in (0, 7):
                what = f"fuzz seed {seed}/{mode[2]}/+{in_off}"
                assert_same(device_match(h, data, in_off, seed % 4), want, what)
                st = h.scanStats()
                assert (st["level1Hits"], st["denseChunks"]) == expected[in_off, False], (what, st)
                assert_pairs(device_reduce(h, data, in_off), want, what + "/compacted")
                st = h.scanStats()
                assert (st["level1Hits"], st["walksPerLane"]) == (expected[in_off, True][0], 2), (what, st)
        finally:
            h.destroy()
