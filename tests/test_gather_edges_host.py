"""tests/gather_edges.py without a GPU: the constants are the sources'; gather_text equals lines_ref.gather_py over the clamped lines; every
case's claims hold for the grid it was built with, 256 compute units and 1; the plain Python transcription of the gather's kernels
(tile_model) equals gather_text; and every named off-by-one of the transcription changes the bytes of a case of the family that claims its
edge -- but for the four that provably change nothing (gather_edges.equivalent_mutants), which are pinned as such, each beside a neighbour
that does change the text.  The device form runs the same cases in tests/test_gather_edges_gpu.py.

Family E and the three large line counts of family D are built for a device; here their twins for one compute unit stand in: the same
builders, 10 lines of 64 KiB for 520, 2047 .. 2049 lines for 524287 .. 524289."""
import functools
import os
import re

import numpy as np
import pytest

from pfac_amd import api
from tests import gather_edges as ge
from tests import lines_ref

CSRC = os.path.join(os.path.dirname(os.path.abspath(api.__file__)), "csrc")
TILE = ge.TILE

# mutant -> the family whose cases must tell it from the kernel, and why there
CAUGHT_BY = {
    "first_le_plus_1": "A",             # a start on oLo + 1: thread 0 writes the newline on oLo by luck and goes on with the line behind the right one
    "last_lt_minus_16": "A",            # a start on the first byte of the tile's last thread is not staged
    "rel_lt": "C",                      # a line that starts on a thread's first byte
    "k_from_tile": "B",                 # a tile inside one line: k counts from the line's start, tiles in front of this one
    "per_unrounded_grid_kept": "D",     # 8 C 256 + 1 lines: the blocks of per = 512 with per = 257 leave the last lines without an offset
    "no_second_trip": "E",              # more tiles than blocks
}


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def built(compute_units):
    return ge.families(compute_units)


def affordable(family, case):
    """the cases whose text the byte-by-byte code of this file walks: all but the 2^32 bytes of family E"""
    return not (family == "E" and case[0] != ge.E_NAMES[0])


@functools.lru_cache(maxsize=None)
def reference(family, name):
    case = ge.by_name(built(1)[family])[name]
    return ge.gather_text(case[1], case[2], case[3]).tobytes()


def model(case, mutate=None):
    name, data, start, length, _, mis, capacity = case
    return ge.tile_model(data, start, length, mis, capacity, 1, mutate)


def expected(family, case):
    """what d_out holds: the text below the capacity, FILL where the call is truncated below it -- its contents are unspecified, the model
    writes the text's head"""
    want = reference(family, case[0])
    return want if case[6] is None else want[:case[6]]


# ---------------------------------------------------------------------------------------------------------------- the constants

def test_the_constants_are_the_sources():
    lines, passes = source("scan_lines.hip"), source("scan_passes.h")
    assert (ge.TILE, ge.STEP, ge.THREADS, ge.BLOCKS_PER_CU, ge.TILE_BLOCKS_PER_CU, ge.SCAN_STEP) == (4096, 16, 256, 8, 32, 1024)
    assert ge.TILE == api.PFACX_GATHER_TILE == api.PFACX_REPLACE_TILE and ge.THREADS == api.PFACX_GATHER_THREADS and ge.TILE == ge.THREADS * ge.STEP
    assert "constexpr unsigned int kOutTile = %d;" % ge.TILE in passes
    assert "constexpr unsigned int kLinesThreads = %d;" % ge.THREADS in lines
    assert "const unsigned long long v0 = vLo + (unsigned long long)threadIdx.x * %d;" % ge.STEP in passes
    assert "__shared__ unsigned int rel[kOutTile + 1];" in lines and "sCount = c > kOutTile ? kOutTile : (unsigned int)c;" in lines
    # the copy: at most 4 x 8 blocks per compute unit, a tile each per trip
    assert "dim3((unsigned int)(tiles < gridCap(c, %d) * 4ull ? tiles : gridCap(c, %d) * 4ull)), dim3(kLinesThreads), 0, 0, g);" % (8, 8) in lines
    assert ge.TILE_BLOCKS_PER_CU == 8 * 4
    assert "vLo < limit + g.misOut; vLo += (unsigned long long)gridDim.x * kOutTile" in lines
    # the cut of the count and the offsets passes
    body = re.search(r"inline unsigned int offsetBlocks\(const PFAC_context \*c, size_t count, unsigned int threads, size_t &per\)\s*\{(.*?)\n\}", passes, re.S)
    assert [s.strip() for s in body.group(1).strip().split("\n")] == [
        "size_t blocks = (count + threads - 1) / threads;",
        "if (blocks > gridCap(c, %d)) blocks = gridCap(c, %d);" % (ge.BLOCKS_PER_CU, ge.BLOCKS_PER_CU),
        "per = blocks ? ((count + blocks - 1) / blocks + threads - 1) / threads * threads : threads;",
        "return (unsigned int)((count + per - 1) / per);"]
    assert "g.blocks = offsetBlocks(c, numSelected, kLinesThreads, g.per);" in lines
    assert "const size_t end = count - first < per ? count : first + per;" in passes
    # the scan of the block totals: one block, 1024 at a time
    assert "hipLaunchKernelGGL(pfac_array_scan<unsigned long long>, dim3(1), dim3(%d), 0, 0, g.blockBase, g.blocks, g.blockBase + g.blocks," % ge.SCAN_STEP in lines
    assert "for (unsigned int base = 0; base < n; base += %d) {" % ge.SCAN_STEP in passes
    # the two searches and the thread's, as the mutants name them
    for text in ("if (g.off[mid] <= oLo) lo = mid; else hi = mid;", "if (g.off[mid] < oHi) lo2 = mid; else hi2 = mid;",
                 "if (rel[mid] <= r) lo = mid; else hi = mid;", "k = lo == 0 ? cLo - g.off[first] : (unsigned long long)(r - rel[lo]);"):
        assert text in lines, text
    assert {"first_lt", "last_le", "cap_minus_1", "rel_lt", "k_from_tile", "per_unrounded", "no_second_trip"} <= set(ge.MUTANTS)
    assert set(ge.MUTANTS) == set(CAUGHT_BY) | set(ge.equivalent_mutants())


def test_the_names_do_not_depend_on_the_device():
    for units in (1, 256, 304):
        assert {f: tuple(c[0] for c in cases) for f, cases in ge.families(units).items()} == ge.NAMES
    assert ge.NAMES["D"] == ge.D_NAMES and ge.NAMES["E"] == ge.E_NAMES
    assert {f: len(names) for f, names in ge.NAMES.items()} == {"A": 33, "B": 10, "C": 30, "D": 7, "E": 3, "F": 24, "G": 16}


# ---------------------------------------------------------------------------------------------------------------- the reference

def test_clamped_is_the_header():
    """s = min(max(start, 0), n); e = s if len <= 0 else min(n, s + len): by hand on the list of test_gather_clamps_bad_line_arrays and at
    the ends of int"""
    s, e = ge.clamped(10, [-4, 8, 1 << 30, 3, 10, ge.INT_MIN, ge.INT_MAX, 0, 4], [3, 100, 5, -2, 1, ge.INT_MAX, ge.INT_MAX, ge.INT_MIN, ge.INT_MAX])
    assert s.tolist() == [0, 8, 10, 3, 10, 0, 10, 0, 4] and e.tolist() == [3, 10, 10, 3, 10, 10, 10, 0, 10]
    data = np.frombuffer(b"0123456789", dtype=np.uint8)
    assert ge.gather_text(data, [-4, 8, 1 << 30, 3, 10], [3, 100, 5, -2, 1]).tobytes() == b"012\n89\n\n\n\n"
    assert ge.gather_total(10, [-4, 8, 1 << 30, 3, 10], [3, 100, 5, -2, 1]) == 10
    assert ge.gather_text(data[:0], [0, 5], [1, 0]).tobytes() == b"\n\n", "an empty input: every line is empty"


@pytest.mark.parametrize("family", sorted(ge.NAMES))
def test_gather_text_is_gather_py_over_the_clamped_lines(family):
    for case in built(1)[family]:
        name, data, start, length = case[:4]
        total = ge.gather_total(data.size, start, length)
        assert case.total() == total
        if not affordable(family, case):
            assert total == (1 << 16) * (ge.E_INPUT + 1) == 1 << 32, "by hand: 65536 lines of 65535 bytes and a newline"
            continue
        s, e = ge.clamped(data.size, start, length)
        want = lines_ref.gather_py(data.tobytes(), s, e - s)
        assert reference(family, name) == want and total == len(want), name


# ---------------------------------------------------------------------------------------------------------------- the claims

@pytest.mark.parametrize("compute_units", [256, 1, 304])
@pytest.mark.parametrize("family", sorted(ge.NAMES))
def test_every_claim_holds_for_its_grid(family, compute_units):
    for case in built(compute_units)[family]:
        ge.check_claims(case, compute_units)


def test_what_the_full_size_cases_reach_on_256_compute_units():
    """by hand, for the device the sizes were chosen for"""
    d, e = ge.by_name(built(256)["D"]), ge.by_name(built(256)["E"])
    assert [int(d[n][2].size) for n in ge.D_NAMES] == [255, 256, 257, 513, 524287, 524288, 524289]
    assert [ge.offset_blocks(int(d[n][2].size), 256) for n in ge.D_NAMES] == [(1, 256), (1, 256), (2, 256), (3, 256), (2048, 256), (2048, 256), (1025, 512)]
    assert all(("scan_steps", 2) in d[n].claims for n in ge.D_NAMES[4:]), "pfac_array_scan over more than 1024 block totals: carry"
    assert 1.4e6 < d["D-full+1"].total() < 1.7e6, "about 1.5 MiB of text"
    big = e[ge.E_NAMES[0]]
    assert int(big[2].size) == 520 and big.total() == 520 << 16 and big.total() > 32 * 256 * TILE + 8 * TILE, "32.5 MiB: 128 tiles past one pass"
    assert all(e[n].total() == 1 << 32 for n in ge.E_NAMES[1:])


# ---------------------------------------------------------------------------------------------------------------- the model

@pytest.mark.parametrize("family", sorted(ge.NAMES))
def test_the_model_is_the_reference(family):
    for case in built(1)[family]:
        if affordable(family, case):
            assert model(case) == expected(family, case), case[0]


def test_the_model_of_the_offsets_at_both_grids():
    """the three launches in front of the copy against cumsum, at the cut for 256 compute units too: 1025 blocks of 512 lines, two steps of
    the scan"""
    for units in (1, 256):
        for case in built(units)["D"]:
            off, total = ge.offsets(case[1].size, case[2], case[3])
            got = ge.model_offsets(case[1].size, case[2], case[3], units)
            assert got[1] == total and np.array_equal(np.asarray(got[0], dtype=np.int64), off), (units, case[0])
    assert ge.model_offsets(ge.E_INPUT, *built(1)["E"][1][2:4], 1)[1] == 1 << 32


def test_the_model_writes_nothing_outside_a_smaller_capacity():
    case = ge.by_name(built(1)["A"])["A-out15-tile1-oHi-1"]
    want = reference("A", case[0])
    for capacity in (0, 1, TILE - 16, TILE - 15, TILE, len(want) - 1):
        assert ge.tile_model(case[1], case[2], case[3], 15, capacity, 1) == want[:capacity]


@pytest.mark.parametrize("mutant", sorted(CAUGHT_BY))
def test_every_mutant_is_caught_by_the_family_that_claims_its_edge(mutant):
    family = CAUGHT_BY[mutant]
    caught = [case[0] for case in built(1)[family] if affordable(family, case) and model(case, mutant) != expected(family, case)]
    assert caught, "no case of family %s tells %s (%s) from the kernel" % (family, mutant, ge.MUTANTS[mutant])
    by_hand = {"first_le_plus_1": {"A-out%d-%s-oLo+1" % (mis, tile) for mis in ge.A_OFFSETS for tile in ("tile1", "last")},
               "last_lt_minus_16": {"A-out%d-tile1-oHi-16" % mis for mis in ge.A_OFFSETS},
               "k_from_tile": {"B-out0-long-line", "B-out7-long-line"},
               "rel_lt": {"C-out%d-runs" % mis for mis in range(ge.STEP)},
               "per_unrounded_grid_kept": {"D-full+1"},
               "no_second_trip": {ge.E_NAMES[0]}}[mutant]
    assert by_hand <= set(caught), (mutant, sorted(by_hand - set(caught)))


@pytest.mark.parametrize("mutant", sorted(ge.equivalent_mutants()))
def test_the_equivalent_mutants_change_no_byte(mutant):
    """first_lt, last_le, cap_minus_1 and per_unrounded (gather_edges.equivalent_mutants says why): no case can catch them, so the claim is
    turned round and pinned -- over every family: family A has the starts on oLo and oHi, family B the tiles with 4096 staged offsets whose
    last is a line that is not empty, family D every cut.  A change to the kernel that makes one of them matter fails here and has to bring
    its case"""
    for family in sorted(ge.NAMES):
        for case in built(1)[family]:
            if affordable(family, case):
                assert model(case, mutant) == expected(family, case), (mutant, case[0])
    if mutant == "per_unrounded":
        for units in (1, 256):
            for case in built(units)["D"]:
                plain = ge.model_offsets(case[1].size, case[2], case[3], units)
                assert ge.model_offsets(case[1].size, case[2], case[3], units, mutant) == plain, (units, case[0])
        assert ge.offset_blocks(524289, 256, mutant) == (2041, 257) and ge.offset_blocks(524289, 256) == (1025, 512)
