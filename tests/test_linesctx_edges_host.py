"""The cases of tests/linesctx_edges.py, without a device: every case holds the shape its name says -- the number of lines, the line block,
word and bit of each hit, the position blocks B from size and offset, a hit on either side of block 8191 | 8192, two members more than a block of
the block scan apart -- H as the builders state it equals linesctx_ref.members() where that matcher is affordable (families A and B), and
PFACX_matchLinesContextFromHost on a host-only handle equals the model for every case of A and B and for the smallest of C and of D.  The
device form runs the same cases in tests/test_linesctx_edges_gpu.py."""
import functools

import numpy as np
import pytest

from pfac_amd import api
from tests import linesctx_edges as le
from tests import linesctx_ref as model
from tests.lines_helpers import pattern_file
from tests.linesctx_helpers import host_context

A = le.by_name(le.line_block_edges())
B = le.by_name(le.groups_across_edges())
MIB = 1 << 20


@pytest.fixture(scope="module")
def x_handle(workdir):
    h = api.PFAC.createHostOnly()
    h.setPlatform(api.PFAC_PLATFORM_CPU)
    h.readPatternFromFileEx(pattern_file(workdir, "ctx_edges_x", model.X), 0)
    yield h
    h.destroy()


@functools.lru_cache(maxsize=None)
def matcher_members(data, invert):
    return model.members(model.X, data, invert)


def check(h, case):
    name, pats, data, before, after, invert, H = case
    want = model.context_model(pats, data, before, after, invert, H=H)
    model.same(host_context(h, data, before, after, invert), want, name)
    return want


# ---------------------------------------------------------------------------------------------------------------- the constants

def test_the_constants_are_the_kernels():
    """the numbers the cases are built around, read from the sources they come from"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pfac_amd", "csrc")
    lines, passes = open(os.path.join(csrc, "scan_lines.hip")).read(), open(os.path.join(csrc, "scan_passes.h")).read()
    number = lambda text, pattern: int(re.search(pattern, text).group(1))  # noqa: E731
    assert 1 << number(lines, r"kBlockShift = (\d+);") == le.BLOCK == number(lines, r"kBlockWords = (\d+);") * le.WORD
    assert number(lines, r"kLinesThreads = (\d+);") // 64 == le.WAVES_PER_GROUP
    assert number(lines, r"waveGridFor\(.*gridCap\(c, (\d+)\); \}") == le.GROUPS_PER_CU
    assert 1024 * number(passes, r"kScanPer = (\d+);") == le.SCAN_BLOCK and "kScanBlock = 1024 * kScanPer" in passes
    assert le.GRID_PASS == le.grid_pass(256) == 8192 == le.SCAN_BLOCK


# ---------------------------------------------------------------------------------------------------------------- A

def test_family_a_holds_its_shapes():
    assert le.A_LINE_COUNTS == (2047, 2048, 2049, 4095, 4096, 4097)
    assert {num: le.a_hits(num) for num in le.A_LINE_COUNTS} == {
        2047: [0, 2046], 2048: [0, 2046, 2047], 2049: [0, 2046, 2047, 2048], 4095: [0, 2046, 2047, 2048, 2049, 4094],
        4096: [0, 2046, 2047, 2048, 2049, 4095], 4097: [0, 2046, 2047, 2048, 2049, 4096]}
    for num, hit, terminated in le.a_shapes():
        data = le.short_lines(num, (hit,), terminated)
        starts, lens = model.all_lines(data)
        assert starts.size == num and data.endswith(b"\n") == terminated, (num, hit, terminated)
        assert data.count(b"x") == 1 and data[starts[hit]:starts[hit] + lens[hit]] == b"x", (num, hit, terminated)
        assert le.place(hit) == le.A_HIT_PLACES[hit], hit
    # the window values of the issue, every one on either side
    assert le.A_WINDOW_VALUES == (0, 1, 31, 32, 33, 2047, 2048, model.MAX)
    assert {b for b, _ in le.A_WINDOWS} == set(le.A_WINDOW_VALUES) == {a for _, a in le.A_WINDOWS}
    assert len(A) == len(le.a_shapes()) * len(le.A_WINDOWS) * 2 == 54 * 9 * 2
    # a window that ends exactly at the last line, from the last bit of a line block and from the first of the next
    ends_at_the_last_line = [c[0] for c in A.values() if not c[5] and c[4] != 0 and int(c[6][0]) + c[4] == model.all_lines(c[2])[0].size - 1]
    assert {"A-2048-hit2046-b33-a1", "A-4096-hit2047-b1-a2048", "A-4096-hit2048-bmax-a2047"} <= set(ends_at_the_last_line)
    for name, _, data, _, _, invert, H in A.values():
        num = int(name.split("-")[1])
        assert H.size == (num - 1 if invert else 1) and np.all(np.diff(H) > 0) and ("-inverted" in name) == invert


@pytest.mark.parametrize("name", sorted(A))
def test_line_block_edges(x_handle, name):
    case = A[name]
    assert np.array_equal(case[6], matcher_members(case[2], case[5])), "H by construction is what a matcher finds"
    want = check(x_handle, case)
    if not case[5]:
        num, hit, before, after = int(name.split("-")[1]), int(case[6][0]), case[3], case[4]
        assert want[2].tolist() == list(range(max(0, hit - before), min(num - 1, hit + after) + 1)), "one window, clipped to the lines"


# ---------------------------------------------------------------------------------------------------------------- B

def test_family_b_holds_its_shapes():
    assert [le.b_hits(p) for p in le.B_PHASES] == [
        [2040, 2044, 2048, 2052, 2056, 4088, 4092, 4096, 4100, 4104], [2041, 2045, 2049, 2053, 4089, 4093, 4097, 4101],
        [2042, 2046, 2050, 2054, 4090, 4094, 4098, 4102], [2043, 2047, 2051, 2055, 4091, 4095, 4099, 4103]]
    assert {b + a for b, a in le.B_WINDOWS} == {0, 1, 2, 3, 4}, "apart (< 3), touching (3) and overlapping (4)"
    assert {(b, a) for b, a in le.B_WINDOWS if b + a == 3} == {(2, 1), (1, 2), (3, 0), (0, 3)}, "the touching windows meet at every line of the period"
    for name, _, data, before, after, invert, H in B.values():
        starts = model.all_lines(data)[0]
        assert starts.size == le.B_LINES == 4112 and not invert and data.count(b"x") == H.size
        if le.b_by_hand(name) is not None:
            e = int(name.split("-")[1])
            assert e in (2048, 4096) and starts[e] % 32 == 0, name + ": a word of the newline bitmap starts with the line block's first line"
    # where the windows of two neighbours touch (after + before = 3), the four phases put the seam between any two lines of 2044 .. 2048
    seams = set()
    for phase in le.B_PHASES:
        for before, after in ((2, 1), (1, 2), (3, 0), (0, 3)):
            seams |= {h + after for h in le.b_hits(phase) if h + 4 in le.b_hits(phase)}
    assert {2046, 2047, 2048, 4094, 4095, 4096} <= seams, "a seam in front of, on and behind each edge"
    assert len(B) == len(le.B_PHASES) * len(le.B_WINDOWS) + 2 * len(le.B_EDGES)


@pytest.mark.parametrize("name", sorted(B))
def test_groups_across_a_line_block_edge(x_handle, name):
    case = B[name]
    assert np.array_equal(case[6], matcher_members(case[2], False)), "H by construction is what a matcher finds"
    want = check(x_handle, case)
    by_hand = le.b_by_hand(name)
    if by_hand is not None:
        groups, listed, members = by_hand
        assert ((want[3] >> 1).tolist(), want[2].tolist(), want[2][(want[3] & 1) == 1].tolist()) == (groups, listed, members), "the model and the count by hand"
        assert want[4][3] == groups[-1] + 1


def test_touching_windows_are_one_group_and_a_gap_of_one_line_makes_two():
    """family B's windows over the hits 2044 and 2048: the count of groups around the edge, by hand"""
    for before, after in le.B_WINDOWS:
        want = model.context_model(*B["B-every-fourth-from-2040-b%d-a%d" % (before, after)][1:6], H=np.asarray(le.b_hits(0)))
        groups = (want[3] >> 1)[(want[2] >= 2044) & (want[2] <= 2048)]
        assert np.unique(groups).size == (2 if before + after < 3 else 1), (before, after)


# ---------------------------------------------------------------------------------------------------------------- C

C_BLOCKS = {le.C_SIZES[0]: 8192, le.C_SIZES[1]: 8193, le.C_SIZES[2]: 16386}
# the block each hit's line ends in: block 0, the blocks on either side of one pass of 8192, the last block that holds bytes, and the last
# block, which holds nothing but the virtual newline of the unterminated last line
C_HIT_BLOCKS = {le.C_SIZES[0]: [0, 8190, 8191], le.C_SIZES[1]: [0, 8191, 8192], le.C_SIZES[2]: [0, 8191, 8192, 16384, 16385]}


def holds_its_shape(text, blocks, hit_blocks):
    starts, lens = model.all_lines(text.data)
    assert starts.size == text.num_lines and np.array_equal(starts + lens, text.ends) and text.data[-1] != le.NL
    assert lens[:-1].min() >= 20 and lens[:-1].max() <= 200 and 20 <= lens[-1] <= 222
    assert text.blocks == blocks == le.position_blocks(text.size, text.mis)
    H = text.H()
    at = np.flatnonzero(text.data == le.HIT)
    assert at.size == H.size and np.array_equal(np.searchsorted(text.ends, at, side="left"), H), "an 'x' in every line of H and nowhere else"
    assert [text.block_of(int(h)) for h in H] == hit_blocks
    assert np.array_equal(text.H(True), np.setdiff1d(np.arange(text.num_lines), H))
    return starts, lens


def test_family_c_holds_its_shapes():
    assert le.C_SIZES == (16 * MIB - 2048, 16 * MIB, 32 * MIB + 2048) and le.c_sizes(le.GRID_PASS) == list(le.C_SIZES)
    assert le.c_sizes(le.grid_pass(304)) == sorted(set(le.C_SIZES) | {9727 * 2048, 9728 * 2048, 19457 * 2048})
    for size in le.C_SIZES:
        text = le.c_text(size)
        holds_its_shape(text, C_BLOCKS[size], C_HIT_BLOCKS[size])
        ended_in = [text.block_of(int(h)) for h in text.H()]
        if text.blocks > le.GRID_PASS:
            assert le.GRID_PASS - 1 in ended_in and min(b for b in ended_in if b >= le.GRID_PASS) < 2 * le.GRID_PASS, "a hit on either side of 8191 | 8192"
        names = [c[0] for c in le.position_block_calls(size, text=text)]
        assert names == ["C-%d-mis0-b0-a0" % size, "C-%d-mis0-b0-a0-inverted" % size, "C-%d-mis0-b3-a3" % size, "C-%d-mis0-b1048576-a1048576" % size]
        assert le.C_WIDE > text.num_lines
    # the offset of the pointer moves B over the edge
    assert (le.position_blocks(le.C_MIS_SIZE, 0), le.position_blocks(le.C_MIS_SIZE, 15)) == (8192, 8193)
    holds_its_shape(le.c_text(le.C_MIS_SIZE, 0), 8192, [0, 8190, 8191])
    holds_its_shape(le.c_text(le.C_MIS_SIZE, 15), 8193, [0, 8191, 8192])


def test_the_smallest_case_of_family_c(x_handle):
    check(x_handle, le.position_block_calls(le.C_SIZES[0])[0])


# ---------------------------------------------------------------------------------------------------------------- D

def test_family_d_holds_its_shapes():
    assert le.D_LINES == 8192 * 2048 + 2048 * 3 + 5 and le.D_HITS == (3, le.D_LINES - 4)
    assert le.D_WINDOWS == ((0, model.MAX), (model.MAX, 0), (2048 * 8192 + 7, 2), (5, 5))
    (b0, w0, _), (b1, w1, _) = le.place(le.D_HITS[0]), le.place(le.D_HITS[1])
    assert (b0, w0, b1, w1) == (0, 0, 8195, 0) and b1 - b0 > le.SCAN_BLOCK, "more than a block of the block scan apart, in line blocks"
    data = le.far_members()
    newlines = np.flatnonzero(data == le.NL)
    assert newlines.size == le.D_LINES == data.size - 2 and data[-1] == le.NL
    assert np.flatnonzero(data == le.HIT).tolist() == [3, le.D_LINES - 3] and newlines[3] == 4 and newlines[le.D_LINES - 4] == le.D_LINES - 2, "lines 3 and D_LINES - 4 are \"x\""
    assert le.position_blocks(data.size) == 8196 > b1, "a line block per position block: the far member's line block exists"
    inverted = le.far_members(True)
    assert inverted.size == 2 * le.D_LINES < 1 << 31 and np.count_nonzero(inverted == le.NL) == le.D_LINES and inverted[-1] == le.NL
    assert np.flatnonzero(inverted != np.tile(np.asarray([le.HIT, le.NL], dtype=np.uint8), le.D_LINES)).tolist() == [6, 2 * (le.D_LINES - 4)]
    assert [c[0] for c in le.far_member_calls(data=data)] == ["D-b0-amax", "D-bmax-a0", "D-b16777223-a2", "D-b5-a5"]
    assert [c[0] for c in le.far_member_calls(True, data=inverted)] == ["D-b0-amax-inverted", "D-bmax-a0-inverted", "D-b5-a5-inverted"]


def test_the_smallest_case_of_family_d(x_handle):
    want = check(x_handle, le.far_member_calls()[3])
    assert want[4] == (le.D_LINES, 18, 2, 2) and want[2].tolist() == list(range(0, 9)) + list(range(le.D_LINES - 9, le.D_LINES))
