"""PFACX_matchLinesContextFromDevice where the context stage of scan_lines.hip takes another path: the cases of tests/linesctx_edges.py through
linesctx_helpers.device_context (poisoned arrays, guard entries behind capacity, the input unchanged), start, len, index, tag and the four counts
compared with linesctx_ref.context_model(..., H=H).  tests/test_linesctx_edges_host.py pins the shape of every case and runs the host form.

    A, B   line counts on both sides of a multiple of a line block, hits and group seams on both sides of lines 2047 | 2048 and 4095 | 4096
    C      8192, 8193 and 16386 position blocks: the second and third trip of the wave-per-block loops, the second and third block of the
           stage's two block scans (here all their values lie in the first 150 line blocks; the back-to-front column has them at its far end)
    D      members in line blocks 0 and 8195: every line block between them learns of the member behind it, and of the one in front, only
           through what pfac_block_scan folds in front of a block; 16.8 million lines

One pass of the grid is 4 x 8 blocks per compute unit (8192 on 256); the count is read from torch, and a device with another count gets the
sizes of family C for its own pass on top.  The inverted form of D (33.5 MB) takes the windows of linesctx_edges.D_INVERTED_WINDOWS: without
the one that only moves a window's lower end.

Wall time on an MI355X, one run, model and copies included: family C 0.36 s (B = 8192), 0.36 s (8193, with the two plain calls), 0.56 s
(16386), 0.26 s at 15 mod 16; family D 1.13 s for its four windows, of which the model takes 0.8 s, and 1.00 s for the three windows of the inverted
form; the 1030 cases of A and B 4 s together."""
import time

import numpy as np
import pytest
import torch                              # before the library loads its HIP runtime, as in every GPU test module

from tests import linesctx_edges as le  # noqa: E402
from tests import linesctx_ref as model  # noqa: E402
from tests.lines_helpers import pattern_file  # noqa: E402
from tests.linesctx_helpers import device_context  # noqa: E402
from tests.test_lines_gpu import device_lines, gpu_handle  # noqa: E402

pytestmark = pytest.mark.gpu

A = le.by_name(le.line_block_edges())
B = le.by_name(le.groups_across_edges())


@pytest.fixture(scope="module")
def x_handle(workdir):
    h = gpu_handle(pattern_file(workdir, "ctx_edges_x", model.X))
    yield h
    h.destroy()


@pytest.fixture(scope="module")
def grid(x_handle):
    """the blocks of one trip of the wave-per-block kernels on this device"""
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert cus == int(x_handle.info().multiProcessorCount), "the library and torch see the same device"
    return le.grid_pass(cus)


def check(h, case, mis=0):
    name, pats, data, before, after, invert, H = case
    t0 = time.perf_counter()
    got, kept = device_context(h, data, before, after, invert, in_offset=mis, keep=True)
    assert (kept[0].data_ptr() + kept[1]) % 16 == mis, "the pointer is as far off a 16-byte boundary as the case says"
    t1 = time.perf_counter()
    want = model.context_model(pats, data, before, after, invert, H=H)
    model.same(got, want, name)
    if len(data) > 1 << 20:
        print("%s: the call and its copies %.2f s, the model %.2f s, %d lines listed" % (name, t1 - t0, time.perf_counter() - t1, got[4][1]))
    return got


@pytest.mark.parametrize("name", sorted(A))
def test_line_block_edges(x_handle, name):
    """numLines on and around 2048 and 4096: the line block behind the last line is "no line here", the word in front of it full; one hit at
    the last bits of a line block or the first of the next, its window clipped at both ends of the lines; under INVERT every other line"""
    check(x_handle, A[name])


@pytest.mark.parametrize("name", sorted(B))
def test_groups_across_a_line_block_edge(x_handle, name):
    """group numbers and member bits where the seam between two windows, or none, lies at a line block's first word"""
    got = check(x_handle, B[name])
    by_hand = le.b_by_hand(name)
    if by_hand is not None:
        groups, listed, members = by_hand
        assert ((got[3] >> 1).tolist(), got[2].tolist(), got[2][(got[3] & 1) == 1].tolist()) == (groups, listed, members)
        assert got[4] == (le.B_LINES, len(listed), len(members), groups[-1] + 1)


def position_blocks(h, size, mis=0, grid=le.GRID_PASS):
    """family C over one input: every window of C_WINDOWS"""
    text = le.c_text(size, mis, grid)
    for case in le.position_block_calls(size, mis, grid, text):
        got = check(h, case, mis)
        before, invert = case[3], case[5]
        hits = len(text.hits)
        if invert:
            assert got[4][:3] == (text.num_lines, text.num_lines - hits, text.num_lines - hits) and 1 < got[4][3] <= hits, "the hits cut the other lines into groups"
        elif before == le.C_WIDE:
            assert got[4] == (text.num_lines, text.num_lines, hits, 1)
        else:
            assert got[4][0] == text.num_lines and got[4][2] == hits
    return text


@pytest.mark.parametrize("size", le.C_SIZES)
def test_position_blocks_on_and_past_one_pass_of_the_grid(x_handle, size):
    """B = 8192, 8193, 16386: hits in the last block of the first trip and the first of the second; the last line's newline alone in the last
    block.  At 8193 the plain call on the same handle, before and behind the context calls: the context stage has a scratch of its own"""
    around = le.position_blocks(size) == le.GRID_PASS + 1
    if around:
        text = le.c_text(size)
        plain = device_lines(x_handle, text.data, False)
        want = model.context_model(model.X, text.data, 0, 0, H=text.H())
        assert plain[0] == want[4][0] and all(np.array_equal(g, w) for g, w in zip(plain[1:], want[:3])), "the plain call in front"
    position_blocks(x_handle, size)
    if around:
        again = device_lines(x_handle, text.data, False)
        assert again[0] == plain[0] and all(np.array_equal(g, w) for g, w in zip(again[1:], plain[1:])), "the plain call is what it was"


def test_an_offset_of_the_pointer_moves_the_position_blocks_over_the_edge(x_handle):
    """16 MiB - 8 bytes at 15 mod 16: B = 8193 where the aligned pointer has 8192, the hits' lines end in other blocks"""
    assert (le.position_blocks(le.C_MIS_SIZE, 0), le.position_blocks(le.C_MIS_SIZE, 15)) == (le.GRID_PASS, le.GRID_PASS + 1)
    position_blocks(x_handle, le.C_MIS_SIZE, mis=15)


def test_position_blocks_past_one_pass_of_this_device(x_handle, grid):
    """the sizes of family C are cut for 256 compute units.  On another device: the same family for its own pass, so that the second trip runs
    here too"""
    extra = [size for size in le.c_sizes(grid) if size not in le.C_SIZES]
    if not extra:
        assert [le.position_blocks(size) for size in le.C_SIZES] == [grid, grid + 1, 2 * grid + 2], "4 x 8 blocks per compute unit: the sizes pass them once and twice"
    for size in extra:
        position_blocks(x_handle, size, grid=grid)
    assert any(le.position_blocks(size) > 2 * grid for size in le.c_sizes(grid))


def far_members(h, invert):
    data = le.far_members(invert)
    lines = le.D_LINES
    by_hand = {(0, model.MAX): (lines - 3, 1), (model.MAX, 0): (lines - 3, 1), (le.BLOCK * le.SCAN_BLOCK + 7, 2): (6 + lines - 1 - 6138, 2), (5, 5): (18, 2)}
    for case in le.far_member_calls(invert, data):
        got = check(h, case)
        assert got[4] == (lines, by_hand[case[3:5]][0], 2, by_hand[case[3:5]][1]), case[0]
        assert got[2][(got[3] & 1) == 1].tolist() == list(le.D_HITS), case[0]


def test_members_more_than_a_block_of_the_block_scan_apart(x_handle):
    """line blocks 0 and 8195 hold the two members: (0, MAX) and (MAX, 0) list every line between them from the member 8192 and more line
    blocks in front, or behind -- the folded front of both columns of pfac_block_scan<max, max> --, (5, 5) keeps two groups of nine lines"""
    far_members(x_handle, False)


def test_members_more_than_a_block_of_the_block_scan_apart_inverted(x_handle):
    """"x" lines but for two: the same H from pfac_lines_members' INVERT, 16.8 million pairs in the scan's list"""
    far_members(x_handle, True)
