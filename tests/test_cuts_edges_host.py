"""tests/cuts_edges.py without a GPU: every case's claims hold for the grid it was built with; the model equals the byte-by-byte references
(tests/split_ref.py, tests/locate_ref.py, tests/capture_ref.py) on the same families over a few tiles; the full-size cases, built for the 2048
blocks of a 256-CU device, go through PFACX_locatePairsFromHost and PFACX_capturePairsFromHost on a host-only handle and equal the model; and
family E's model, which reads only the special bytes, equals the references on a copy of three tiles."""
import os
import re

import numpy as np
import pytest

from pfac_amd import api
from tests import capture_ref, locate_ref, split_ref
from tests import cuts_edges as ce

GRID = 2048                               # 8 blocks on each of 256 compute units
CSRC = os.path.join(os.path.dirname(os.path.abspath(api.__file__)), "csrc")
T = ce.T


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_launch_shapes_are_the_sources():
    """the three constants the cases are built around, where the kernels and their launches state them"""
    passes, cuts, locate, capture = source("scan_passes.h"), source("scan_cuts.h"), source("scan_locate.hip"), source("scan_capture.hip")
    per_cu, block, step = api.PFACX_GRID_BLOCKS_PER_CU, api.PFACX_PAIRS_MARK_BLOCK, api.PFACX_LOCATE_CARRY_STEP
    assert (per_cu, block, step) == (8, 256, 1024)
    assert re.search(r"inline unsigned int gridFor\(const PFAC_context \*c, size_t items\)\s*\{\s*const size_t cap = gridCap\(c, %d\), blocks = "
                     r"\(items \+ %d\) / %d;" % (per_cu, block - 1, block), passes)
    assert "std::min<size_t>(tiles, gridCap(c, %d))" % per_cu in cuts
    for text, kernel in ((locate, "pfac_locate_mark"), (capture, "pfac_capture_mark")):
        assert "hipLaunchKernelGGL(%s, dim3(gridFor(c, a.numPairs)), dim3(%d)" % (kernel, block) in text
        assert "i = (size_t)blockIdx.x * %d + threadIdx.x; i < a.numPairs; i += (size_t)gridDim.x * %d" % (block, block) in text
    assert "for (size_t base = 0; base < a.tiles; base += %d)" % step in locate and "blockExclusive<%d>(own" % step in locate
    assert ce.a_tiles(GRID) == 2051 and ce.mark_pass(GRID) == 524288


@pytest.fixture(scope="module")
def full():
    """name -> the full-size case, built once"""
    built, make = {}, ce.builders(GRID)

    def get(name):
        if name not in built:
            built[name] = make[name]()
        return built[name]
    return get


@pytest.fixture(scope="module")
def handle():
    h = api.PFAC.createHostOnly()
    h.readPatternFromMemory(ce.PATTERNS)
    yield h
    h.destroy()


@pytest.mark.parametrize("name", ce.NAMES)
def test_claims_of_the_full_size_cases(full, name):
    case = full(name)
    assert case.claims
    ce.check_claims(case)


@pytest.mark.parametrize("grid", [2, 8 * 304, 8 * 64])
def test_claims_for_other_grids(grid):
    """a few tiles for the references; more and fewer compute units than 256"""
    for name, make in ce.builders(grid, small=grid == 2).items():
        if grid != 2 and name[0] in "AB" and name not in ("A0", "B-tail"):
            continue                                                       # the same code with another seed
        ce.check_claims(make())


def some(case, most=240):
    """the indices of a few pairs of a long list: both ends, and a stride between"""
    k = case.pos.size
    return np.arange(k) if k <= most else np.unique(np.concatenate([np.arange(40), np.arange(k - 40, k), np.arange(0, k, k // (most - 80))]))


def against_the_references(case, most=240):
    data = case.text.dense()
    at = some(case, most)
    for cls, flags in case.locate:
        record, column, records = case.want_locate(cls, flags)
        want = locate_ref.locate(data, case.pos, cls, flags)
        assert records == want[2] and np.array_equal(record, want[0]) and np.array_equal(column, want[1]), (case.name, cls, flags)
        assert np.array_equal(ce.model_cuts(case.text, cls, flags, case.dense).astype(np.uint64), split_ref.cuts(data, cls, flags))
    for skip, stop, window, flags in case.capture:
        start, length, _ = case.want_capture(skip, stop, window, flags)
        want = capture_ref.capture(data, None if case.ids is None else case.ids[at], case.pos[at], ce.LENS.tolist(), skip, stop, window, flags)
        assert np.array_equal(start[at], want[0]) and np.array_equal(length[at], want[1]), (case.name, skip, stop, window, flags)


@pytest.mark.parametrize("name", ce.NAMES)
def test_the_model_equals_the_references_over_a_few_tiles(name):
    case = ce.builders(2, small=True)[name]()
    assert case.tiles <= 7
    against_the_references(case)


def slow_by_the_kernel_text(case, call):
    """the slow count again, pair by pair and from the values alone, as scan_capture.hip's header words it: a pair whose b lies behind the bitmap, or
    whose search reaches the bitmap's last bit without an answer while w lies beyond it"""
    skip, stop, window, flags = call
    start, length, slow = case.want_capture(*call)
    count = 0
    for k in np.flatnonzero(start >= 0):
        p = int(case.pos[k])
        b = min(p + (0 if flags & ce.AT_POS else int(ce.LENS[case.ids[k]])), case.n)
        w = case.n if window == 0 else min(case.n, b + window)
        hi = p // T * T + T + ce.R
        s, e = int(start[k]), int(start[k]) + int(length[k])
        left = b < w and (b >= hi or (hi < w and (s >= hi or e >= hi)))    # ... an answer at or behind hi is none of the bitmap's
        assert left == bool(slow[k]), (case.name, call, k)
        count += left
    return count


@pytest.mark.parametrize("window", ce.D_WINDOWS)
def test_the_slow_count_of_family_d(full, window):
    case = full("D-%d" % window)
    by_hand = {0: (3 * 6, 3 * 6), 64: (3 * 2, 0)}[window]                  # three tiles with slow pairs; tile grid + 1 has none: GRID + 3 tiles
    for call, want in zip(case.capture, by_hand):
        assert slow_by_the_kernel_text(case, call) == want == int(np.count_nonzero(case.want_capture(*call)[2]))


def arrays(k):
    return np.full(k + 2, -7, dtype=np.int32), np.full(k + 2, -7, dtype=np.int32)


@pytest.mark.parametrize("name", ce.NAMES)
def test_the_full_size_cases_through_the_host_forms(full, handle, name):
    case = full(name)
    data = case.text.dense()
    before = data.copy() if name == "A0" else None
    k = case.pos.size
    for cls, flags in case.locate:
        rec, col = arrays(k)
        st, records = handle.locatePairsFromHost(data.ctypes.data, case.n, cls, flags, case.pos.ctypes.data, k, rec.ctypes.data + 4, col.ctypes.data + 4)
        want = case.want_locate(cls, flags)
        assert (st, records) == (0, want[2]) and np.array_equal(rec[1:-1], want[0]) and np.array_equal(col[1:-1], want[1]), (case.name, cls, flags)
        assert rec[0] == rec[-1] == col[0] == col[-1] == -7
    for skip, stop, window, flags in case.capture:
        start, length = arrays(k)
        st = handle.capturePairsFromHost(data.ctypes.data, case.n, skip, stop, window, flags, None if flags & ce.AT_POS else case.ids.ctypes.data,
                                         case.pos.ctypes.data, k, start.ctypes.data + 4, length.ctypes.data + 4)
        want = case.want_capture(skip, stop, window, flags)
        assert st == 0 and np.array_equal(start[1:-1], want[0]) and np.array_equal(length[1:-1], want[1]), (case.name, skip, stop, window, flags)
        assert start[0] == start[-1] == length[0] == length[-1] == -7
    assert before is None or np.array_equal(data, before)


@pytest.mark.parametrize("kind", ce.E_KINDS)
def test_family_e_on_a_copy_of_three_tiles(handle, kind):
    """the same special bytes at the same distances from the end: the model from the special bytes alone against the references, byte by byte,
    and against the host forms; the model from the array agrees; and the full-size case says what it claims"""
    case = ce.top_of_range(kind, 3 * T - 1)
    assert not case.dense and case.text.fill == 0 and case.tiles == 3
    against_the_references(case)
    data = case.text.dense()
    k = case.pos.size
    for cls, flags in case.locate:
        assert all(np.array_equal(a, b) for a, b in zip(case.want_locate(cls, flags), ce.model_locate(case.text, case.pos, cls, flags, dense=True)))
    for call in case.capture:
        assert all(np.array_equal(a, b) for a, b in zip(case.want_capture(*call), ce.model_capture(case.text, case.ids, case.pos, *call, dense=True)))
        start, length = arrays(k)
        st = handle.capturePairsFromHost(data.ctypes.data, case.n, *call, None if call[3] & ce.AT_POS else case.ids.ctypes.data, case.pos.ctypes.data,
                                         k, start.ctypes.data + 4, length.ctypes.data + 4)
        assert st == 0 and np.array_equal(start[1:-1], case.want_capture(*call)[0]) and np.array_equal(length[1:-1], case.want_capture(*call)[1])
        slow_by_the_kernel_text(case, call)
    big = ce.top_of_range(kind)
    ce.check_claims(big)
    assert big.n == ce.INT_MAX and big.text.sparse()[0].size < 200, "described by its special bytes only"
    last = (big.n - 1) // T * T
    ends = {call: (big.want_capture(*call)[0].astype(np.int64) + big.want_capture(*call)[1]) for call in big.capture}
    if kind == "open-end":
        at = int(np.flatnonzero(big.pos == last - 50)[0])
        start, length, slow = big.want_capture(b" ", None, 0, ce.AT_POS)
        assert (start[at], start[at] + length[at], bool(slow[at])) == (last - 50, big.n, True), "from the tile in front of the last, slow, to n"
        at = int(np.flatnonzero(big.pos == big.n - 100)[0])
        assert [int(ends[(b" ", None, w, ce.AT_POS)][at]) for w in (99, 100, 101)] == [big.n - 1, big.n, big.n]
    else:
        at = int(np.flatnonzero(big.pos == big.n - 2)[0])
        assert big.want_capture(b" ", None, 0, 0)[0][at] == big.n, "a pattern's length carries b to n"
        assert big.want_locate(None, 0)[0][-3] == big.want_locate(None, 0)[2] - 1 and big.want_locate(None, 0)[1][-3] == 0, "a cut at n - 1"
