"""PFACX_matchLinesContextFromHost on a CPU platform (host-only handles: no device needed) against the model of tests/linesctx_ref.py,
and the model itself against grep: identity with the plain call at before = after = 0, the word edges of the line bitmap, windows that cross
whole words, clipping at both ends, groups that are apart, touch and overlap, INVERT with nothing behind the last line leaking in, 320 KiB of
short lines, a caseless set, NULL lineIndex / lineTag, the entries beyond capacity, every error row of the contract."""

import ctypes as C

import numpy as np
import pytest

from pfac_amd import api
from tests import linesctx_ref as model
from tests.lines_helpers import host_lines, pattern_file
from tests.linesctx_helpers import POISON, host_context
from tests.linesctx_ref import test_the_model_equals_grep  # noqa: F401  (runs here: linesctx_ref.py is not collected)

INVALID, NOT_READY, NOT_EXIST = api.STATUS.INVALID_PARAMETER, api.STATUS.PATTERNS_NOT_READY, api.STATUS.LIB_NOT_EXIST


def host_handle(pf, platform=api.PFAC_PLATFORM_CPU, flags=0):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    h.readPatternFromFileEx(pf, flags)
    return h


@pytest.fixture(scope="module")
def x_handle(workdir):
    h = host_handle(pattern_file(workdir, "ctx_x", model.X))
    yield h
    h.destroy()


def check(h, pats, data, before, after, invert, what, **kw):
    got = host_context(h, data, before, after, invert)
    model.same(got, model.context_model(pats, data, before, after, invert, **kw), what)
    return got


@pytest.mark.parametrize("invert", [False, True])
def test_no_context_is_the_plain_call(x_handle, invert):
    data = model.tiny_lines(200, [0, 1, 2, 40, 63, 64, 65, 130, 199])
    got = host_context(x_handle, data, 0, 0, invert)
    (nl, start, length, index), _ = host_lines(x_handle, data, invert)
    assert got[4][0] == nl and got[4][1] == got[4][2] == start.size
    assert np.array_equal(got[0], start) and np.array_equal(got[1], length) and np.array_equal(got[2], index)
    assert np.all(got[3] & 1 == 1), "without context every listed line is a member of H"
    model.same(got, model.context_model(model.X, data, 0, 0, invert), f"invert {invert}")


@pytest.mark.parametrize("hit", model.WORD_EDGE_HITS)
def test_single_hits_at_the_word_edges_of_the_line_bitmap(x_handle, hit):
    data = model.tiny_lines(model.WORD_EDGE_LINES, [hit])
    for before in model.WORD_EDGE_WINDOWS:
        for after in model.WORD_EDGE_WINDOWS:
            check(x_handle, model.X, data, before, after, False, f"hit {hit}/before {before}/after {after}")
    check(x_handle, model.X, data, 1, 32, True, f"hit {hit}/inverted")


def test_windows_that_cross_whole_words_and_64_words(x_handle):
    data = model.wave_input()
    for before in model.WAVE_WINDOWS:
        for after in model.WAVE_WINDOWS:
            got = check(x_handle, model.X, data, before, after, False, f"before {before}/after {after}")
            assert got[4][2:] == (1, 1) and got[4][1] == min(before, model.WAVE_HIT) + 1 + min(after, model.WAVE_LINES - 1 - model.WAVE_HIT)


@pytest.mark.parametrize("case", model.SMALL, ids=[c[0] for c in model.SMALL])
def test_clipping_groups_and_invert(workdir, case):
    name, pats, data, before, after, invert = case
    h = host_handle(pattern_file(workdir, "ctx_" + name, pats))
    try:
        check(h, pats, data, before, after, invert, name)
    finally:
        h.destroy()


def test_group_counts_of_windows_apart_touching_and_overlapping(x_handle):
    want = {"windows-one-line-apart": (2, [0] * 9 + [1] * 9), "windows-touching": (1, [0] * 20), "windows-overlapping": (1, [0] * 24)}
    for name, pats, data, before, after, invert in model.SMALL:
        if name in want:
            got = host_context(x_handle, data, before, after, invert)
            assert (got[4][3], (got[3] >> 1).tolist()) == want[name], name
            assert got[2][(got[3] & 1) == 1].tolist() == [10, 20], name


@pytest.mark.parametrize("num", model.INVERT_LINE_COUNTS)
def test_inverted_with_every_line_matching_selects_nothing(x_handle, num):
    data = model.every_line_matches(num)
    for before, after in ((0, 0), (1, 1), (33, 2), (model.MAX, model.MAX)):
        got = host_context(x_handle, data, before, after, True)
        assert got[4] == (num, 0, 0, 0), f"{num} lines/before {before}/after {after}: {got[4]}"
    # one line that does not match, the last: its window reaches back, nothing behind numLines reaches in
    data = data[:-2] + b"z\n"
    check(x_handle, model.X, data, 2, model.MAX, True, f"{num} lines, the last does not match")


@pytest.mark.parametrize("window", model.FOLD_WINDOWS)
def test_320_kib_of_short_lines(x_handle, window):
    data = model.fold_input()
    got = check(x_handle, model.X, data, window, window, False, f"window {window}")
    assert got[4][2:] == (6, 2), "six hits, a group at each end"


def test_caseless_set(workdir):
    pats, data, before, after = model.NOCASE
    h = host_handle(pattern_file(workdir, "ctx_nocase", pats), flags=api.PFACX_READ_NOCASE)
    try:
        got = check(h, pats, data, before, after, False, "nocase", nocase=True)
        assert got[4][2] == 2 and model.context_model(pats, data, before, after, False, nocase=False)[4][2] == 0, "only the folded input matches"
        check(h, pats, data, 0, 1, True, "nocase/inverted", nocase=True)
    finally:
        h.destroy()


def test_null_index_and_null_tag(x_handle):
    data = model.tiny_lines(model.WORD_EDGE_LINES, [33, 64])
    full = host_context(x_handle, data, 2, 31, False)
    for with_index, with_tag in ((False, True), (True, False), (False, False)):
        got = host_context(x_handle, data, 2, 31, False, with_index=with_index, with_tag=with_tag)
        assert got[4] == full[4] and np.array_equal(got[0], full[0]) and np.array_equal(got[1], full[1])
        assert not with_index or np.array_equal(got[2], full[2])
        assert not with_tag or np.array_equal(got[3], full[3])


def test_cpu_omp_platform(workdir):
    h = host_handle(pattern_file(workdir, "ctx_omp", model.X), api.PFAC_PLATFORM_CPU_OMP)
    try:
        check(h, model.X, model.tiny_lines(model.WORD_EDGE_LINES, [31, 64]), 3, 2, False, "cpu-omp")
    finally:
        h.destroy()


def test_every_error_row_of_the_contract(workdir):
    data = np.frombuffer(b"x\ncd\n", dtype=np.uint8).copy()
    n = data.size
    arrays = [np.full(n, POISON, dtype=np.int32) for _ in range(4)]
    I, (S, L, X, T) = data.ctypes.data, (a.ctypes.data for a in arrays)
    untouched = lambda: all(np.all(a == POISON) for a in arrays)  # noqa: E731
    h = host_handle(pattern_file(workdir, "ctx_errors", model.X))
    try:
        call = lambda *a: h.matchLinesContextFromHost(*a, check=False)[0]  # noqa: E731
        assert call(I, n, 0, 1, 1, S, L, X, T, n - 1) == INVALID, "capacity < size"
        assert call(I, 1 << 31, 0, 1, 1, S, L, X, T, 1 << 31) == INVALID, "size >= 2^31"
        assert call(I, n, 2, 1, 1, S, L, X, T, n) == INVALID and call(I, n, 0x80000001, 1, 1, S, L, X, T, n) == INVALID, "an unknown flag bit"
        assert call(None, n, 0, 1, 1, S, L, X, T, n) == INVALID and call(I, n, 0, 1, 1, None, L, X, T, n) == INVALID
        assert call(I, n, 0, 1, 1, S, None, X, T, n) == INVALID
        lib = api.load_library()
        for missing in range(4):
            counts = [C.c_size_t(5) for _ in range(4)]
            refs = [None if k == missing else C.byref(c) for k, c in enumerate(counts)]
            assert lib.PFACX_matchLinesContextFromHost(h._h, I, n, 0, 1, 1, S, L, X, T, n, *refs) == INVALID, f"count pointer {missing} is null"
            assert lib.PFACX_matchLinesContextFromDevice(h._h, I, n, 0, 1, 1, S, L, X, T, n, *refs) == INVALID
        assert untouched(), "a refused call wrote"
        # size == 0: success, all four counts 0, nothing touched (whatever the capacity)
        assert h.matchLinesContextFromHost(I, 0, api.PFACX_LINES_INVERT, 3, 3, S, L, X, T, 0, check=False) == (0, 0, 0, 0, 0) and untouched()
        # the device form on a host-only handle
        assert h.matchLinesContextFromDevice(I, n, 0, 1, 1, S, L, X, T, n, check=False)[0] == NOT_EXIST and untouched()
        # NULL lineIndex and lineTag are no errors
        assert call(I, n, 0, 0, 1, S, L, None, None, n) == 0 and (arrays[0][:2].tolist(), arrays[1][:2].tolist()) == ([0, 2], [1, 2])
    finally:
        h.destroy()
    bare = api.PFAC.createHostOnly()
    try:
        assert bare.matchLinesContextFromHost(I, n, 0, 1, 1, S, L, X, T, n, check=False)[0] == NOT_READY
        assert bare.matchLinesContextFromDevice(I, n, 0, 1, 1, S, L, X, T, n, check=False)[0] == NOT_READY
    finally:
        bare.destroy()


def test_the_array_form_of_the_binding(x_handle):
    data = model.tiny_lines(20, [5])
    got = x_handle.match_lines_context_host_array(np.frombuffer(data, dtype=np.uint8), before=1, after=2)
    model.same(got, model.context_model(model.X, data, 1, 2), "match_lines_context_host_array")
