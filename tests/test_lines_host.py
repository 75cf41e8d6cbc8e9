"""PFACX_matchLinesFromHost on the CPU platforms (host-only handles: no device needed) against references that use none of the library's
line code (tests/lines_ref.py): the edge cases of the line definition, matches at line ends, INVERT, caseless sets, lineIndex NULL, every
error row of the contract, 1 MiB of the C3 workload against the oracle."""

import ctypes as C
import os

import numpy as np
import pytest

from pfac_amd import api
from tests import lines_ref as ref
from tests.lines_helpers import host_lines, pattern_file
from tests.lines_ref import test_the_two_references_agree_on_the_small_cases  # noqa: F401  (runs here: lines_ref.py is not collected)

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
INVALID, NOT_READY, NOT_EXIST = api.STATUS.INVALID_PARAMETER, api.STATUS.PATTERNS_NOT_READY, api.STATUS.LIB_NOT_EXIST


def host_handle(pf, platform=api.PFAC_PLATFORM_CPU, flags=0):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    h.readPatternFromFileEx(pf, flags)
    return h


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_small_cases_equal_pure_python(workdir, case, invert, platform, pname):
    name, pats, data = case
    h = host_handle(pattern_file(workdir, name, pats), platform)
    try:
        got, after = host_lines(h, data, invert)
        ref.same(got, ref.lines_py(pats, data, invert), f"{name}/{pname}/invert {invert}")
        assert after == data, "the caller's input was modified"
        if invert:
            assert int(np.count_nonzero(got[2] == 0)) == sum(1 for _, line in ref.split_lines(data) if not line), "empty lines are selected under INVERT"
        # the same call without a lineIndex array
        got2, _ = host_lines(h, data, invert, with_index=False)
        assert got2[0] == got[0] and np.array_equal(got2[1], got[1]) and np.array_equal(got2[2], got[2])
    finally:
        h.destroy()


def test_a_line_with_fifty_matches_is_listed_once(workdir):
    name, pats, data = next(c for c in ref.CASES if c[0] == "fifty-matches-in-one-line")
    h = host_handle(pattern_file(workdir, name, pats))
    try:
        (nl, start, length, index), _ = host_lines(h, data, False)
        assert (nl, start.tolist(), length.tolist(), index.tolist()) == (3, [3], [150], [1])
    finally:
        h.destroy()


def test_crlf_lines_count_the_carriage_return(workdir):
    name, pats, data = next(c for c in ref.CASES if c[0] == "crlf")
    h = host_handle(pattern_file(workdir, name, pats))
    try:
        (nl, start, length, index), _ = host_lines(h, data, False)
        assert (nl, start.tolist(), length.tolist(), index.tolist()) == (4, [0, 15], [7, 13], [0, 3])
    finally:
        h.destroy()


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("invert", [False, True])
def test_caseless_set_over_mixed_case_text(workdir, invert, platform, pname):
    name, pats, data = ref.NOCASE_CASES[0]
    h = host_handle(pattern_file(workdir, name, pats), platform, api.PFACX_READ_NOCASE)
    try:
        got, after = host_lines(h, data, invert)
        ref.same(got, ref.lines_py(pats, data, invert, nocase=True), f"{name}/{pname}/invert {invert}")
        assert after == data, "the caller's input was modified"
        assert got[1].size != ref.lines_py(pats, data, invert, nocase=False)[1].size, "the case is meant to matter here"
    finally:
        h.destroy()


def test_every_error_row_of_the_contract(workdir):
    pf = pattern_file(workdir, "errors", ref.PATS)
    data = np.frombuffer(b"ab\ncd\n", dtype=np.uint8).copy()
    n = data.size
    start, length, index = (np.full(n, -7, dtype=np.int32) for _ in range(3))
    I, S, L, X = data.ctypes.data, start.ctypes.data, length.ctypes.data, index.ctypes.data
    h = host_handle(pf)
    try:
        call = lambda *a: h.matchLinesFromHost(*a, check=False)[0]  # noqa: E731
        assert call(I, n, 0, S, L, X, n - 1) == INVALID, "capacity < size"
        assert call(I, 1 << 31, 0, S, L, X, 1 << 31) == INVALID, "size >= 2^31"
        assert call(I, n, 2, S, L, X, n) == INVALID and call(I, n, 0x80000001, S, L, X, n) == INVALID, "an unknown flag bit"
        assert call(None, n, 0, S, L, X, n) == INVALID and call(I, n, 0, None, L, X, n) == INVALID and call(I, n, 0, S, None, X, n) == INVALID
        lib = api.load_library()
        nl, ns = C.c_size_t(5), C.c_size_t(5)
        assert lib.PFACX_matchLinesFromHost(h._h, I, n, 0, S, L, X, n, None, C.byref(ns)) == INVALID
        assert lib.PFACX_matchLinesFromHost(h._h, I, n, 0, S, L, X, n, C.byref(nl), None) == INVALID
        assert np.all(start == -7) and np.all(length == -7) and np.all(index == -7), "a refused call wrote"
        # size == 0: success, 0 lines, 0 selected, nothing touched (whatever the capacity)
        st, a, b = h.matchLinesFromHost(I, 0, api.PFACX_LINES_INVERT, S, L, X, 0, check=False)
        assert (st, a, b) == (0, 0, 0) and np.all(start == -7) and np.all(length == -7) and np.all(index == -7)
        # the device form on a host-only handle, and the gather
        assert h.matchLinesFromDevice(I, n, 0, S, L, X, n, check=False)[0] == NOT_EXIST
        assert h.gatherLinesFromDevice(I, n, S, L, 1, I, n, check=False)[0] == NOT_EXIST
        assert h.gatherLinesFromDevice(I, n, S, L, 0, None, 0, check=False) == (0, 0), "numSelected == 0 is success, d_out may be null"
        # a lineIndex of NULL is no error
        assert call(I, n, 0, S, L, None, n) == 0 and start[0] == 0 and length[0] == 2
    finally:
        h.destroy()
    bare = api.PFAC.createHostOnly()
    try:
        assert bare.matchLinesFromHost(I, n, 0, S, L, X, n, check=False)[0] == NOT_READY
        assert bare.matchLinesFromDevice(I, n, 0, S, L, X, n, check=False)[0] == NOT_READY
    finally:
        bare.destroy()


@pytest.mark.parametrize("platform,pname", PLATFORMS)
def test_one_mib_of_c3_equals_the_oracle(workloads, platform, pname):
    w = workloads["c3"]
    data = w.data[:1 << 20]
    assert int(np.count_nonzero(data == 10)) > 100, "the workload is meant to have lines"
    from oracle import binding as ob
    o = ob.Oracle(w.pattern_file, hashed=False)
    try:
        result = o.match(data)
    finally:
        o.close()
    h = host_handle(w.pattern_file, platform)
    try:
        for invert in (False, True):
            got, after = host_lines(h, data.tobytes(), invert)
            ref.same(got, ref.lines_from_result(result, data, invert), f"c3/{pname}/invert {invert}")
            assert after == data.tobytes()
    finally:
        h.destroy()
