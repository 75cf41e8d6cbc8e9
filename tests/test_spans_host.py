"""PFACX_matchSpansFromHost on the CPU platforms (host-only handles: no device needed) against the two references of tests/spans_ref.py: the
edge cases of the definition against the pure-Python one, seeded random cases against the numpy one over the oracle's vector, coveredBytes,
every status row of the contract."""

import ctypes as C

import numpy as np
import pytest

from pfac_amd import api
from tests import spans_ref as ref
from tests.spans_helpers import RANDOM_SEEDS, host_spans, pattern_file, random_case
from tests.spans_ref import test_the_two_references_agree_on_every_case  # noqa: F401  (runs here: spans_ref.py is not collected)

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
INVALID, NOT_READY, NOT_EXIST = api.STATUS.INVALID_PARAMETER, api.STATUS.PATTERNS_NOT_READY, api.STATUS.LIB_NOT_EXIST


def host_handle(pf, platform=api.PFAC_PLATFORM_CPU, flags=0):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    h.readPatternFromFileEx(pf, flags)
    return h


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_equals_pure_python(workdir, case, platform, pname):
    name, pats, data = case
    nocase = name.startswith("nocase")
    h = host_handle(pattern_file(workdir, name, pats), platform, api.PFACX_READ_NOCASE if nocase else 0)
    try:
        got, covered, after = host_spans(h, data)
        want = ref.spans_py(pats, data, nocase)
        ref.same(got, want, f"{name}/{pname}")
        assert covered == int(want[1].sum()) == int(got[1].sum()), "coveredBytes is the sum of the lengths"
        assert after == data, "the caller's input was modified"
        assert np.all(got[1] >= 1) and np.all(got[0][1:] > got[0][:-1] + got[1][:-1]), "ascending, disjoint, never adjacent"
    finally:
        h.destroy()


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_cases_equal_the_oracle(workdir, seed, platform, pname):
    from oracle import binding as ob
    pats, data = random_case(seed)
    pf = pattern_file(workdir, f"random{seed}", pats)
    o = ob.Oracle(pf, hashed=False)
    try:
        result = o.match(data)
    finally:
        o.close()
    want = ref.spans_from_result(result, ref.pattern_lengths(pats))
    h = host_handle(pf, platform)
    try:
        got, covered, after = host_spans(h, data.tobytes())
        ref.same(got, want, f"seed {seed}/{pname}")
        assert covered == int(want[1].sum())
        assert after == data.tobytes()
    finally:
        h.destroy()


def test_every_status_row_of_the_contract(workdir):
    pf = pattern_file(workdir, "errors", [b"ab", b"cd"])
    data = np.frombuffer(b"ab.cd.", dtype=np.uint8).copy()
    n = data.size
    start, length = (np.full(n, -7, dtype=np.int32) for _ in range(2))
    I, S, L = data.ctypes.data, start.ctypes.data, length.ctypes.data
    lib = api.load_library()
    h = host_handle(pf)
    try:
        call = lambda *a: h.matchSpansFromHost(*a, check=False)[0]  # noqa: E731
        assert call(I, n, S, L, n - 1) == INVALID, "capacity < size"
        assert call(I, 1 << 31, S, L, 1 << 31) == INVALID, "size >= 2^31"
        assert call(None, n, S, L, n) == INVALID and call(I, n, None, L, n) == INVALID and call(I, n, S, None, n) == INVALID
        ns, cb = C.c_size_t(5), C.c_size_t(5)
        assert lib.PFACX_matchSpansFromHost(h._h, I, n, S, L, n, None, C.byref(cb)) == INVALID
        assert lib.PFACX_matchSpansFromHost(h._h, I, n, S, L, n, C.byref(ns), None) == INVALID
        assert np.all(start == -7) and np.all(length == -7) and (ns.value, cb.value) == (5, 5), "a refused call wrote"
        # size == 0: success, both counts 0, nothing touched (whatever the capacity)
        assert lib.PFACX_matchSpansFromHost(h._h, I, 0, S, L, 0, C.byref(ns), C.byref(cb)) == 0 and (ns.value, cb.value) == (0, 0)
        assert np.all(start == -7) and np.all(length == -7)
        # the device form and the redaction on a host-only handle
        assert h.matchSpansFromDevice(I, n, S, L, n, check=False)[0] == NOT_EXIST
        assert h.redactSpansFromDevice(I, n, S, L, 1, 0x2A, I, check=False) == NOT_EXIST
        assert np.all(start == -7) and bytes(data) == b"ab.cd."
        assert h.matchSpansFromHost(I, n, S, L, n) == (0, 2, 4) and start[:2].tolist() == [0, 3] and length[:2].tolist() == [2, 2]
    finally:
        h.destroy()
    bare = api.PFAC.createHostOnly()
    try:
        assert bare.matchSpansFromHost(I, n, S, L, n, check=False)[0] == NOT_READY
        assert bare.matchSpansFromDevice(I, n, S, L, n, check=False)[0] == NOT_READY
    finally:
        bare.destroy()
    ns, cb = C.c_size_t(0), C.c_size_t(0)
    assert lib.PFACX_matchSpansFromHost(None, I, n, S, L, n, C.byref(ns), C.byref(cb)) == api.STATUS.INVALID_HANDLE
    assert lib.PFACX_matchSpansFromDevice(None, I, n, S, L, n, C.byref(ns), C.byref(cb)) == api.STATUS.INVALID_HANDLE
    assert lib.PFACX_redactSpansFromDevice(None, I, n, S, L, 1, 0, I) == api.STATUS.INVALID_HANDLE
