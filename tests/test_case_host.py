"""PFACX_caseOpen / PFACX_caseMatchFromHost on the CPU platforms (host-only handles: no device needed) against the references of tests/case_ref.py:
every case of the table in both modes -- the three-variant class, duplicates of each kind, chains whose longest member fails, the compare edges, the
fold edges --, maxMatchesPerPosition, every capacity from 0 to the list's length, every refusal of the open call and every status row of the match
calls, the stale object, the two reductions (all caseless: the handle's own lists; all sensitive: a plain handle of the unfolded text), the CaseSet
wrapper."""

import ctypes as C

import numpy as np
import pytest

from pfac_amd import api
from tests import case_ref as ref
from tests.case_ref import test_the_references_agree_on_every_case  # noqa: F401  (runs here: case_ref.py is not collected)

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
INVALID, NOT_READY, NOT_EXIST, TRUNCATED = (api.STATUS.INVALID_PARAMETER, api.STATUS.PATTERNS_NOT_READY, api.STATUS.LIB_NOT_EXIST,
                                            api.STATUS.OUTPUT_TRUNCATED)
ALL = api.PFACX_CASE_ALL
NOCASE = api.PFACX_READ_NOCASE
GUARD = 16


def text_of(pats):
    return b"".join(bytes(p) + b"\n" for p in pats)


def host_handle(pats, platform=api.PFAC_PLATFORM_CPU, flags=NOCASE):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    h.readPatternFromMemoryEx(text_of(pats), flags)
    return h


def host_case(cs, data, flags, capacity=None):
    """match_host into poisoned arrays of `capacity` entries (default: the full length, asked for first) with GUARD poisoned ints on both sides
    -> (status, (pos, ids) of the pairs written, the full length); nothing outside the written pairs may change, nor the input"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    n = buf.size
    if capacity is None:
        st, capacity = cs.match_host(buf.ctypes.data, n, flags, None, None, 0, check=False)
        assert st in (0, TRUNCATED) and (st == TRUNCATED) == (capacity > 0)
    ids, pos = (np.full(GUARD + capacity + GUARD, -7, dtype=np.int32) for _ in range(2))
    st, total = cs.match_host(buf.ctypes.data, n, flags, ids.ctypes.data + 4 * GUARD, pos.ctypes.data + 4 * GUARD, capacity, check=False)
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > capacity)
    k = min(total, capacity)
    for a in (ids, pos):
        assert np.all(a[:GUARD] == -7) and np.all(a[GUARD + capacity:] == -7), "wrote outside the arrays"
        assert np.all(a[GUARD + k:GUARD + capacity] == -7), "wrote behind the list"
    assert buf.tobytes() == bytes(data), "the caller's input was modified"
    return st, (pos[GUARD:GUARD + k].copy(), ids[GUARD:GUARD + k].copy()), total


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_equals_the_references(case, platform, pname):
    name, pats, sens, data = case
    h = host_handle(pats, platform)
    try:
        with h.caseOpen(text_of(pats), ref.flags_by_id(sens)) as cs:
            assert cs.status == 0 and cs.max_matches_per_position == ref.max_per_position(pats, sens)
            for flags in (0, ALL):
                want = ref.case_brute(pats, sens, data, bool(flags))
                st, got, total = host_case(cs, data, flags)
                assert st == 0 and total == want[0].size
                ref.same(got, want, f"{name}/{pname}/flags {flags}")
                if name in ref.WANT:
                    ids, pos = ref.WANT[name][flags]
                    ref.same(got, (pos, ids), f"{name}/{pname}/flags {flags}: against the list worked out by hand")
                ref.same(cs.match_host_array(np.frombuffer(data, dtype=np.uint8), bool(flags)), want, f"{name}/match_host_array")
    finally:
        h.destroy()


def test_every_capacity_from_zero_to_the_length(workdir):
    name, pats, sens, data = ref.CASES[6]                       # the three-deep chain: ALL is longer than the list
    h = host_handle(pats)
    try:
        with h.caseOpen(text_of(pats), ref.flags_by_id(sens)) as cs:
            for flags in (0, ALL):
                want = ref.case_brute(pats, sens, data, bool(flags))
                total = int(want[0].size)
                assert total > 2
                for cap in (0, 1, total - 1, total, total + 3):
                    st, got, n = host_case(cs, data, flags, capacity=cap)
                    assert (st, n) == (TRUNCATED if cap < total else 0, total)
                    ref.same(got, (want[0][:cap], want[1][:cap]), f"flags {flags}/capacity {cap}")
    finally:
        h.destroy()


def test_the_open_call_refuses_what_is_not_the_handles_set():
    pats = [b"GET", b"get", b"Host: "]
    text, flags = text_of(pats), ref.flags_by_id([1, 1, 0])
    lib = api.load_library()
    h = host_handle(pats)
    plain = host_handle(pats, flags=0)
    try:
        refused = lambda handle, t, f: handle.caseOpen(t, f, check=False)  # noqa: E731
        assert refused(plain, text, flags).status == INVALID, "the handle is not caseless"
        assert refused(h, text_of(pats[:2]), flags).status == INVALID and refused(h, text + b"more\n", np.zeros(8, np.uint8)).status == INVALID, "another F"
        assert refused(h, text_of([b"GET", b"gex", b"Host: "]), flags).status == INVALID, "one folded line differs"
        assert refused(h, text_of([b"GET", b"ge", b"Host: "]), flags).status == INVALID, "one line is shorter"
        assert refused(h, text_of([b"get", b"Host: ", b"GET"]), flags).status == INVALID, "the same lines in another order"
        assert refused(h, text, flags[:3]).status == INVALID, "numFlags < F + 1"
        assert refused(h, b"GET\n\nget\nHost: \n", flags).status == INVALID, "a blank line: the reader's own refusal"
        s, most = C.c_void_p(), C.c_int(0)
        assert lib.PFACX_caseOpen(h._h, None, 0, 0, flags.ctypes.data, 4, C.byref(s), C.byref(most)) == INVALID
        assert lib.PFACX_caseOpen(h._h, text, len(text), 0, None, 4, C.byref(s), C.byref(most)) == INVALID
        assert lib.PFACX_caseOpen(h._h, text, len(text), 0, flags.ctypes.data, 4, None, C.byref(most)) == INVALID
        assert lib.PFACX_caseOpen(None, text, len(text), 0, flags.ctypes.data, 4, C.byref(s), C.byref(most)) == api.STATUS.INVALID_HANDLE
        assert not s.value
        assert lib.PFACX_caseOpen(h._h, text, len(text), 0, flags.ctypes.data, 4, C.byref(s), None) == 0, "maxMatchesPerPosition may be null"
        assert lib.PFACX_caseClose(s) == 0 and lib.PFACX_caseClose(None) == api.STATUS.INVALID_HANDLE
        # the case of the text is free, the STRIP_CR bit of the read is honoured, a set bit of NOCASE is ignored
        with h.caseOpen(text_of([b"get", b"GET", b"hOST: "]), flags) as cs:
            ref.same(cs.match_host_array(np.frombuffer(b"GET get host: ", dtype=np.uint8), True), ref.case_brute([b"get", b"GET", b"hOST: "], [1, 1, 0], b"GET get host: ", True), "another casing")
        crlf = api.PFAC.createHostOnly()
        try:
            crlf.readPatternFromMemoryEx(b"GET\r\nHost: \r\n", NOCASE | api.PFACX_READ_STRIP_CR)
            assert crlf.caseOpen(b"GET\r\nHost: \r\n", [0, 1, 0], check=False).status == INVALID, "the lines keep their '\\r' without the bit"
            with crlf.caseOpen(b"GET\r\nHost: \r\n", [0, 1, 0], api.PFACX_READ_STRIP_CR | NOCASE) as cs:
                assert cs.match_host_array(np.frombuffer(b"get GET host: ", dtype=np.uint8))[1].tolist() == [1, 2]
        finally:
            crlf.destroy()
        bare = api.PFAC.createHostOnly()
        try:
            assert bare.caseOpen(text, flags, check=False).status == NOT_READY
        finally:
            bare.destroy()
    finally:
        h.destroy()
        plain.destroy()


def test_every_status_row_of_the_match_calls_and_the_stale_object():
    pats = [b"Ab", b"cd"]
    data = np.frombuffer(b"Ab.cd.ab", dtype=np.uint8).copy()
    n = data.size
    ids, pos = (np.full(n + GUARD, -7, dtype=np.int32) for _ in range(2))
    I, A, P = data.ctypes.data, ids.ctypes.data, pos.ctypes.data
    lib = api.load_library()
    h = host_handle(pats)
    try:
        cs = h.caseOpen(text_of(pats), [0, 1, 0])
        call = lambda *a: cs.match_host(*a, check=False)[0]  # noqa: E731
        pairs = lambda *a: cs.pairs_device(*a, check=False)[0]  # noqa: E731
        assert call(I, 1 << 31, 0, A, P, n) == INVALID, "size >= 2^31"
        assert call(I, n, 2, A, P, n) == INVALID and call(I, n, 0x80000000, A, P, n) == INVALID, "an unknown flag bit"
        assert call(None, n, 0, A, P, n) == INVALID and call(I, n, 0, None, P, n) == INVALID and call(I, n, 0, A, None, n) == INVALID
        assert lib.PFACX_caseMatchFromHost(cs._c, I, n, 0, A, P, n, None) == INVALID
        # the device forms on a host-only handle, and behind their argument checks
        assert cs.match_device(I, n, 0, A, P, n, check=False)[0] == NOT_EXIST
        assert pairs(I, n, 0, A, P, 2, A + 64, P + 64, 2) == NOT_EXIST and pairs(I, n, 0, A, P, 2, None, None, 0) == NOT_EXIST
        assert cs.match_device(I, n, 0, A, P, n - 1, check=False)[0] == INVALID, "the device form: capacity < size"
        assert cs.match_device(I, n, 4, A, P, n, check=False)[0] == INVALID and cs.match_device(I, n, 0, None, P, n, check=False)[0] == INVALID
        assert pairs(I, n, 2, A, P, 2, A + 64, P + 64, 2) == INVALID and pairs(I, 1 << 31, 0, A, P, 2, A + 64, P + 64, 2) == INVALID
        assert pairs(None, n, 0, A, P, 2, A + 64, P + 64, 2) == INVALID and pairs(I, n, 0, None, P, 2, A + 64, P + 64, 2) == INVALID
        assert pairs(I, n, 0, A, P, 2, None, P + 64, 2) == INVALID and pairs(I, n, 0, A, P, 1 << 31, A + 64, P + 64, 2) == INVALID
        for out_ids, out_pos in ((A, P + 64), (A + 64, P), (A + 4, P + 64), (P + 4, A + 64), (A - 4, P + 64)):
            assert pairs(I, n, 0, A, P, 2, out_ids, out_pos, 2) == INVALID, "output arrays that overlap the pair arrays"
        total = C.c_size_t(0)
        assert lib.PFACX_caseMatchFromHost(None, I, n, 0, A, P, n, C.byref(total)) == api.STATUS.INVALID_HANDLE
        assert lib.PFACX_caseMatchFromDevice(None, I, n, 0, A, P, n, C.byref(total)) == api.STATUS.INVALID_HANDLE
        assert lib.PFACX_casePairsFromDevice(None, I, n, 0, A, P, 2, A + 64, P + 64, 2, C.byref(total)) == api.STATUS.INVALID_HANDLE
        assert np.all(ids == -7) and np.all(pos == -7) and bytes(data) == b"Ab.cd.ab", "a refused call wrote"
        total.value = 5
        assert lib.PFACX_caseMatchFromHost(cs._c, I, 0, 0, None, None, 0, C.byref(total)) == 0 and total.value == 0, "size 0"
        st, found = cs.match_host(I, n, 0, A, P, n)
        assert (st, found) == (0, 2) and ids[:2].tolist() == [1, 2] and pos[:2].tolist() == [0, 3], "the object is usable after refused calls"
        # the GPU platform of a host-only handle says so loudly
        h.setPlatform(api.PFAC_PLATFORM_GPU)
        assert call(I, n, 0, A, P, n) == NOT_EXIST
        h.setPlatform(api.PFAC_PLATFORM_CPU)
        # another set, even the same text: the object is stale and only close works
        h.readPatternFromMemoryEx(text_of(pats), NOCASE)
        assert call(I, n, 0, A, P, n) == INVALID and call(I, 0, 0, A, P, n) == INVALID
        assert cs.match_device(I, n, 0, A, P, n, check=False)[0] in (INVALID, NOT_EXIST) and pairs(I, n, 0, A, P, 2, A + 64, P + 64, 2) in (INVALID, NOT_EXIST)
        assert cs.close() == 0
        fresh = h.caseOpen(text_of(pats), [0, 1, 0])
        assert fresh.match_host(I, n, 0, A, P, n) == (0, 2)
        # `fresh` stays open: PFAC_destroy closes what is left open
    finally:
        h.destroy()


@pytest.mark.parametrize("platform,pname", PLATFORMS)
def test_all_caseless_flags_give_the_handles_own_lists(platform, pname):
    pats = [b"Needle", b"NEE", b"needles", b"dle", b"nee", b"D"]
    data = (b"a NEEDLES, nEe-dLe needle NeEdLeS d " * 30)
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    h = host_handle(pats, platform)
    try:
        with h.caseOpen(text_of(pats), np.zeros(len(pats) + 1, dtype=np.uint8)) as cs:
            assert cs.max_matches_per_position == h.info().maxMatchesPerPosition
            ref.same(host_case(cs, data, ALL)[1], h.match_all_host_array(buf), "ALL with no sensitive line is the all-match list")
            ids, pos = (np.full(buf.size, -7, dtype=np.int32) for _ in range(2))
            _, n = h.matchFromHostReduce(buf.ctypes.data, buf.size, ids.ctypes.data, pos.ctypes.data)
            st, got, total = host_case(cs, data, 0)
            assert total == n
            ref.same(got, (pos[:n], ids[:n]), "the list with no sensitive line is the list of PFAC_matchFromHostReduce")
    finally:
        h.destroy()


@pytest.mark.parametrize("platform,pname", PLATFORMS)
def test_all_sensitive_flags_give_the_lists_of_a_plain_handle(platform, pname):
    pats = [b"Needle", b"NEE", b"needles", b"dLe", b"nee", b"needle", b"Nee"]
    data = (b"a NEEDLES, nEe-dLe needle Needles NeEdLeS Nee nee " * 30)
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    h = host_handle(pats, platform)
    plain = host_handle(pats, platform, flags=0)
    try:
        with h.caseOpen(text_of(pats), np.ones(len(pats) + 1, dtype=np.uint8)) as cs:
            ref.same(host_case(cs, data, ALL)[1], plain.match_all_host_array(buf), "ALL with every line sensitive is the plain all-match list")
            ids, pos = (np.full(buf.size, -7, dtype=np.int32) for _ in range(2))
            _, n = plain.matchFromHostReduce(buf.ctypes.data, buf.size, ids.ctypes.data, pos.ctypes.data)
            st, got, total = host_case(cs, data, 0)
            assert total == n
            ref.same(got, (pos[:n], ids[:n]), "the list with every line sensitive is the plain list of PFAC_matchFromHostReduce")
    finally:
        h.destroy()
        plain.destroy()


def test_the_wrapper_closes_itself_and_reports_its_statuses():
    name, pats, sens, data = ref.CASES[0]
    h = host_handle(pats)
    try:
        with h.caseOpen(text_of(pats), ref.flags_by_id(sens)) as cs:
            assert isinstance(cs, api.CaseSet) and cs.status == 0 and cs.max_matches_per_position == 3
            pos, ids = cs.match_host_array(np.frombuffer(data, dtype=np.uint8), all_matches=True)
            assert ids.tolist() == [3, 1, 3, 2, 3, 3] and pos.tolist() == [0, 0, 4, 4, 8, 12]
            assert cs.match_host_array(np.zeros(0, dtype=np.uint8))[0].size == 0
        assert not cs._c, "the context manager closed it"
        with pytest.raises(api.PFACError):
            h.caseOpen(text_of(pats[:1]), [0, 1])
        cs = h.caseOpen(text_of(pats), ref.flags_by_id(sens))
        assert cs.close() == 0
        assert h.info().deviceTableBytes == 0, "a host-only handle holds nothing on a device"
    finally:
        h.destroy()
