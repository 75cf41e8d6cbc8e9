"""PFACX_countFromHost on the CPU platforms (host-only handles: no device needed) against the two references of tests/count_ref.py: the edge cases
of the definition against the pure-Python one, seeded random cases against the numpy one over the oracle's vector, the total against
PFACX_matchAllFromHost, PFACX_COUNT_LONGEST against the full result, PFACX_COUNT_ACCUMULATE, the guard words around counts[0, F], every status row
of the contract."""

import ctypes as C

import numpy as np
import pytest

from pfac_amd import api
from tests import allmatch_ref as am
from tests import count_ref as ref
from tests.count_ref import test_the_two_references_agree_on_every_case  # noqa: F401  (runs here: count_ref.py is not collected)
from tests.spans_helpers import RANDOM_SEEDS, pattern_file, random_case

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
INVALID, NOT_READY, NOT_EXIST = api.STATUS.INVALID_PARAMETER, api.STATUS.PATTERNS_NOT_READY, api.STATUS.LIB_NOT_EXIST
LONGEST, ACCUMULATE = api.PFACX_COUNT_LONGEST, api.PFACX_COUNT_ACCUMULATE
GUARD = 8
POISON = 0xDEADBEEFDEADBEEF


def host_handle(pf, platform=api.PFAC_PLATFORM_CPU, flags=0):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    h.readPatternFromFileEx(pf, flags)
    return h


def host_counts(h, data, flags=0, preset=None):
    """countFromHost into counts[0, F] with GUARD poisoned words on both sides -> (counts, total); the guards and the input must stay as they were"""
    f = int(h.info().numOfPatterns)
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    arr = np.full(GUARD + f + 1 + GUARD, POISON, dtype=np.uint64)
    if preset is not None:
        arr[GUARD:GUARD + f + 1] = preset
    st, total = h.countFromHost(buf.ctypes.data if buf.size else arr.ctypes.data, buf.size, flags, arr.ctypes.data + 8 * GUARD, f + 1)
    assert st == 0
    assert np.all(arr[:GUARD] == POISON) and np.all(arr[GUARD + f + 1:] == POISON), "wrote outside counts[0, F]"
    assert buf.tobytes() == bytes(data), "the caller's input was modified"
    return arr[GUARD:GUARD + f + 1].copy(), total


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_equals_pure_python(workdir, case, platform, pname):
    name, pats, data = case
    nocase = name.startswith("nocase")
    h = host_handle(pattern_file(workdir, "count_" + name, pats), platform, api.PFACX_READ_NOCASE if nocase else 0)
    try:
        for longest in (False, True):
            want = ref.counts_py(pats, data, nocase, longest)
            got, total = host_counts(h, data, LONGEST if longest else 0)
            ref.same(got, want, f"{name}/{pname}/longest {longest}")
            assert total == int(want.sum()), "the total is what the call added"
        got, total = h.count_host_array(np.frombuffer(data, dtype=np.uint8))
        ref.same(got, ref.counts_py(pats, data, nocase), f"{name}/count_host_array")
    finally:
        h.destroy()


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_cases_equal_the_oracle(workdir, seed, platform, pname):
    from oracle import binding as ob
    pats, data = random_case(seed)
    pf = pattern_file(workdir, f"count_random{seed}", pats)
    o = ob.Oracle(pf, hashed=False)
    try:
        result = o.match(data)
    finally:
        o.close()
    prefix, chain, most = am.prefix_table(pats)
    h = host_handle(pf, platform)
    try:
        assert np.array_equal(h.table(api.PFACX_TABLE_PREFIX_PATTERN), prefix)
        for longest in (False, True):
            got, total = host_counts(h, data.tobytes(), LONGEST if longest else 0)
            ref.same(got, ref.counts_from_result(result, (prefix, chain), longest), f"seed {seed}/{pname}/longest {longest}")
            assert total == ref.total_of(result, (prefix, chain), longest)
        # the total is the length of the all-match list; the longest counts are the bincount of the full result
        cap = data.size * most
        ids, pos = (np.zeros(cap, dtype=np.int32) for _ in range(2))
        buf = data.copy()
        _, n = h.matchAllFromHost(buf.ctypes.data, buf.size, ids.ctypes.data, pos.ctypes.data, cap)
        got, total = host_counts(h, data.tobytes())
        assert total == n
        ref.same(got, np.bincount(ids[:n], minlength=len(pats) + 1), f"seed {seed}/{pname}/bincount of the all-match list")
        full = h.match_host_array(data)
        ref.same(host_counts(h, data.tobytes(), LONGEST)[0], np.bincount(full[full > 0], minlength=len(pats) + 1), f"seed {seed}/{pname}/bincount of the full result")
    finally:
        h.destroy()


@pytest.mark.parametrize("platform,pname", PLATFORMS)
def test_accumulate_over_two_pieces_is_the_sum_of_their_counts(workdir, platform, pname):
    pats = ref.NESTED + [b"needle", b"nee", b"dle"]
    data = (b"b" + b"a" * 11 + b" needle nee " + b"a" * 5) * 40
    cut = len(data) // 2 + 3
    h = host_handle(pattern_file(workdir, "count_pieces", pats), platform)
    try:
        for flags in (0, LONGEST):
            first, t1 = host_counts(h, data[:cut], flags)
            second, t2 = host_counts(h, data[cut:], flags)
            both, t = host_counts(h, data[cut:], flags | ACCUMULATE, preset=first)
            ref.same(both, first + second, f"{pname}/flags {flags}")
            assert t == t2 and t1 == int(first.sum()) and t2 == int(second.sum()), "the total is what THIS call added"
            ref.same(first, ref.counts_py(pats, data[:cut], longest=bool(flags)), "the first piece")
        # entry 0 is left alone under ACCUMULATE, and zeroed without it
        preset = np.full(len(pats) + 1, 5, dtype=np.uint64)
        assert host_counts(h, data, ACCUMULATE, preset=preset)[0][0] == 5 and host_counts(h, data, 0, preset=preset)[0][0] == 0
    finally:
        h.destroy()


def test_accumulate_carries_into_the_high_word(workdir):
    h = host_handle(pattern_file(workdir, "count_carry", [b"a", b"zz"]))
    try:
        preset = np.array([7, 0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint64)
        got, total = host_counts(h, b"aaa", ACCUMULATE, preset=preset)
        assert got.tolist() == [7, 0x100000002, 0xFFFFFFFF] and total == 3
    finally:
        h.destroy()


def test_size_zero(workdir):
    h = host_handle(pattern_file(workdir, "count_zero", [b"ab", b"cd"]))
    try:
        preset = np.array([9, 9, 9], dtype=np.uint64)
        got, total = host_counts(h, b"", 0, preset=preset)
        assert got.tolist() == [0, 0, 0] and total == 0, "size == 0 zeroes the counts"
        got, total = host_counts(h, b"", ACCUMULATE, preset=preset)
        assert got.tolist() == [9, 9, 9] and total == 0, "... and leaves them alone under ACCUMULATE"
    finally:
        h.destroy()


def test_every_status_row_of_the_contract(workdir):
    pf = pattern_file(workdir, "count_errors", [b"ab", b"cd"])
    data = np.frombuffer(b"ab.cd.", dtype=np.uint8).copy()
    n = data.size
    counts = np.full(3 + GUARD, POISON, dtype=np.uint64)
    ids = np.full(4, -7, dtype=np.int32)
    I, K, D = data.ctypes.data, counts.ctypes.data, ids.ctypes.data
    lib = api.load_library()
    h = host_handle(pf)
    try:
        call = lambda *a: h.countFromHost(*a, check=False)[0]  # noqa: E731
        assert call(I, n, 0, K, 2) == INVALID, "numCounts < F + 1"
        assert call(I, 1 << 31, 0, K, 3) == INVALID, "size >= 2^31"
        assert call(I, n, 4, K, 3) == INVALID and call(I, n, 0x80000000, K, 3) == INVALID, "an unknown flag bit"
        assert call(None, n, 0, K, 3) == INVALID and call(I, n, 0, None, 3) == INVALID
        total = C.c_size_t(5)
        assert lib.PFACX_countFromHost(h._h, I, n, 0, K, 3, None) == INVALID
        # the device forms on a host-only handle
        assert h.countFromDevice(I, n, 0, K, 3, check=False)[0] == NOT_EXIST
        assert h.countFromDevice(I, 0, 0, K, 3, check=False)[0] == NOT_EXIST
        assert h.countPairsFromDevice(D, 4, 0, K, 3, check=False) == NOT_EXIST
        assert h.countPairsFromDevice(None, 0, 0, K, 3, check=False) == NOT_EXIST
        assert h.countNonzeroFromDevice(K, 3, D, K, 3, check=False)[0] == NOT_EXIST
        # ... behind their argument checks
        assert h.countFromDevice(I, n, 0, K, 2, check=False)[0] == INVALID and h.countFromDevice(I, n, 8, K, 3, check=False)[0] == INVALID
        assert h.countPairsFromDevice(D, 4, 0, K, 2, check=False) == INVALID and h.countPairsFromDevice(D, 1 << 31, 0, K, 3, check=False) == INVALID
        assert h.countPairsFromDevice(None, 4, 0, K, 3, check=False) == INVALID and h.countPairsFromDevice(D, 4, 4, K, 3, check=False) == INVALID
        assert h.countNonzeroFromDevice(None, 3, D, K, 3, check=False)[0] == INVALID and h.countNonzeroFromDevice(K, 3, None, K, 3, check=False)[0] == INVALID
        assert h.countNonzeroFromDevice(K, 1 << 31, D, K, 3, check=False)[0] == INVALID
        nd, tot = C.c_size_t(5), C.c_ulonglong(5)
        assert lib.PFACX_countNonzeroFromDevice(h._h, K, 3, D, K, 3, None, C.byref(tot)) == INVALID
        assert lib.PFACX_countNonzeroFromDevice(h._h, K, 3, D, K, 3, C.byref(nd), None) == INVALID
        assert np.all(counts == POISON) and np.all(ids == -7) and (total.value, nd.value, tot.value) == (5, 5, 5), "a refused call wrote"
        assert bytes(data) == b"ab.cd."
        # numCounts == 0 of the non-zero call: success with zeros, no device asked for
        assert lib.PFACX_countNonzeroFromDevice(h._h, None, 0, None, None, 0, C.byref(nd), C.byref(tot)) == 0 and (nd.value, tot.value) == (0, 0)
        assert h.countFromHost(I, n, 0, K, 3) == (0, 2) and counts[:3].tolist() == [0, 1, 1] and np.all(counts[3:] == POISON)
    finally:
        h.destroy()
    bare = api.PFAC.createHostOnly()
    try:
        assert bare.countFromHost(I, n, 0, K, 3, check=False)[0] == NOT_READY
        assert bare.countFromDevice(I, n, 0, K, 3, check=False)[0] == NOT_READY
        assert bare.countPairsFromDevice(D, 4, 0, K, 3, check=False) == NOT_READY
    finally:
        bare.destroy()
    total = C.c_size_t(0)
    assert lib.PFACX_countFromHost(None, I, n, 0, K, 3, C.byref(total)) == api.STATUS.INVALID_HANDLE
    assert lib.PFACX_countFromDevice(None, I, n, 0, K, 3, C.byref(total)) == api.STATUS.INVALID_HANDLE
    assert lib.PFACX_countPairsFromDevice(None, D, 4, 0, K, 3) == api.STATUS.INVALID_HANDLE
    assert lib.PFACX_countNonzeroFromDevice(None, K, 3, D, K, 3, C.byref(total), C.byref(C.c_ulonglong(0))) == api.STATUS.INVALID_HANDLE
