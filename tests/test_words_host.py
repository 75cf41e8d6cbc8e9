"""PFACX_matchWordsFromHost on the CPU platforms (host-only handles: no device needed) against the references of tests/words_ref.py: every case of
the table in both modes, seeded random cases over the oracle's vector with a delimiter class, truncation, every status row of the contract, size 0,
the empty-class identities against PFACX_matchAllFromHost and PFAC_matchFromHostReduce, the word_class helper."""

import ctypes as C

import numpy as np
import pytest

from pfac_amd import api
from tests import allmatch_ref as am
from tests import words_ref as ref
from tests.words_ref import test_the_two_references_agree_on_every_case  # noqa: F401  (runs here: words_ref.py is not collected)
from tests.spans_helpers import RANDOM_SEEDS, pattern_file, random_case

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
INVALID, NOT_READY, NOT_EXIST, TRUNCATED = (api.STATUS.INVALID_PARAMETER, api.STATUS.PATTERNS_NOT_READY, api.STATUS.LIB_NOT_EXIST,
                                            api.STATUS.OUTPUT_TRUNCATED)
ALL = api.PFACX_WORDS_ALL
GUARD = 16


def cls_arg(cls):
    return None if cls is None else api.word_class(cls)


def host_handle(pf, platform=api.PFAC_PLATFORM_CPU, flags=0):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    h.readPatternFromFileEx(pf, flags)
    return h


def host_words(h, data, cls, flags, capacity=None):
    """matchWordsFromHost into poisoned arrays of `capacity` entries (default: what never truncates) with GUARD poisoned ints on both sides ->
    (status, (pos, ids) of the pairs written, the full length); nothing outside the written pairs may change, nor the input"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    n = buf.size
    cap = max(n, 1) * max(1, int(h.info().maxMatchesPerPosition)) if capacity is None else capacity
    ids, pos = (np.full(GUARD + cap + GUARD, -7, dtype=np.int32) for _ in range(2))
    st, total = h.matchWordsFromHost(buf.ctypes.data, n, cls_arg(cls), flags, ids.ctypes.data + 4 * GUARD, pos.ctypes.data + 4 * GUARD, cap, check=False)
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > cap)
    k = min(total, cap)
    for a in (ids, pos):
        assert np.all(a[:GUARD] == -7) and np.all(a[GUARD + cap:] == -7), "wrote outside the arrays"
        assert np.all(a[GUARD + k:GUARD + cap] == -7), "wrote behind the list"
    assert buf.tobytes() == bytes(data), "the caller's input was modified"
    return st, (pos[GUARD:GUARD + k].copy(), ids[GUARD:GUARD + k].copy()), total


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_equals_the_references(workdir, case, platform, pname):
    name, pats, data, cls, nocase = case
    h = host_handle(pattern_file(workdir, "words_" + name, pats), platform, api.PFACX_READ_NOCASE if nocase else 0)
    try:
        for flags in (0, ALL):
            want = ref.words_brute(pats, data, cls, bool(flags), nocase)
            st, got, total = host_words(h, data, cls, flags)
            assert st == 0 and total == want[0].size
            ref.same(got, want, f"{name}/{pname}/flags {flags}")
            if cls is None:
                ref.same(got, ref.words_re(pats, data, bool(flags), nocase), f"{name}/{pname}/flags {flags}: against re")
            if name in ref.WANT:
                ids, pos = ref.WANT[name][flags]
                ref.same(got, (pos, ids), f"{name}/{pname}/flags {flags}: against the list worked out by hand")
            ref.same(h.match_words_host_array(np.frombuffer(data, dtype=np.uint8), cls_arg(cls), bool(flags)), want, f"{name}/match_words_host_array")
    finally:
        h.destroy()


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_cases_equal_the_oracle(workdir, seed, platform, pname):
    """letters a, b (c): the class {a} (and {a, b}) makes the other letters delimiters"""
    from oracle import binding as ob
    pats, data = random_case(seed)
    pf = pattern_file(workdir, f"words_random{seed}", pats)
    o = ob.Oracle(pf, hashed=False)
    try:
        result = o.match(data)
    finally:
        o.close()
    prefix, chain, _ = am.prefix_table(pats)
    lengths = [0] + [len(p) for p in pats]
    h = host_handle(pf, platform)
    try:
        for cls in (b"a", b"ab", ref.EMPTY):
            for flags in (0, ALL):
                want = ref.words_from_result(result, (prefix, chain), lengths, data, cls, bool(flags))
                st, got, total = host_words(h, data.tobytes(), cls, flags)
                assert st == 0 and total == want[0].size
                ref.same(got, want, f"seed {seed}/{pname}/class {cls}/flags {flags}")
    finally:
        h.destroy()


@pytest.mark.parametrize("platform,pname", PLATFORMS)
def test_the_empty_class_gives_the_lists_of_the_calls_without_a_class(workdir, platform, pname):
    pats = ref.NESTED + [b"needle", b"nee", b"dle"]
    data = (b"b" + b"a" * 11 + b" needle nee " + b"a" * 5) * 40
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    h = host_handle(pattern_file(workdir, "words_identity", pats), platform)
    try:
        st, got, total = host_words(h, data, ref.EMPTY, ALL)
        ref.same(got, h.match_all_host_array(buf), "ALL under the empty class is the all-match list")
        ids, pos = (np.full(buf.size, -7, dtype=np.int32) for _ in range(2))
        _, n = h.matchFromHostReduce(buf.ctypes.data, buf.size, ids.ctypes.data, pos.ctypes.data)
        st, got, total = host_words(h, data, ref.EMPTY, 0)
        assert total == n
        ref.same(got, (pos[:n], ids[:n]), "the word list under the empty class is the list of PFAC_matchFromHostReduce")
    finally:
        h.destroy()


def test_truncation_writes_the_first_capacity_pairs_and_nothing_behind_them(workdir):
    """ALL can be longer than the input, and capacity >= size: the 15 pairs of 9 bytes at capacities 14 (the length minus 1) and 9 (the size); the
    capacity of 1 over one byte (capacity >= size and one byte holds one pair at most: the only call with capacity 1, and it cannot truncate)"""
    h = host_handle(pattern_file(workdir, "words_trunc", ref.SPACED))
    try:
        data = b"a a a a a"
        want = ref.words_brute(ref.SPACED, data, None, True)
        assert want[0].size == 15
        for cap in (14, 9):
            st, got, total = host_words(h, data, None, ALL, capacity=cap)
            assert (st, total) == (TRUNCATED, 15)
            ref.same(got, (want[0][:cap], want[1][:cap]), f"capacity {cap}")
        st, got, total = host_words(h, data, None, ALL, capacity=15)
        assert (st, total) == (0, 15)
        st, got, total = host_words(h, b"a", None, ALL, capacity=1)
        assert (st, total) == (0, 1) and got[0].tolist() == [0] and got[1].tolist() == [1]
        with pytest.raises(api.PFACError):
            h.match_words_host_array(np.frombuffer(data, dtype=np.uint8), None, True, capacity=9)
    finally:
        h.destroy()


def test_size_zero_touches_nothing(workdir):
    h = host_handle(pattern_file(workdir, "words_zero", [b"ab"]))
    try:
        ids = np.full(4, -7, dtype=np.int32)
        n = C.c_size_t(5)
        lib = api.load_library()
        for flags in (0, ALL):
            assert lib.PFACX_matchWordsFromHost(h._h, ids.ctypes.data, 0, None, flags, ids.ctypes.data, ids.ctypes.data, 0, C.byref(n)) == 0
            assert n.value == 0 and np.all(ids == -7)
            n.value = 5
    finally:
        h.destroy()


def test_every_status_row_of_the_contract(workdir):
    pf = pattern_file(workdir, "words_errors", [b"ab", b"cd"])
    data = np.frombuffer(b"ab.cd.", dtype=np.uint8).copy()
    n = data.size
    ids, pos = (np.full(n + GUARD, -7, dtype=np.int32) for _ in range(2))
    I, A, P = data.ctypes.data, ids.ctypes.data, pos.ctypes.data
    lib = api.load_library()
    h = host_handle(pf)
    try:
        call = lambda *a: h.matchWordsFromHost(*a, check=False)[0]  # noqa: E731
        assert call(I, n, None, 0, A, P, n - 1) == INVALID, "capacity < size"
        assert call(I, 1 << 31, None, 0, A, P, 1 << 31) == INVALID, "size >= 2^31"
        assert call(I, n, None, 2, A, P, n) == INVALID and call(I, n, None, 0x80000000, A, P, n) == INVALID, "an unknown flag bit"
        assert call(None, n, None, 0, A, P, n) == INVALID and call(I, n, None, 0, None, P, n) == INVALID and call(I, n, None, 0, A, None, n) == INVALID
        assert lib.PFACX_matchWordsFromHost(h._h, I, n, None, 0, A, P, n, None) == INVALID
        # the device forms on a host-only handle, and behind their argument checks
        pairs = lambda *a: h.wordsPairsFromDevice(*a, check=False)[0]  # noqa: E731
        assert h.matchWordsFromDevice(I, n, None, 0, A, P, n, check=False)[0] == NOT_EXIST
        assert pairs(I, n, None, 0, A, P, 2, A + 64, P + 64, 2) == NOT_EXIST
        assert pairs(I, n, None, 0, A, P, 2, None, None, 0) == NOT_EXIST, "the count query"
        assert h.matchWordsFromDevice(I, n, None, 0, A, P, n - 1, check=False)[0] == INVALID
        assert h.matchWordsFromDevice(I, n, None, 4, A, P, n, check=False)[0] == INVALID
        assert pairs(I, n, None, 2, A, P, 2, A + 64, P + 64, 2) == INVALID and pairs(I, 1 << 31, None, 0, A, P, 2, A + 64, P + 64, 2) == INVALID
        assert pairs(None, n, None, 0, A, P, 2, A + 64, P + 64, 2) == INVALID and pairs(I, n, None, 0, None, P, 2, A + 64, P + 64, 2) == INVALID
        assert pairs(I, n, None, 0, A, P, 2, None, P + 64, 2) == INVALID and pairs(I, n, None, 0, A, P, 1 << 31, A + 64, P + 64, 2) == INVALID
        for out_ids, out_pos in ((A, P + 64), (A + 64, P), (A + 4, P + 64), (P + 4, A + 64), (A - 4, P + 64)):
            assert pairs(I, n, None, 0, A, P, 2, out_ids, out_pos, 2) == INVALID, "output arrays that overlap the pair arrays"
        assert lib.PFACX_wordsPairsFromDevice(h._h, I, n, None, 0, A, P, 2, A + 64, P + 64, 2, None) == INVALID
        assert np.all(ids == -7) and np.all(pos == -7) and bytes(data) == b"ab.cd.", "a refused call wrote"
        st, total = h.matchWordsFromHost(I, n, None, 0, A, P, n)
        assert (st, total) == (0, 2) and ids[:2].tolist() == [1, 2] and pos[:2].tolist() == [0, 3], "the handle is usable after refused calls"
    finally:
        h.destroy()
    bare = api.PFAC.createHostOnly()
    try:
        assert bare.matchWordsFromHost(I, n, None, 0, A, P, n, check=False)[0] == NOT_READY
        assert bare.matchWordsFromDevice(I, n, None, 0, A, P, n, check=False)[0] == NOT_READY
        assert bare.wordsPairsFromDevice(I, n, None, 0, A, P, 2, A + 64, P + 64, 2, check=False)[0] == NOT_READY
    finally:
        bare.destroy()
    total = C.c_size_t(0)
    assert lib.PFACX_matchWordsFromHost(None, I, n, None, 0, A, P, n, C.byref(total)) == api.STATUS.INVALID_HANDLE
    assert lib.PFACX_matchWordsFromDevice(None, I, n, None, 0, A, P, n, C.byref(total)) == api.STATUS.INVALID_HANDLE
    assert lib.PFACX_wordsPairsFromDevice(None, I, n, None, 0, A, P, 2, A + 64, P + 64, 2, C.byref(total)) == api.STATUS.INVALID_HANDLE
    # a host form on the GPU platform of a host-only handle says so loudly
    h = host_handle(pf)
    try:
        h.setPlatform(api.PFAC_PLATFORM_GPU)
        assert h.matchWordsFromHost(I, n, None, 0, A, P, n, check=False)[0] == NOT_EXIST
    finally:
        h.destroy()


def test_word_class_builds_the_eight_words():
    assert list(api.word_class()) == [0, 0x03FF0000, 0x87FFFFFE, 0x07FFFFFE, 0, 0, 0, 0], "the default class [0-9A-Za-z_]"
    assert list(api.word_class(b"")) == [0] * 8 and list(api.word_class(bytes(range(256)))) == [0xFFFFFFFF] * 8
    assert list(api.word_class(b"\x00\x1f \xff")) == [0x80000001, 1, 0, 0, 0, 0, 0, 0x80000000]
    words = list(api.word_class_except(b"\n"))
    assert words[0] == 0xFFFFFFFF & ~(1 << 10) and words[1:] == [0xFFFFFFFF] * 7
    for cls in (None, ref.CSV, b"a"):
        words = list(api.word_class(cls))
        assert [b for b in range(256) if words[b >> 5] >> (b & 31) & 1] == sorted(ref.members(cls))
