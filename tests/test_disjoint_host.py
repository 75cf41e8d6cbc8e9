"""PFACX_matchDisjointFromHost / PFACX_replaceFromHost on the CPU platforms (host-only handles: no device needed) against the references of
tests/disjoint_ref.py: the edge cases of the definition and seeded random cases over small alphabets against both references, every status row of
the contract, the replacement with empty, longer and shorter strings, truncation at every capacity, the size query, the overlap refusal, hostile
token and offset arrays, the 64-bit size, the example program."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pfac_amd import api
from tests import disjoint_ref as ref
from tests.disjoint_ref import GUARD, KINDS, RANDOM_SEEDS, host_disjoint, host_replace, repl_table, replacements_for
from tests.disjoint_ref import test_the_two_references_agree_on_every_case  # noqa: F401  (runs here: disjoint_ref.py is not collected)
from tests.spans_helpers import pattern_file, random_case
from tests.spans_ref import brute_result, pattern_lengths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
INVALID, NOT_READY, NOT_EXIST, TRUNCATED = (api.STATUS.INVALID_PARAMETER, api.STATUS.PATTERNS_NOT_READY, api.STATUS.LIB_NOT_EXIST,
                                            api.STATUS.OUTPUT_TRUNCATED)


def host_handle(pf, platform=api.PFAC_PLATFORM_CPU, flags=0):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    h.readPatternFromFileEx(pf, flags)
    return h


def check_replace(h, data, tokens, pats, what):
    """every kind of replacement table over one token list, against replace_py"""
    lengths = pattern_lengths(pats)
    for kind in KINDS:
        repls = replacements_for(pats, kind)
        want = ref.replace_py(data, tokens[0], tokens[1], lengths, repls)
        st, total, got = host_replace(h, data, tokens[0], tokens[1], repls)
        assert st == 0 and total == len(want) and got == want, f"{what}/{kind}: got {got[:80]!r} want {want[:80]!r}"


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_equals_both_references(workdir, case, platform, pname):
    name, pats, data = case
    nocase = name.startswith("nocase")
    h = host_handle(pattern_file(workdir, "dj_" + name, pats), platform, api.PFACX_READ_NOCASE if nocase else 0)
    try:
        got, covered, after = host_disjoint(h, data)
        ref.same(got, ref.disjoint_py(pats, data, nocase), f"{name}/{pname}/re")
        ref.same(got, ref.disjoint_from_result(brute_result(pats, data, nocase), pattern_lengths(pats)), f"{name}/{pname}/loop")
        assert covered == ref.covered_of(got, pattern_lengths(pats)), "coveredBytes is the sum of the lengths"
        assert after == data, "the caller's input was modified"
        if data:
            check_replace(h, data, got, pats, f"{name}/{pname}")      # (a caseless set: the text keeps the caller's bytes outside the tokens)
    finally:
        h.destroy()


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_cases_equal_both_references(workdir, seed):
    from oracle import binding as ob
    pats, data = random_case(seed)
    pf = pattern_file(workdir, f"dj_random{seed}", pats)
    o = ob.Oracle(pf, hashed=False)
    try:
        result = o.match(data)
    finally:
        o.close()
    lengths = pattern_lengths(pats)
    want = ref.disjoint_from_result(result, lengths)
    ref.same(ref.disjoint_py(pats, data.tobytes()), want, f"seed {seed}: the references")
    for platform, pname in PLATFORMS:
        h = host_handle(pf, platform)
        try:
            got, covered, after = host_disjoint(h, data.tobytes())
            ref.same(got, want, f"seed {seed}/{pname}")
            assert covered == ref.covered_of(want, lengths) and after == data.tobytes()
            if platform == api.PFAC_PLATFORM_CPU:
                check_replace(h, data.tobytes(), got, pats, f"seed {seed}")
        finally:
            h.destroy()


def test_every_status_row_of_the_selection(workdir):
    pf = pattern_file(workdir, "dj_errors", [b"ab", b"cd"])
    data = np.frombuffer(b"ab.cd.", dtype=np.uint8).copy()
    n = data.size
    ids, pos = (np.full(n, -7, dtype=np.int32) for _ in range(2))
    I, S, L = data.ctypes.data, ids.ctypes.data, pos.ctypes.data
    lib = api.load_library()
    h = host_handle(pf)
    try:
        call = lambda *a: h.matchDisjointFromHost(*a, check=False)[0]  # noqa: E731
        assert call(I, n, S, L, n - 1) == INVALID, "capacity < size"
        assert call(I, 1 << 31, S, L, 1 << 31) == INVALID, "size >= 2^31"
        assert call(None, n, S, L, n) == INVALID and call(I, n, None, L, n) == INVALID and call(I, n, S, None, n) == INVALID
        nt, cb = C.c_size_t(5), C.c_size_t(5)
        assert lib.PFACX_matchDisjointFromHost(h._h, I, n, S, L, n, None, C.byref(cb)) == INVALID
        assert lib.PFACX_matchDisjointFromHost(h._h, I, n, S, L, n, C.byref(nt), None) == INVALID
        assert np.all(ids == -7) and np.all(pos == -7) and (nt.value, cb.value) == (5, 5), "a refused call wrote"
        # size == 0: success, both counts 0, nothing touched (whatever the capacity)
        assert lib.PFACX_matchDisjointFromHost(h._h, I, 0, S, L, 0, C.byref(nt), C.byref(cb)) == 0 and (nt.value, cb.value) == (0, 0)
        assert np.all(ids == -7) and np.all(pos == -7)
        # the device forms on a host-only handle
        assert h.matchDisjointFromDevice(I, n, S, L, n, check=False)[0] == NOT_EXIST
        off, blob = repl_table([b"", b"x", b"y"])
        assert h.replaceFromDevice(I, n, S, L, 1, off.ctypes.data, off.size, blob.ctypes.data, blob.size, None, 0, check=False)[0] == NOT_EXIST
        assert np.all(ids == -7) and bytes(data) == b"ab.cd."
        assert h.matchDisjointFromHost(I, n, S, L, n) == (0, 2, 4) and ids[:2].tolist() == [1, 2] and pos[:2].tolist() == [0, 3]
    finally:
        h.destroy()
    bare = api.PFAC.createHostOnly()
    try:
        assert bare.matchDisjointFromHost(I, n, S, L, n, check=False)[0] == NOT_READY
        assert bare.matchDisjointFromDevice(I, n, S, L, n, check=False)[0] == NOT_READY
        assert bare.replaceFromHost(I, n, S, L, 0, None, 0, None, 0, None, 0, check=False)[0] == NOT_READY, "the replacement needs the pattern lengths"
        assert bare.replaceFromDevice(I, n, S, L, 0, None, 0, None, 0, None, 0, check=False)[0] == NOT_READY
    finally:
        bare.destroy()
    nt, cb = C.c_size_t(0), C.c_size_t(0)
    assert lib.PFACX_matchDisjointFromHost(None, I, n, S, L, n, C.byref(nt), C.byref(cb)) == api.STATUS.INVALID_HANDLE
    assert lib.PFACX_matchDisjointFromDevice(None, I, n, S, L, n, C.byref(nt), C.byref(cb)) == api.STATUS.INVALID_HANDLE
    assert lib.PFACX_replaceFromHost(None, I, n, S, L, 0, None, 0, None, 0, None, 0, C.byref(nt)) == api.STATUS.INVALID_HANDLE
    assert lib.PFACX_replaceFromDevice(None, I, n, S, L, 0, None, 0, None, 0, None, 0, C.byref(nt)) == api.STATUS.INVALID_HANDLE


# ---------------------------------------------------------------- the replacement


PATS = [b"needle", b"ab", b"x"]
TEXT = b"a needle, abab and x; needlex ab."


@pytest.fixture(scope="module")
def small(workdir):
    h = host_handle(pattern_file(workdir, "dj_small", PATS))
    tokens, _, _ = host_disjoint(h, TEXT)
    yield h, tokens
    h.destroy()


def test_replace_empty_longer_and_shorter_by_hand(small):
    h, tokens = small
    assert (tokens[0].tolist(), tokens[1].tolist()) == ([1, 2, 2, 3, 1, 3, 2], [2, 10, 12, 19, 22, 28, 30])
    for repls, want in (([b"", b"", b"", b""], b"a ,  and ;  ."),
                        ([b"", b"<N>", b"", b"times"], b"a <N>,  and times; <N>times ."),
                        ([b"", b"n", b"B", b"x"], b"a n, BB and x; nx B."),
                        ([b"", b"NEEDLE", b"AB", b"X"], b"a NEEDLE, ABAB and X; NEEDLEX AB.")):
        st, total, got = host_replace(h, TEXT, tokens[0], tokens[1], repls)
        assert (st, total, got) == (0, len(want), want)


def test_replace_without_tokens_is_a_copy(small):
    h, _ = small
    empty = np.zeros(0, dtype=np.int32)
    st, total, got = host_replace(h, TEXT, empty, empty, [b"", b"1", b"2", b"3"])
    assert (st, total, got) == (0, len(TEXT), TEXT)
    data = np.frombuffer(TEXT, dtype=np.uint8).copy()
    out = np.full(len(TEXT), 0xEE, dtype=np.uint8)
    assert h.replaceFromHost(data.ctypes.data, data.size, None, None, 0, None, 0, None, 0, out.ctypes.data, out.size) == (0, len(TEXT)), "the arrays may be null"
    assert out.tobytes() == TEXT
    assert h.replaceFromHost(data.ctypes.data, data.size, None, None, 1, None, 0, None, 0, out.ctypes.data, out.size, check=False)[0] == INVALID


def test_replace_truncation_at_every_capacity(small):
    h, tokens = small
    repls = [b"", b"<NEEDLE>", b"", b"yy"]
    want = ref.replace_py(TEXT, tokens[0], tokens[1], pattern_lengths(PATS), repls)
    for cap in range(len(want) + 1):
        st, total, got = host_replace(h, TEXT, tokens[0], tokens[1], repls, capacity=cap)          # (checks the guard bytes)
        assert total == len(want), "the full size whatever the capacity"
        assert st == (0 if cap == len(want) else TRUNCATED), f"capacity {cap}"
        if st == 0:
            assert got == want
    st, total, _ = host_replace(h, TEXT, tokens[0], tokens[1], repls, capacity=len(want) + 9)
    assert (st, total) == (0, len(want))


def test_replace_size_query_with_a_null_output(small):
    h, tokens = small
    off, blob = repl_table([b"", b"<NEEDLE>", b"", b"yy"])
    data = np.frombuffer(TEXT, dtype=np.uint8).copy()
    st, total = h.replaceFromHost(data.ctypes.data, data.size, tokens[0].ctypes.data, tokens[1].ctypes.data, tokens[0].size, off.ctypes.data, off.size,
                                  blob.ctypes.data, blob.size, None, 0, check=False)
    assert (st, total) == (TRUNCATED, len(TEXT) + 2 * 2 - 3 * 2 + 2 * 1)
    assert h.replaceFromHost(data.ctypes.data, data.size, tokens[0].ctypes.data, tokens[1].ctypes.data, tokens[0].size, off.ctypes.data, off.size,
                             blob.ctypes.data, blob.size, None, 5, check=False)[0] == INVALID, "a null output with a capacity"
    assert h.replaceFromHost(data.ctypes.data, 0, None, None, 0, None, 0, None, 0, None, 0) == (0, 0), "size == 0"


def test_replace_refuses_overlap_and_short_offset_tables(small):
    h, tokens = small
    n = len(TEXT)
    buf = np.full(3 * n, 0x61, dtype=np.uint8)
    buf[n:2 * n] = np.frombuffer(TEXT, dtype=np.uint8)
    off, blob = repl_table([b"", b"N", b"A", b"X"])
    base = buf.ctypes.data + n
    args = (tokens[0].ctypes.data, tokens[1].ctypes.data, tokens[0].size, off.ctypes.data, off.size, blob.ctypes.data, blob.size)
    for delta in (0, 1, -1, n - 1, 1 - n):
        assert h.replaceFromHost(base, n, *args, base + delta, n, check=False)[0] == INVALID, f"h_out = h_input + {delta}"
    assert buf[n:2 * n].tobytes() == TEXT and np.all(buf[:n] == 0x61) and np.all(buf[2 * n:] == 0x61), "a refused call wrote"
    for delta in (n, -n):                                       # ranges that touch do not overlap
        st, total = h.replaceFromHost(base, n, *args, base + delta, n, check=False)
        assert st == 0 and total <= n
    short = (tokens[0].ctypes.data, tokens[1].ctypes.data, tokens[0].size, off.ctypes.data, len(PATS) + 1, blob.ctypes.data, blob.size)
    out = np.zeros(2 * n, dtype=np.uint8)
    assert h.replaceFromHost(base, n, *short, out.ctypes.data, out.size, check=False)[0] == INVALID, "numOff < F + 2"


def test_replace_hostile_arrays_stay_inside_the_buffers(small):
    """the arrays are the caller's contract: unspecified text is allowed, an access outside the buffers is not (host_replace checks the guards; the
    input, token and table arrays are exactly as long as the call is told)"""
    h, _ = small
    n, big = len(TEXT), (1 << 31) - 1
    F = len(PATS)
    good = repl_table([b"", b"<N>", b"", b"times"])
    lists = {
        "negative starts": ([1, 2, 3], [-7, -1, -big]),
        "starts beyond size": ([1, 2, 3, 1], [n, n + 1, big, n - 2]),
        "descending": ([1, 2, 3, 2, 1], [30, 22, 19, 10, 2]),
        "ids 0, F + 1, negative": ([0, F + 1, -1, big, -big, 1], [2, 10, 12, 19, 22, 28]),
        "all the same": ([1] * 300, [2] * 300),
    }
    for what, (ids, pos) in lists.items():
        for cap in (0, 7, 4 * n):
            st, total, got = host_replace(h, TEXT, ids, pos, None, capacity=cap, table=good)
            assert st in (0, TRUNCATED), what
    tokens = ([1, 2, 2, 3], [2, 10, 12, 19])
    blob = np.frombuffer(b"0123456789", dtype=np.uint8).copy()
    for what, off in {"negative": [0, -5, -1, 3, 9], "beyond replBytes": [0, 5, big, 11, 10], "descending": [0, 9, 6, 3, 0]}.items():
        off = np.array(off, dtype=np.int32)
        for cap in (0, 4 * n):
            st, total, got = host_replace(h, TEXT, tokens[0], tokens[1], None, capacity=cap, table=(off, blob))
            assert st in (0, TRUNCATED), what
    # by the rules: ids outside [1, F] do nothing; a decreasing pair of offsets is an empty replacement; offsets are clamped to [0, replBytes]
    st, total, got = host_replace(h, b"a needle x", [0, 1, F + 1, 3], [0, 2, 8, 9], None, table=(np.array([0, 8, 4, 4, 99], dtype=np.int32), blob))
    assert (st, got) == (0, b"a  456789")


def test_replace_size_is_computed_in_64_bits(workdir):
    h = host_handle(pattern_file(workdir, "dj_justa", [b"a"]))
    try:
        n = 64 << 10
        tokens, covered, _ = host_disjoint(h, b"a" * n)
        assert tokens[0].size == n == covered
        st, total, _ = host_replace(h, b"a" * n, tokens[0], tokens[1], [b"", b"r" * n], capacity=0)
        assert (st, total) == (TRUNCATED, 1 << 32)
    finally:
        h.destroy()


def test_example_program_passes_its_self_check_on_the_host_forms(workdir):
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "replace_example"], check=True, stdout=subprocess.PIPE)
    exe = os.path.join(ROOT, "examples", "replace_example")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")          # no GPU visible: the host forms
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
    assert p.returncode == 0, p.stderr.decode()
    assert b"self-check passed" in p.stdout and b"(host forms)" in p.stdout
    rules = os.path.join(workdir, "dj_rules.txt")
    with open(rules, "wb") as f:
        f.write(b"cat\tdog\nthe \n")
    p = subprocess.run([exe, rules], input=b"the cat sat on the mat", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
    assert p.returncode == 0 and p.stdout == b"dog sat on mat", p.stderr.decode()
