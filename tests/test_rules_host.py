"""PFACX_rulesOpen / PFACX_rulesMatchFromHost / PFACX_rulesClose on the CPU platforms (host-only handles: no device needed) against the reference of
tests/rules_ref.py, which never calls the library: the case table, a 33-pattern rule, one byte that fires 1 000 rules with truncation and the
count query, the seeded random cases, every invalid-argument status of the contract, a rule set whose pattern set has been replaced, PFAC_destroy
with a rule set open, and the example program on its host path."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pfac_amd import api
from tests import rules_ref as ref
from tests.spans_helpers import pattern_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
INVALID, TRUNCATED = api.STATUS.INVALID_PARAMETER, api.STATUS.OUTPUT_TRUNCATED
GUARD = 16


def host_handle(pf, platform=api.PFAC_PLATFORM_CPU, flags=0):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    h.readPatternFromFileEx(pf, flags)
    return h


def host_fired(r, data, offsets, capacity=None, seg_first=True):
    """match_host over poisoned arrays with guard words behind capacity and behind segFirst -> (status, (seg, rule, segFirst), full count); the
    input must stay untouched"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy() if not isinstance(data, np.ndarray) else data.copy()
    keep = buf.copy()
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uintp)
    segs = 1 if off is None else off.size - 1
    if capacity is None:                                                    # the count query first, as a caller would
        _, capacity = r.match_host(buf.ctypes.data, buf.size, None if off is None else off.ctypes.data, segs, None, None, 0, None)
    seg, rule = (np.full(capacity + GUARD, -7, dtype=np.int32) for _ in range(2))
    first = np.full(segs + 1 + GUARD, 0xDEAD, dtype=np.uintp)
    st, n = r.match_host(buf.ctypes.data if buf.size else seg.ctypes.data, buf.size, None if off is None else off.ctypes.data, segs,
                         seg.ctypes.data, rule.ctypes.data, capacity, first.ctypes.data if seg_first else None, check=False)
    assert np.array_equal(buf, keep), "the caller's input was modified"
    k = min(n, capacity)
    assert np.all(seg[k:] == -7) and np.all(rule[k:] == -7), "wrote behind the list or behind capacity"
    assert np.all(first[segs + 1:] == 0xDEAD), "wrote behind segFirst"
    return st, (seg[:k].copy(), rule[:k].copy(), first[:segs + 1].copy()), n


@pytest.mark.parametrize("platform", PLATFORMS, ids=[p[1] for p in PLATFORMS])
@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_case_table(workdir, case, platform):
    name, pats, rules, data, offsets = case
    nocase = ref.is_nocase(name)
    h = host_handle(pattern_file(workdir, "rules_" + name, pats), platform[0], api.PFACX_READ_NOCASE if nocase else 0)
    try:
        r = h.rulesOpen(*ref.csr(rules))
        want = ref.fired_py(pats, rules, data, offsets, nocase)
        st, got, n = host_fired(r, data, offsets)
        assert st == 0 and n == want[0].size
        ref.same(got, want, name)
        ref.same(r.match_host_array(np.frombuffer(data, dtype=np.uint8), offsets), want, name + "/match_host_array")
        assert r.close() == 0
    finally:
        h.destroy()


def test_the_cases_say_what_the_issue_says():
    """the reference itself, on the cases whose answer the contract spells out"""
    by = {c[0]: c for c in ref.CASES}

    def pairs(name):
        _, pats, rules, data, offsets = by[name]
        seg, rule, _ = ref.fired_py(pats, rules, data, offsets, ref.is_nocase(name))
        return list(zip(seg.tolist(), rule.tolist()))

    assert pairs("two-patterns-in-different-segments") == []
    assert pairs("two-patterns-in-one-segment") == [(1, 0), (1, 1), (1, 2)]
    assert pairs("proper-prefix-never-the-longest") == [(0, 0), (0, 1), (0, 2)]
    assert pairs("only-across-a-border") == [(0, 1)]
    assert pairs("thirty-two-patterns-31-present") == [(0, 1)]
    assert pairs("thirty-two-patterns-all-present") == [(0, 0), (0, 1)]
    assert pairs("nocase") == [(0, 0), (1, 1), (1, 2)]


def test_a_rule_of_33_distinct_patterns_is_refused_and_33_ids_of_32_patterns_are_not(workdir):
    pats = [b"q%02d;" % i for i in range(33)]
    h = host_handle(pattern_file(workdir, "rules_33", pats))
    try:
        r = h.rulesOpen(*ref.csr([list(range(1, 34))]), check=False)
        assert r.status == INVALID
        r = h.rulesOpen(*ref.csr([list(range(1, 33)) + [7]]))               # 33 ids, 32 distinct
        st, got, n = host_fired(r, b"".join(pats[:32]), None)
        assert (st, n) == (0, 1) and got[1].tolist() == [0]
        r.close()
    finally:
        h.destroy()


def test_one_byte_fires_a_thousand_rules(workdir):
    h = host_handle(pattern_file(workdir, "rules_byte", [b"x", b"y"]))
    try:
        rules = [[1]] * 1000 + [[2]] + [[1, 2]]
        r = h.rulesOpen(*ref.csr(rules))
        want = ref.fired_py([b"x", b"y"], rules, b"x", [0, 1])
        st, got, n = host_fired(r, b"x", [0, 1])
        assert (st, n) == (0, 1000)
        ref.same(got, want, "1000 rules from one byte")
        st, got, n = host_fired(r, b"x", [0, 1], capacity=10)               # exactly 10 pairs, the full count, the full segFirst
        assert (st, n) == (TRUNCATED, 1000)
        ref.same(got, (want[0][:10], want[1][:10], want[2]), "truncated at 10")
        buf = np.frombuffer(b"x", dtype=np.uint8).copy()
        off = np.array([0, 1], dtype=np.uintp)
        st, n = r.match_host(buf.ctypes.data, 1, off.ctypes.data, 1, None, None, 0, None, check=False)     # the count query with null arrays
        assert (st, n) == (TRUNCATED, 1000)
        r.close()
    finally:
        h.destroy()


@pytest.mark.parametrize("platform", PLATFORMS, ids=[p[1] for p in PLATFORMS])
@pytest.mark.parametrize("seed", ref.RANDOM_SEEDS)
def test_random_cases(workdir, seed, platform):
    pats, rules, data, offsets = ref.random_case(seed)
    h = host_handle(pattern_file(workdir, "rules_rnd%d" % seed, pats), platform[0])
    try:
        r = h.rulesOpen(*ref.csr(rules))
        want = ref.fired_py(pats, rules, data.tobytes(), offsets)
        st, got, n = host_fired(r, data, offsets)
        assert st == 0 and n == want[0].size
        ref.same(got, want, f"seed {seed}")
        if n > 1:
            st, got, n2 = host_fired(r, data, offsets, capacity=n - 1)
            assert (st, n2) == (TRUNCATED, n)
            ref.same(got, (want[0][:n - 1], want[1][:n - 1], want[2]), f"seed {seed}/truncated")
        r.close()
    finally:
        h.destroy()


@pytest.mark.parametrize("platform", PLATFORMS, ids=[p[1] for p in PLATFORMS])
def test_every_capacity_with_and_without_seg_first(workdir, platform):
    """the list frame at its edges: an empty first, middle and last segment; every capacity from 0 to the length of the list + 1 -- inside a segment,
    exactly at a segment's border (segFirst = 0, 0, 4, 4, 7, 7), the length - 1, the length itself --, each with segFirst and with a null one"""
    pats, rules = [b"a", b"aa", b"aaa", b"b", b"ab"], [[1, 4], [3], [5, 2], [1]]
    data, offsets = ref.cut(b"", b"aaab", b"", b"baab", b"")
    want = ref.fired_py(pats, rules, data, offsets)
    assert want[2].tolist() == [0, 0, 4, 4, 7, 7]
    total = int(want[0].size)
    h = host_handle(pattern_file(workdir, "rules_caps", pats), platform[0])
    try:
        r = h.rulesOpen(*ref.csr(rules))
        for capacity in range(total + 2):
            for seg_first in (True, False):
                st, got, n = host_fired(r, data, offsets, capacity=capacity, seg_first=seg_first)
                assert (st, n) == (TRUNCATED if capacity < total else 0, total), f"capacity {capacity}"
                ref.same(got[:2], (want[0][:capacity], want[1][:capacity]), f"capacity {capacity}")
                if seg_first:
                    assert got[2].tolist() == want[2].tolist(), f"capacity {capacity}: segFirst is complete"
                else:
                    assert np.all(got[2] == 0xDEAD), "a null segFirst and something was written"
        r.close()
    finally:
        h.destroy()


def test_numpy_reference_agrees_with_the_plain_one():
    for seed in ref.RANDOM_SEEDS[:12]:
        pats, rules, data, offsets = ref.random_case(seed)
        ref.same(ref.fired_np(pats, rules, data, offsets), ref.fired_py(pats, rules, data.tobytes(), offsets), f"seed {seed}")


def test_open_statuses(workdir):
    pats = [b"a", b"b", b"c"]
    h = host_handle(pattern_file(workdir, "rules_open", pats))
    bare = api.PFAC.createHostOnly()
    lib = api.load_library()
    try:
        def status(off, ids, handle=h):
            return handle.rulesOpen(np.array(off, dtype=np.int32), np.array(ids, dtype=np.int32), check=False).status

        assert status([0, 1], [1], bare) == api.STATUS.PATTERNS_NOT_READY
        assert status([0, 1], [0]) == INVALID                               # an id below 1
        assert status([0, 1], [4]) == INVALID                               # an id above F
        assert status([0, 0], [1]) == INVALID                               # an empty rule
        assert status([1, 2], [1, 2]) == INVALID                            # offsets that do not start at 0
        assert status([0, 2, 1], [1, 2]) == INVALID                         # offsets that decrease
        assert status([0], []) == INVALID                                   # no rule
        off, ids = np.array([0, 1], dtype=np.int32), np.array([1], dtype=np.int32)
        out = C.c_void_p()
        assert lib.PFACX_rulesOpen(h._h, None, ids.ctypes.data, 1, C.byref(out)) == INVALID
        assert lib.PFACX_rulesOpen(h._h, off.ctypes.data, None, 1, C.byref(out)) == INVALID
        assert lib.PFACX_rulesOpen(h._h, off.ctypes.data, ids.ctypes.data, 1, None) == INVALID
        assert lib.PFACX_rulesOpen(h._h, off.ctypes.data, ids.ctypes.data, 1 << 24, C.byref(out)) == INVALID
        assert lib.PFACX_rulesOpen(None, off.ctypes.data, ids.ctypes.data, 1, C.byref(out)) == api.STATUS.INVALID_HANDLE
        assert lib.PFACX_rulesClose(None) == api.STATUS.INVALID_HANDLE
        good = h.rulesOpen(off, ids)
        ids[0] = 3                                                          # the arrays were copied
        assert host_fired(good, b"a", None)[2] == 1
        good.close()
    finally:
        bare.destroy()
        h.destroy()


def test_match_statuses(workdir):
    h = host_handle(pattern_file(workdir, "rules_args", [b"ab", b"b"]))
    try:
        r = h.rulesOpen(*ref.csr([[1], [1, 2]]))
        buf = np.frombuffer(b"abab", dtype=np.uint8).copy()
        off = np.array([0, 2, 4], dtype=np.uintp)
        seg, rule = (np.zeros(8, dtype=np.int32) for _ in range(2))
        first = np.zeros(3, dtype=np.uintp)
        I, O, S, R, F = buf.ctypes.data, off.ctypes.data, seg.ctypes.data, rule.ctypes.data, first.ctypes.data

        def status(*args):
            return r.match_host(*args, check=False)[0]

        assert status(I, 4, O, 2, S, R, 8, F) == 0
        assert status(None, 4, O, 2, S, R, 8, F) == INVALID
        assert status(I, 4, O, 2, None, R, 8, F) == INVALID                 # null arrays with a capacity
        assert status(I, 4, O, 2, S, None, 8, F) == INVALID
        assert status(I, 4, None, 2, S, R, 8, F) == INVALID                 # no offsets: one segment only
        assert status(I, 4, O, 0, S, R, 8, F) == INVALID                    # no segment, but bytes
        assert status(I, 1 << 31, O, 2, S, R, 8, F) == INVALID
        assert status(I, 4, O, 1 << 31, S, R, 8, F) == INVALID
        for bad in ([1, 2, 4], [0, 2, 3], [0, 3, 2]):                       # host offsets are validated
            b = np.array(bad, dtype=np.uintp)
            assert status(I, 4, b.ctypes.data, 2, S, R, 8, F) == INVALID
        lib = api.load_library()
        assert lib.PFACX_rulesMatchFromHost(r._r, I, 4, O, 2, S, R, 8, F, None) == INVALID
        assert lib.PFACX_rulesMatchFromHost(None, I, 4, O, 2, S, R, 8, F, C.byref(C.c_size_t())) == api.STATUS.INVALID_HANDLE
        assert status(I, 4, O, 2, S, R, 8, None) == 0                       # segFirst may be null
        assert r.match_device(I, 4, O, 2, S, R, 8, F, check=False)[0] == api.STATUS.LIB_NOT_EXIST      # the device form on a host-only handle
        # size == 0: success, nothing fired, segFirst all zero
        first[:] = 77
        st, n = r.match_host(I, 0, np.zeros(3, dtype=np.uintp).ctypes.data, 2, S, R, 8, F)
        assert (st, n) == (0, 0) and first.tolist() == [0, 0, 0]
        assert r.match_host(I, 0, None, 1, S, R, 8, None) == (0, 0)
        assert r.match_host(I, 0, O, 0, S, R, 8, None) == (0, 0)
        r.close()
    finally:
        h.destroy()


def test_a_rule_set_of_a_replaced_pattern_set_only_closes(workdir):
    h = host_handle(pattern_file(workdir, "rules_gen_a", [b"ab", b"b"]))
    try:
        r = h.rulesOpen(*ref.csr([[1, 2]]))
        assert host_fired(r, b"ab", None)[2] == 1
        h.readPatternFromFile(pattern_file(workdir, "rules_gen_b", [b"zz", b"b", b"ab"]))
        st, _, _ = host_fired(r, b"ab", None, capacity=4)
        assert st == INVALID
        buf = np.frombuffer(b"ab", dtype=np.uint8).copy()
        assert r.match_device(buf.ctypes.data, 2, None, 1, None, None, 0, None, check=False)[0] in (INVALID, api.STATUS.LIB_NOT_EXIST)
        assert r.close() == 0
        fresh = h.rulesOpen(*ref.csr([[1, 2]]))                             # the same ids over the new set
        assert host_fired(fresh, b"ab", None)[2] == 0 and host_fired(fresh, b"zzb", None)[2] == 1
        fresh.close()
    finally:
        h.destroy()


def test_destroy_closes_open_rule_sets(workdir):
    h = host_handle(pattern_file(workdir, "rules_destroy", [b"a"]))
    for _ in range(3):
        h.rulesOpen(*ref.csr([[1]] * 5))
    assert h.destroy() == 0


def test_example_program_on_its_host_path(workdir):
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "rules_example"], check=True, stdout=subprocess.PIPE)
    exe = os.path.join(ROOT, "examples", "rules_example")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")          # no GPU visible: the host form
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
    assert p.returncode == 0, p.stderr.decode()
    assert b"self-check passed" in p.stdout and b"(host form)" in p.stdout
    rules = os.path.join(workdir, "rules_example.txt")
    with open(rules, "wb") as f:
        f.write(b"pay-error\tERROR\tpayment-service\nany-get\tGET\nadmin\tGET\t/admin\n")
    text = b"GET /index\nERROR in payment-service\npayment-service ok\nGET /admin ERROR\n"
    p = subprocess.run([exe, rules], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout.decode().splitlines() == ["record 0: rule any-get", "record 1: rule pay-error", "record 3: rule any-get", "record 3: rule admin"]
