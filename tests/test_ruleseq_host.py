"""PFACX_rulesOpenSeq -- ordered rule members with distance and within -- through PFACX_rulesMatchFromHost on the CPU platforms (host-only handles:
no device needed) against the reference of tests/ruleseq_ref.py, which never calls the library and is itself checked against Python's `re`: the
greedy traps, the bounds, the same pattern twice, a member that is a proper prefix, own windows on relative members, two chains that share an
occurrence, a chain with a negated member, a 32-member chain, a caseless set, borders and empty segments, the cases sized by the kernel's trip,
window, touched list and grid, the equivalence with PFACX_rulesOpenEx for sets without a relative member, the seeded random cases and every refusal
of the contract.  Every case also runs truncated at half its list and as a count query."""

import ctypes as C

import numpy as np
import pytest

from pfac_amd import api
from tests import rulecond_ref as rc
from tests import rules_ref as ref
from tests import ruleseq_ref as rs
from tests.spans_helpers import pattern_file

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
INVALID = api.STATUS.INVALID_PARAMETER
NOT, FROM_END, RELATIVE, S, R = rs.NOT, rs.FROM_END, rs.RELATIVE, rs.S, rs.R
BUILT = [rs.window_case(), rs.touched_case(), rs.clean_state_case(8), rs.TRUNCATION]


def host_handle(pf, platform=api.PFAC_PLATFORM_CPU, flags=0):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    h.readPatternFromFileEx(pf, flags)
    return h


def check_host(r, want, data, offsets, what):
    rc.check_forms(lambda capacity, null: rc.host_fired(r, data, offsets, capacity, null), want, what)


def test_the_binding_matches_the_header():
    assert (api.PFACX_RULE_NOT, api.PFACX_RULE_FROM_END, api.PFACX_RULE_RELATIVE) == (NOT, FROM_END, RELATIVE)
    assert api.rule_seq_member_dtype() == rs.MEMBER and rs.MEMBER.itemsize == 24
    assert (rs.WINDOW, rs.TOUCHED, rs.TRIP) == (api.PFACX_RULES_WINDOW, api.PFACX_RULES_TOUCHED, api.PFACX_RULES_BLOCK_PAIRS)
    assert "PFACX_rulesOpenSeq" in api.EXPORTED_SYMBOLS


@pytest.mark.parametrize("platform", PLATFORMS, ids=[p[1] for p in PLATFORMS])
@pytest.mark.parametrize("case", rs.CASES + BUILT, ids=[c[0] for c in rs.CASES + BUILT])
def test_case_table(workdir, case, platform):
    name, pats, rules, data, offsets = case
    nocase = rs.is_nocase(name)
    h = host_handle(pattern_file(workdir, "ruleseq_" + name, pats), platform[0], api.PFACX_READ_NOCASE if nocase else 0)
    try:
        r = h.rulesOpenSeq(*rs.csr(rules))
        want = rs.fired_py(pats, rules, data, offsets, nocase)
        check_host(r, want, data, offsets, name)
        assert r.close() == 0
    finally:
        h.destroy()


def test_the_cases_say_what_the_issue_says():
    """the reference itself, on the cases whose answer the contract spells out"""
    by = {c[0]: c for c in rs.CASES + BUILT}

    def fired(name):
        _, pats, rules, data, offsets = by[name]
        return rc.pairs(rs.fired_py(pats, rules, data, offsets, rs.is_nocase(name)))

    assert fired("trap-only-the-second-A-is-near-enough") == [(0, 0), (0, 1), (1, 0)]
    assert fired("trap-only-the-second-B-is-far-enough") == [(0, 0)]
    assert fired("trap-the-latest-A-leads-nowhere") == [(0, 0), (1, 0)]
    assert fired("trap-the-earliest-A-leads-nowhere") == [(0, 0)]
    assert fired("trap-the-near-A-is-not-reachable") == [(0, 1), (1, 0), (1, 1)]
    bounds = fired("bounds")
    assert [k for k, r in bounds if r == 0] == []                           # within < len(B): never
    assert [k for k, r in bounds if r == 1] == [0]                          # within == len(B), distance 0: adjacency
    assert [k for k, r in bounds if r in (2, 3, 6)] == []                   # distance past the segment; 0xFFFFFFFF satisfies nothing
    assert [k for k, r in bounds if r == 4] == [0, 1, 3]                    # within == 0: somewhere behind, not overlapping
    assert [k for k, r in bounds if r == 7] == [0, 1, 3]
    assert [k for k, r in bounds if r == 5] == [1, 3]
    assert [k for k, r in bounds if r == 10] == [3] and [k for k, r in bounds if r == 11] == []
    assert fired("same-pattern-twice") == [(1, 0), (2, 0), (2, 2), (3, 0), (3, 1), (3, 2)]          # aa then aa: not over aaa, over aaaa
    prefix = fired("proper-prefix-member")
    assert [r for k, r in prefix if k == 0] == [0, 1, 2]                    # foo then bar over `foobar bar`, with foobar in the set
    assert fired("two-chains-share-an-occurrence")[:3] == [(0, 0), (0, 1), (2, 0)]
    assert [k for k, r in fired("thirty-two-member-chain") if r == 0] == [0, 1, 3]
    assert [k for k, r in fired("thirty-two-member-chain") if r == 1] == [0]
    assert fired("nocase-chain") == [(0, 0), (3, 1)]
    assert fired("across-a-border-and-empty-segments") == [(4, 0), (8, 1)]
    trips = fired("links-in-different-trips")
    assert [r for k, r in trips if k == 0] == [0, 2, 9] and [r for k, r in trips if k == 1] == [0, 2, 4, 6, 8, 9, 11]
    window = fired("chains-beyond-one-window")
    assert [(k, r - rs.WINDOW) for k, r in window if rs.WINDOW - 1 <= r <= rs.WINDOW + 1] == [(0, -1), (0, 1), (1, 0), (2, -1), (5, -1), (5, 1)]
    assert fired("clean-state-behind-a-failed-candidate") == [(0, 1), (8, 0), (11, 2), (12, 1)]
    assert fired("truncation-between-two-candidates") == [(0, 0), (0, 2), (0, 3), (1, 0), (1, 1), (1, 3), (2, 0), (2, 2), (2, 3)]


@pytest.mark.parametrize("platform", PLATFORMS, ids=[p[1] for p in PLATFORMS])
def test_a_set_without_relative_members_gives_the_list_of_rules_open_ex(workdir, platform):
    """the case table and the random cases of tests/rulecond_ref.py, members widened by {distance 0, within 0}"""
    cases = [(name, pats, rules, data, offsets, rc.is_nocase(name)) for name, pats, rules, data, offsets in rc.CASES]
    cases += [("seed %d" % s,) + tuple(rc.random_case(s)) + (False,) for s in rc.RANDOM_SEEDS]
    for name, pats, rules, data, offsets, nocase in cases:
        data = data.tobytes() if isinstance(data, np.ndarray) else data
        h = host_handle(pattern_file(workdir, "ruleseq_eq", pats), platform[0], api.PFACX_READ_NOCASE if nocase else 0)
        try:
            want = rc.fired_py(pats, rules, data, offsets, nocase)
            old = h.rulesOpenEx(*rc.csr(rules))
            new = h.rulesOpenSeq(*rs.csr(rs.widen(rules)))
            check_host(old, want, data, offsets, name + "/PFACX_rulesOpenEx")
            check_host(new, want, data, offsets, name + "/PFACX_rulesOpenSeq")
            ref.same(rs.fired_py(pats, rs.widen(rules), data, offsets, nocase), want, name + "/the two references")
            old.close()
            new.close()
        finally:
            h.destroy()


@pytest.mark.parametrize("platform", PLATFORMS, ids=[p[1] for p in PLATFORMS])
@pytest.mark.parametrize("seed", rs.RANDOM_SEEDS)
def test_random_cases(workdir, seed, platform):
    pats, rules, data, offsets = rs.random_case(seed)
    h = host_handle(pattern_file(workdir, "ruleseq_rnd%d" % seed, pats), platform[0])
    try:
        r = h.rulesOpenSeq(*rs.csr(rules))
        check_host(r, rs.fired_py(pats, rules, data.tobytes(), offsets), data, offsets, f"seed {seed}")
        r.close()
    finally:
        h.destroy()


def test_the_random_seeds_verify_candidates_both_ways():
    """on the reference alone: of the (segment, rule) pairs that pass the AND stage -- every member holds by itself -- at least a quarter fire
    and at least a quarter fail; otherwise the random cases show nothing"""
    candidates = fire = 0
    for seed in rs.RANDOM_SEEDS:
        pats, rules, data, offsets = rs.random_case(seed)
        passed = set(rc.pairs(rc.fired_py(pats, rs.and_stage(rules), data.tobytes(), offsets)))
        fired = set(rc.pairs(rs.fired_py(pats, rules, data.tobytes(), offsets)))
        assert fired <= passed, seed
        candidates += len(passed)
        fire += len(fired)
    assert candidates >= 1000
    assert 4 * fire >= candidates and 4 * (candidates - fire) >= candidates, (fire, candidates)


def test_truncation_between_a_failed_and_a_verified_candidate(workdir):
    name, pats, rules, data, offsets = rs.TRUNCATION
    want = rs.fired_py(pats, rules, data, offsets)
    h = host_handle(pattern_file(workdir, "ruleseq_trunc", pats))
    try:
        r = h.rulesOpenSeq(*rs.csr(rules))
        for capacity in range(1, want[0].size + 1):
            st, got, n = rc.host_fired(r, data, offsets, capacity)
            assert (st, n) == (0 if capacity == want[0].size else api.STATUS.OUTPUT_TRUNCATED, want[0].size)
            ref.same(got, (want[0][:capacity], want[1][:capacity], want[2]), f"capacity {capacity}")
        r.close()
    finally:
        h.destroy()


def test_open_refusals(workdir):
    pats = [b"a", b"b", b"c", b"a"] + [b"m%02d;" % i for i in range(33)]    # ids 1 and 4 are duplicate lines: both resolve to 4
    h = host_handle(pattern_file(workdir, "ruleseq_open", pats))
    bare = api.PFAC.createHostOnly()
    lib = api.load_library()
    try:
        def status(off, members, handle=h):
            return handle.rulesOpenSeq(np.array(off, dtype=np.int32), members, check=False).status

        assert status([0, 1], [S(1)], bare) == api.STATUS.PATTERNS_NOT_READY
        # everything PFACX_rulesOpenEx refuses
        assert status([0, 1], [S(0)]) == INVALID
        assert status([0, 1], [S(len(pats) + 1)]) == INVALID
        assert status([0, 0], [S(1)]) == INVALID
        assert status([1, 2], [S(1), S(2)]) == INVALID
        assert status([0, 2, 1], [S(1), S(2)]) == INVALID
        assert status([0], []) == INVALID
        assert status([0, 1], [S(1, NOT)]) == INVALID                       # a rule without a positive member
        off, mem = rs.csr([[S(1)]])
        out = C.c_void_p()
        assert lib.PFACX_rulesOpenSeq(h._h, None, mem.ctypes.data, 1, C.byref(out)) == INVALID
        assert lib.PFACX_rulesOpenSeq(h._h, off.ctypes.data, None, 1, C.byref(out)) == INVALID
        assert lib.PFACX_rulesOpenSeq(h._h, off.ctypes.data, mem.ctypes.data, 1, None) == INVALID
        assert lib.PFACX_rulesOpenSeq(h._h, off.ctypes.data, mem.ctypes.data, 1 << 24, C.byref(out)) == INVALID
        assert lib.PFACX_rulesOpenSeq(None, off.ctypes.data, mem.ctypes.data, 1, C.byref(out)) == api.STATUS.INVALID_HANDLE
        # 32 members: a rule without a relative member merges equal ones, a rule with one merges nothing
        many = [S(5 + i) for i in range(33)]
        assert status([0, 33], many) == INVALID
        assert status([0, 34], many[:32] + [S(7), S(9)]) == 0
        assert status([0, 32], many[:31] + [R(7)]) == 0
        assert status([0, 33], many[:31] + [R(7), S(9)]) == INVALID         # 33 members in the order given
        assert status([0, 33], [S(5)] + [R(6 + i) for i in range(32)]) == INVALID
        assert status([0, 32], [S(5)] + [R(6 + i) for i in range(31)]) == 0
        # an unknown flag bit
        assert status([0, 1], [S(1, 8)]) == INVALID
        assert status([0, 2], [S(1), R(2, 0, 0, 0x80000000)]) == INVALID
        assert h.rulesOpenEx(np.array([0, 2], dtype=np.int32), [(1, 0, 0, 0), (2, RELATIVE, 0, 0)], check=False).status == INVALID      # PFACX_rulesOpenEx does not know the flag
        # RELATIVE on the first member of a rule, also of a later rule
        assert status([0, 1], [R(1)]) == INVALID
        assert status([0, 2, 4], [S(1), R(2), R(1), S(2)]) == INVALID
        # RELATIVE together with NOT; a RELATIVE member behind a NOT member
        assert status([0, 2], [S(1), R(2, 0, 0, NOT)]) == INVALID
        assert status([0, 3], [S(1), S(2, NOT), R(3)]) == INVALID
        assert status([0, 3], [S(2, NOT), S(1), R(3)]) == 0
        # distance or within on a member without RELATIVE
        assert status([0, 1], [(1, 0, 0, 0, 1, 0)]) == INVALID
        assert status([0, 2], [S(1), (2, FROM_END, 0, 0, 0, 7)]) == INVALID
        assert status([0, 2], [S(1), (2, NOT, 0, 0, 3, 0)]) == INVALID
        # ids of duplicate lines resolve to the reported id inside a chain too
        good = h.rulesOpenSeq(*rs.csr([[S(1), R(2, 0, 1)]]))
        assert rc.host_fired(good, b"ab", None)[2] == 1 and rc.host_fired(good, b"a.b", None)[2] == 0
        good.close()
        off, mem = rs.csr([[S(2), R(3)]])
        good = h.rulesOpenSeq(off, mem)
        mem["pattern"][0] = 3                                               # the arrays were copied
        assert rc.host_fired(good, b"bc", None)[2] == 1
        good.close()
    finally:
        bare.destroy()
        h.destroy()


def test_a_chained_set_follows_its_pattern_set_and_its_handle(workdir):
    h = host_handle(pattern_file(workdir, "ruleseq_gen_a", [b"ab", b"b"]))
    try:
        r = h.rulesOpenSeq(*rs.csr([[S(1), R(2)]]))
        assert rc.host_fired(r, b"ab b", None)[2] == 1 and rc.host_fired(r, b"ab", None)[2] == 0
        h.readPatternFromFile(pattern_file(workdir, "ruleseq_gen_b", [b"zz", b"b", b"ab"]))
        assert rc.host_fired(r, b"ab b", None, capacity=4)[0] == INVALID    # the set belongs to the pattern set that has gone
        assert r.close() == 0
        h.rulesOpenSeq(*rs.csr([[S(1), R(2)]]))                             # left open: PFAC_destroy closes it
    finally:
        assert h.destroy() == 0
