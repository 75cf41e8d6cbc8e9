"""PFACX_rulesOpenEx -- negated and position-bounded rule members -- through PFACX_rulesMatchFromHost on the CPU platforms (host-only handles: no
device needed) against the reference of tests/rulecond_ref.py, which never calls the library: the case table (window edges in both directions, the
chain member that decides, second segments and a border, negation, 32 members, more pairs than a trip of the kernel, a caseless set), the cases
sized by the kernel's window, touched list and grid, the equivalence with PFACX_rulesOpen over every case of tests/rules_ref.py, the seeded random
cases and every refusal of the contract.  Every case also runs truncated at half its list and as a count query."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pfac_amd import api
from tests import rulecond_ref as rc
from tests import rules_ref as ref
from tests.spans_helpers import pattern_file

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
INVALID = api.STATUS.INVALID_PARAMETER
NOT, FROM_END, M = rc.NOT, rc.FROM_END, rc.M
BUILT = [rc.window_case(), rc.touched_case(), rc.clean_state_case(8)]


def host_handle(pf, platform=api.PFAC_PLATFORM_CPU, flags=0):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    h.readPatternFromFileEx(pf, flags)
    return h


def check_host(r, want, data, offsets, what):
    rc.check_forms(lambda capacity, null: rc.host_fired(r, data, offsets, capacity, null), want, what)


def test_the_binding_matches_the_header():
    assert (api.PFACX_RULE_NOT, api.PFACX_RULE_FROM_END) == (NOT, FROM_END)
    assert api.rule_member_dtype() == rc.MEMBER and rc.MEMBER.itemsize == 16


@pytest.mark.parametrize("platform", PLATFORMS, ids=[p[1] for p in PLATFORMS])
@pytest.mark.parametrize("case", rc.CASES + BUILT, ids=[c[0] for c in rc.CASES + BUILT])
def test_case_table(workdir, case, platform):
    name, pats, rules, data, offsets = case
    nocase = rc.is_nocase(name)
    h = host_handle(pattern_file(workdir, "rulecond_" + name, pats), platform[0], api.PFACX_READ_NOCASE if nocase else 0)
    try:
        r = h.rulesOpenEx(*rc.csr(rules))
        want = rc.fired_py(pats, rules, data, offsets, nocase)
        check_host(r, want, data, offsets, name)
        ref.same(r.match_host_array(np.frombuffer(data, dtype=np.uint8), offsets), want, name + "/match_host_array")
        assert r.close() == 0
    finally:
        h.destroy()


def test_the_cases_say_what_the_issue_says():
    """the reference itself, on the cases whose answer the contract spells out"""
    by = {c[0]: c for c in rc.CASES + BUILT}

    def fired(name):
        _, pats, rules, data, offsets = by[name]
        return rc.pairs(rc.fired_py(pats, rules, data, offsets, rc.is_nocase(name)))

    edges = fired("window-edges")
    seg_of = {s: k for k, s in enumerate(rc.EDGE_STARTS)}
    for rule, starts in ((0, [4, 5, 6]), (1, [3, 4, 5]), (2, [4, 5, 6, 7, 9]), (3, []), (4, [0]), (5, [9]), (6, []), (7, []),
                         (8, rc.EDGE_STARTS), (9, rc.EDGE_STARTS[1:]), (10, [0, 1, 2, 3, 4, 5])):
        assert [k for k, r in edges if r == rule] == [seg_of[s] for s in starts], rule
    assert fired("chain-member-decides") == [(0, 0), (0, 2), (0, 3)]        # {GET, depth 3} fires, {GET /admin, depth 3} does not
    assert fired("second-segment-and-a-border") == [(0, 0), (0, 3), (2, 2), (4, 1), (5, 0)]      # `bor` ends segment 0; `border` only in segment 4
    negation = fired("negation")
    assert [k for k, r in negation if r == 0] == [0, 2, 4, 7]               # absent; in the neighbouring segment only; never where `bad` is
    assert [k for k, r in negation if r == 1] == [0, 1, 2, 4, 7]            # `bad` at 3: outside {0, 3}
    assert [k for k, r in negation if r == 2] == [0, 1]                     # starts with ok and does not end with it
    assert [r for k, r in negation if k in (3, 9)] == []                    # only negated bits touched
    assert [k for k, r in negation if r == 4] == []                         # a contradiction never fires
    assert fired("thirty-two-members-5-negated") == [(0, 0), (0, 1), (1, 1)]
    assert fired("beyond-one-trip-one-segment") == [(0, 1)]
    window = fired("beyond-one-window")
    assert [(k, r) for k, r in window if r in (8191, 8192, 8199)] == [(0, 8192), (0, 8199), (1, 8191), (1, 8199), (2, 8192)]
    assert fired("clean-state") == [(8, 1), (8, 2), (12, 0)]
    assert fired("nocase-window") == [(0, 0), (1, 1), (2, 2), (3, 1), (3, 2)]


@pytest.mark.parametrize("platform", PLATFORMS, ids=[p[1] for p in PLATFORMS])
def test_members_without_conditions_give_the_list_of_rules_open(workdir, platform):
    cases = [(name, pats, rules, data, offsets, ref.is_nocase(name)) for name, pats, rules, data, offsets in ref.CASES]
    cases += [("seed %d" % s,) + tuple(ref.random_case(s)) + (False,) for s in ref.RANDOM_SEEDS]
    for name, pats, rules, data, offsets, nocase in cases:
        data = data.tobytes() if isinstance(data, np.ndarray) else data
        h = host_handle(pattern_file(workdir, "rulecond_eq", pats), platform[0], api.PFACX_READ_NOCASE if nocase else 0)
        try:
            want = ref.fired_py(pats, rules, data, offsets, nocase)
            old = h.rulesOpen(*ref.csr(rules))
            new = h.rulesOpenEx(*rc.csr(rc.plain(rules)))
            ref.same(old.match_host_array(np.frombuffer(data, dtype=np.uint8), offsets), want, name + "/PFACX_rulesOpen")
            check_host(new, want, data, offsets, name + "/PFACX_rulesOpenEx")
            ref.same(rc.fired_py(pats, rc.plain(rules), data, offsets, nocase), want, name + "/the two references")
            old.close()
            new.close()
        finally:
            h.destroy()


@pytest.mark.parametrize("platform", PLATFORMS, ids=[p[1] for p in PLATFORMS])
@pytest.mark.parametrize("seed", rc.RANDOM_SEEDS)
def test_random_cases(workdir, seed, platform):
    pats, rules, data, offsets = rc.random_case(seed)
    h = host_handle(pattern_file(workdir, "rulecond_rnd%d" % seed, pats), platform[0])
    try:
        r = h.rulesOpenEx(*rc.csr(rules))
        check_host(r, rc.fired_py(pats, rules, data.tobytes(), offsets), data, offsets, f"seed {seed}")
        r.close()
    finally:
        h.destroy()


def test_every_capacity_of_a_conditioned_list(workdir):
    """the list frame at its edges for a conditioned set: an empty first, middle and last segment and every capacity from 0 to the length of the
    list + 1 -- inside a segment, exactly at a segment's border (segFirst = 0, 0, 2, 2, 4, 4), the length - 1, the length itself"""
    pats = [b"a", b"aa", b"aaa", b"b", b"ab"]
    rules = [[M(1, 0, 0, 1)], [M(4, FROM_END, 0, 1), M(3, NOT)], [M(2, 0, 1), M(5, NOT | FROM_END, 1)]]
    data, offsets = ref.cut(b"", b"aaab", b"", b"baab", b"")
    want = rc.fired_py(pats, rules, data, offsets)
    assert rc.pairs(want) == [(1, 0), (1, 2), (3, 1), (3, 2)] and want[2].tolist() == [0, 0, 2, 2, 4, 4]
    total = int(want[0].size)
    h = host_handle(pattern_file(workdir, "rulecond_caps", pats))
    try:
        r = h.rulesOpenEx(*rc.csr(rules))
        for capacity in range(total + 2):
            st, got, n = rc.host_fired(r, data, offsets, capacity)
            assert (st, n) == (api.STATUS.OUTPUT_TRUNCATED if capacity < total else 0, total), f"capacity {capacity}"
            ref.same(got, (want[0][:capacity], want[1][:capacity], want[2]), f"capacity {capacity}")
        r.close()
    finally:
        h.destroy()


def test_the_random_seeds_fire_and_exercise_both_polarities_and_both_directions():
    """on the reference alone: three quarters of the seeds fire something; among the fired rules some have a negated member and some a window from
    the end; some rule is kept from firing by its negated members alone, some by its windows alone"""
    fire = with_not = with_end = vetoed = windowed = 0
    for seed in rc.RANDOM_SEEDS:
        pats, rules, data, offsets = rc.random_case(seed)
        got = set(rc.pairs(rc.fired_py(pats, rules, data.tobytes(), offsets)))
        fire += bool(got)
        fired_rules = {r for _, r in got}
        with_not += any(f & NOT for r in fired_rules for _, f, _, _ in rules[r])
        with_end += any(f & FROM_END for r in fired_rules for _, f, _, _ in rules[r])
        positive = [[m for m in rule if not m[1] & NOT] for rule in rules]
        vetoed += bool(set(rc.pairs(rc.fired_py(pats, positive, data.tobytes(), offsets))) - got)
        anywhere = [[M(i, f & NOT) for i, f, _, _ in rule if not f & NOT] for rule in rules]
        windowed += bool(set(rc.pairs(rc.fired_py(pats, anywhere, data.tobytes(), offsets))) - set(rc.pairs(rc.fired_py(pats, positive, data.tobytes(), offsets))))
    assert 4 * fire >= 3 * len(rc.RANDOM_SEEDS), fire
    assert min(with_not, with_end, vetoed, windowed) >= len(rc.RANDOM_SEEDS) // 4, (with_not, with_end, vetoed, windowed)


def test_open_refusals(workdir):
    pats = [b"a", b"b", b"c", b"a"] + [b"m%02d;" % i for i in range(33)]    # ids 1 and 4 are duplicate lines: both resolve to 4
    h = host_handle(pattern_file(workdir, "rulecond_open", pats))
    bare = api.PFAC.createHostOnly()
    lib = api.load_library()
    try:
        def status(off, members, handle=h):
            return handle.rulesOpenEx(np.array(off, dtype=np.int32), members, check=False).status

        assert status([0, 1], [M(1)], bare) == api.STATUS.PATTERNS_NOT_READY
        # everything PFACX_rulesOpen refuses
        assert status([0, 1], [M(0)]) == INVALID                            # an id below 1
        assert status([0, 1], [M(len(pats) + 1)]) == INVALID                # an id above F
        assert status([0, 0], [M(1)]) == INVALID                            # an empty rule
        assert status([1, 2], [M(1), M(2)]) == INVALID                      # offsets that do not start at 0
        assert status([0, 2, 1], [M(1), M(2)]) == INVALID                   # offsets that decrease
        assert status([0], []) == INVALID                                   # no rule
        off, mem = rc.csr([[M(1)]])
        out = C.c_void_p()
        assert lib.PFACX_rulesOpenEx(h._h, None, mem.ctypes.data, 1, C.byref(out)) == INVALID
        assert lib.PFACX_rulesOpenEx(h._h, off.ctypes.data, None, 1, C.byref(out)) == INVALID
        assert lib.PFACX_rulesOpenEx(h._h, off.ctypes.data, mem.ctypes.data, 1, None) == INVALID
        assert lib.PFACX_rulesOpenEx(h._h, off.ctypes.data, mem.ctypes.data, 1 << 24, C.byref(out)) == INVALID
        assert lib.PFACX_rulesOpenEx(None, off.ctypes.data, mem.ctypes.data, 1, C.byref(out)) == api.STATUS.INVALID_HANDLE
        # more than 32 distinct members: 33 patterns; 33 windows of one pattern; 32 are fine
        many = [M(5 + i) for i in range(33)]
        assert status([0, 33], many) == INVALID
        assert status([0, 33], [M(2, 0, i, 0) for i in range(33)]) == INVALID
        assert status([0, 32], many[:32]) == 0 and status([0, 32], [M(2, 0, i, 0) for i in range(32)]) == 0
        # equal members count once, and ids of duplicate lines resolve before that: 34 members, 32 distinct
        assert status([0, 34], many[:32] + [M(7), M(9)]) == 0
        assert status([0, 34], many[:31] + [M(1, 0, 2, 3), M(4, 0, 2, 3), M(4, 0, 2, 3)]) == 0
        assert status([0, 33], many[:31] + [M(1, 0, 2, 3), M(4, 0, 2, 4)]) == INVALID         # another window: another member
        assert status([0, 33], many[:31] + [M(1, 0, 2, 3), M(4, NOT, 2, 3)]) == INVALID       # another polarity too
        # an unknown flag bit
        assert status([0, 1], [M(1, 4)]) == INVALID
        assert status([0, 2], [M(1), M(2, 0x80000000)]) == INVALID
        assert status([0, 1], [M(1, NOT | FROM_END | 8)]) == INVALID
        # a rule without a positive member, wherever it stands
        assert status([0, 1], [M(1, NOT)]) == INVALID
        assert status([0, 1, 3], [M(1), M(2, NOT), M(3, NOT | FROM_END, 1, 2)]) == INVALID
        assert status([0, 2], [M(1, NOT), M(1, FROM_END)]) == 0
        good = h.rulesOpenEx(off, mem)
        mem["pattern"][0] = 3                                               # the arrays were copied
        assert rc.host_fired(good, b"a", None)[2] == 1
        good.close()
    finally:
        bare.destroy()
        h.destroy()


def test_a_conditioned_set_follows_its_pattern_set_and_its_handle(workdir):
    h = host_handle(pattern_file(workdir, "rulecond_gen_a", [b"ab", b"b"]))
    try:
        r = h.rulesOpenEx(*rc.csr([[M(1, 0, 0, 2), M(2, NOT, 2, 0)]]))
        assert rc.host_fired(r, b"ab", None)[2] == 1 and rc.host_fired(r, b"abb", None)[2] == 0
        h.readPatternFromFile(pattern_file(workdir, "rulecond_gen_b", [b"zz", b"b", b"ab"]))
        assert rc.host_fired(r, b"ab", None, capacity=4)[0] == INVALID      # the set belongs to the pattern set that has gone
        assert r.close() == 0
        h.rulesOpenEx(*rc.csr([[M(1)]]))                                    # left open: PFAC_destroy closes it
    finally:
        assert h.destroy() == 0


def test_example_program_on_its_host_path():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-C", os.path.join(root, "examples"), "rulecond_example"], check=True, stdout=subprocess.PIPE)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")          # no GPU visible: the host form
    p = subprocess.run([os.path.join(root, "examples", "rulecond_example")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
    assert p.returncode == 0, p.stderr.decode()
    assert b"self-check passed" in p.stdout and b"(host form)" in p.stdout
    assert p.stdout.decode().splitlines()[:5] == ["record 0: rule payment-error", "record 3: rule admin-from-outside", "record 3: rule ends-in-401",
                                                  "record 5: rule get-not-first", "record 6: rule ends-in-401"]
