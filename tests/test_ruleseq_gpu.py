"""PFACX_rulesOpenSeq -- ordered rule members with distance and within -- through PFACX_rulesMatchFromDevice and through PFACX_rulesMatchFromHost on
the GPU platform against the reference of tests/ruleseq_ref.py: the case table of the host file (greedy traps, bounds, links in different trips of
the kernel), the cases sized by scan_rules.hip (chain rules on both sides of a window's border, more candidates than the touched list holds with
failed ones among them, more segments than the grid, a truncation between a failed and a verified candidate), the equivalence with
PFACX_rulesOpenEx, the seeded random cases, device offsets beyond the buffer and the memory accounting.  Every case also runs truncated at half
its list and as a count query; all arrays are poisoned, with guard words behind capacity and behind segFirst, and the input is compared after
every call (the helpers of tests/test_rulecond_gpu.py)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import rulecond_ref as rc  # noqa: E402
from tests import rules_ref as ref  # noqa: E402
from tests import ruleseq_ref as rs  # noqa: E402
from tests.spans_helpers import pattern_file  # noqa: E402
from tests.test_rulecond_gpu import BLOCKS_PER_CU, as_array, check_both_forms, device_fired, gpu_handle  # noqa: E402

NOT, FROM_END, S, R = rs.NOT, rs.FROM_END, rs.S, rs.R
assert (rs.WINDOW, rs.TOUCHED, rs.TRIP) == (api.PFACX_RULES_WINDOW, api.PFACX_RULES_TOUCHED, api.PFACX_RULES_BLOCK_PAIRS)


def round256(n):
    return (n + 255) & ~255


def run_case(workdir, case, in_offset=0):
    name, pats, rules, data, offsets = case
    nocase = rs.is_nocase(name)
    h = gpu_handle(pattern_file(workdir, "ruleseq_" + name, pats), api.PFACX_READ_NOCASE if nocase else 0)
    try:
        r = h.rulesOpenSeq(*rs.csr(rules))
        check_both_forms(r, rs.fired_py(pats, rules, data, offsets, nocase), data, offsets, name, in_offset)
        assert r.close() == 0
    finally:
        h.destroy()


@pytest.mark.parametrize("case", rs.CASES, ids=[c[0] for c in rs.CASES])
def test_every_case_of_the_host_file(workdir, case):
    run_case(workdir, case, in_offset=5 if len(case[0]) % 2 else 0)        # (5: a misaligned d_input)


def test_chain_rules_on_both_sides_of_a_window_border(workdir):
    run_case(workdir, rs.window_case())


def test_more_candidates_than_the_touched_list_holds_and_failed_ones_among_them(workdir):
    """the sweep over the whole table; in every word of the bitmap a verified candidate next to a failed one"""
    run_case(workdir, rs.touched_case())


def test_what_a_failed_candidate_leaves_behind_in_its_block(workdir):
    """more segments than the grid has blocks: segment 0 leaves a failed candidate; segment `grid` is the same block's next one"""
    probe = gpu_handle(pattern_file(workdir, "ruleseq_probe", [b"x"]))
    grid = int(probe.info().multiProcessorCount) * BLOCKS_PER_CU
    probe.destroy()
    case = rs.clean_state_case(grid)
    assert rc.pairs(rs.fired_py(*case[1:])) == [(0, 1), (grid, 0), (grid + 3, 2), (grid + 4, 1)]
    run_case(workdir, case)


def test_truncation_between_a_failed_and_a_verified_candidate(workdir):
    name, pats, rules, data, offsets = rs.TRUNCATION
    want = rs.fired_py(pats, rules, data, offsets)
    h = gpu_handle(pattern_file(workdir, "ruleseq_trunc", pats))
    try:
        r = h.rulesOpenSeq(*rs.csr(rules))
        for capacity in range(1, want[0].size + 1):
            st, got, n = device_fired(r, data, offsets, capacity)
            assert (st, n) == (0 if capacity == want[0].size else api.STATUS.OUTPUT_TRUNCATED, want[0].size)
            ref.same(got, (want[0][:capacity], want[1][:capacity], want[2]), f"capacity {capacity}")
        r.close()
    finally:
        h.destroy()


EQUIVALENT = [c[0] for c in rc.CASES] + ["seed %d" % s for s in rc.RANDOM_SEEDS[:6]]


@pytest.mark.parametrize("which", range(len(EQUIVALENT)), ids=EQUIVALENT)
def test_a_set_without_relative_members_gives_the_list_of_rules_open_ex(workdir, which):
    if which < len(rc.CASES):
        name, pats, rules, data, offsets = rc.CASES[which]
    else:
        name, (pats, rules, data, offsets) = EQUIVALENT[which], rc.random_case(rc.RANDOM_SEEDS[which - len(rc.CASES)])
    nocase = rc.is_nocase(name)
    h = gpu_handle(pattern_file(workdir, "ruleseq_eq", pats), api.PFACX_READ_NOCASE if nocase else 0)
    try:
        want = rc.fired_py(pats, rules, bytes(as_array(data)), offsets, nocase)
        old = h.rulesOpenEx(*rc.csr(rules))
        new = h.rulesOpenSeq(*rs.csr(rs.widen(rules)))
        st, got, n = device_fired(old, data, offsets)
        assert (st, n) == (0, want[0].size)
        ref.same(got, want, name + "/PFACX_rulesOpenEx")
        check_both_forms(new, want, data, offsets, name + "/PFACX_rulesOpenSeq")
        old.close()
        new.close()
    finally:
        h.destroy()


@pytest.mark.parametrize("seed", rs.RANDOM_SEEDS)
def test_random_cases(workdir, seed):
    pats, rules, data, offsets = rs.random_case(seed)
    h = gpu_handle(pattern_file(workdir, "ruleseq_rnd%d" % seed, pats))
    try:
        r = h.rulesOpenSeq(*rs.csr(rules))
        check_both_forms(r, rs.fired_py(pats, rules, data.tobytes(), offsets), data, offsets, f"seed {seed}", in_offset=seed % 4)
        r.close()
    finally:
        h.destroy()


def test_device_offsets_beyond_the_buffer_are_clamped(workdir):
    """a last offset beyond `size` gives the list of the offsets clamped to `size`; hostile offsets may give a wrong list, but no guard word
    changes (device_fired asserts it)"""
    pats = [b"ab", b"cd"]
    rules = [[S(1), R(2, 0, 0, FROM_END, 0, 2)], [S(1), R(2, 1, 5)], [S(2), R(1), S(1, NOT, 0, 2)]]
    data, offsets = ref.cut(b"ab.cd", b"cd.ab", b"ab cd ab cd")
    n = len(data)
    want = rs.fired_py(pats, rules, data, offsets)
    assert rc.pairs(want) == [(0, 0), (0, 1), (1, 2), (2, 0), (2, 1)]
    h = gpu_handle(pattern_file(workdir, "ruleseq_clamp", pats))
    try:
        r = h.rulesOpenSeq(*rs.csr(rules))
        for last in (n + 1, n + 100, 2 ** 40, 2 ** 64 - 1):
            st, got, total = device_fired(r, data, np.array(offsets[:-1] + [last], dtype=np.uint64))
            assert (st, total) == (0, want[0].size)
            ref.same(got, want, f"last offset {last}")
        for hostile in ([0, n, n // 2, 5, n], [n + 100, 2 ** 40, 0, n], [7, 3, 2 ** 63, 1, 0], [n, n, n, n], [0, 3, 1, n, 2, n]):
            st, _, total = device_fired(r, data, np.array(hostile, dtype=np.uint64))
            assert st == 0 and total <= len(rules) * (len(hostile) - 1)
        r.close()
    finally:
        h.destroy()


def test_memory_accounting(workdir):
    """a set with chains adds 4 (R + 1) + 20 K bytes to its device tables at the first device call -- K the members of all chains -- and a call of
    it 8 bytes per pair of the scan, each of the two arrays rounded up to 256, to the handle's scratch; a set without chains adds neither;
    PFACX_trim gives the scratch back and keeps the tables, PFACX_rulesClose frees them"""
    pats = [b"ab", b"b", b"abc"]
    chained = [[S(1, 0, 0, 2), R(2), S(3, NOT)], [S(3)], [S(2), R(1, 1, 8), R(2)]]              # I = 7 members, K = 5 of them in chains
    unchained = [[S(1, 0, 0, 2), S(2), S(3, NOT)], [S(3)], [S(2), S(1), S(2)]]                    # I = 6: the equal members of rule 2 merge
    data = as_array(b"ab b ab. " * 100)
    text = bytes(data)
    found = sum(any(text.startswith(p, i) for p in pats) for i in range(len(text)))              # the longest pairs: one per position a pattern starts at
    assert found == 500
    assert rs.links(chained) == 5 and rs.links(unchained) == 0
    h = gpu_handle(pattern_file(workdir, "ruleseq_mem", pats))
    try:
        h.trim()
        tables0, scratch0 = int(h.info().deviceTableBytes), int(h.info().deviceScratchBytes)
        scratch = {}
        for name, rules, members, extra in (("unchained", unchained, 6, 0), ("chained", chained, 7, 4 * (3 + 1) + 20 * 5)):
            opened = h.rulesOpenSeq(*rs.csr(rules))
            assert int(h.info().deviceTableBytes) == tables0                # nothing on the device before the first device call
            device_fired(opened, data, None)
            tables = tables0 + 4 * (len(pats) + 2) + 4 * members + 4 * 3 + 8 * members + extra
            assert int(h.info().deviceTableBytes) == tables
            scratch[name] = int(h.info().deviceScratchBytes)
            h.trim()                                                        # the scratch goes, the tables of the set stay
            assert int(h.info().deviceTableBytes) == tables
            assert int(h.info().deviceScratchBytes) == scratch0
            opened.close()
            assert int(h.info().deviceTableBytes) == tables0
        assert scratch["chained"] - scratch["unchained"] == 2 * round256(4 * found)
        r = h.rulesOpenSeq(*rs.csr(chained))
        want = rs.fired_py(pats, chained, bytes(data), None)
        rc.check_forms(lambda capacity, null: device_fired(r, data, None, capacity, null), want, "after trim")
        r.close()
    finally:
        h.destroy()
