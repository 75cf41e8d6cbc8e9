"""PFACX_rulesOpenEx -- negated and position-bounded rule members -- through PFACX_rulesMatchFromDevice and through PFACX_rulesMatchFromHost on the
GPU platform against the reference of tests/rulecond_ref.py: the case table of the host file, the cases sized by scan_rules.hip (more pairs than a
trip, more rules than a window, more touched rules than the list, more segments than the grid), the equivalence with PFACX_rulesOpen, the seeded
random cases, device offsets beyond the buffer and the memory accounting.  Every case also runs truncated at half its list and as a count query;
all arrays are poisoned, with guard words behind capacity and behind segFirst, and the input is compared after every call."""

import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import rulecond_ref as rc  # noqa: E402
from tests import rules_ref as ref  # noqa: E402
from tests.gpu_helpers import make_handle  # noqa: E402
from tests.spans_helpers import pattern_file  # noqa: E402

BLOCKS_PER_CU = 4                               # scan_rules.hip: the grid of a pass is at most this many blocks per compute unit
GUARD = 16
POISON = 0x5A5A5A5A5A5A5A5A
NOT, FROM_END, M = rc.NOT, rc.FROM_END, rc.M
assert (rc.WINDOW, rc.TOUCHED, rc.TRIP) == (api.PFACX_RULES_WINDOW, api.PFACX_RULES_TOUCHED, api.PFACX_RULES_BLOCK_PAIRS)


def as_array(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)


def gpu_handle(pf, flags=0):
    h = api.PFAC.create()
    h.readPatternFromFileEx(pf, flags)
    return h


def device_fired(r, data, offsets, capacity=None, null_arrays=False, in_offset=0):
    """match_device over poisoned device arrays with guard words -> (status, (seg, rule, segFirst), full count).  capacity None: the count query
    first, as a caller would; null_arrays: capacity 0 and no arrays.  The input must stay untouched, nothing may be written behind the list,
    capacity or segFirst"""
    data = as_array(data)
    n = int(data.size)
    d_in = torch.zeros(n + in_offset + 64, dtype=torch.uint8, device="cuda:0")
    d_in[in_offset:in_offset + n] = torch.from_numpy(data.copy()).to("cuda:0")
    segs = 1 if offsets is None else len(offsets) - 1
    d_off = None if offsets is None else torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")
    o_ptr = None if d_off is None else d_off.data_ptr()
    if capacity is None:
        _, capacity = r.match_device(d_in.data_ptr() + in_offset, n, o_ptr, segs, None, None, 0, None, check=False)
    d_seg = torch.full((capacity + GUARD,), -7, dtype=torch.int32, device="cuda:0")
    d_rule = torch.full((capacity + GUARD,), -7, dtype=torch.int32, device="cuda:0")
    d_first = torch.from_numpy(np.full(segs + 1 + GUARD, POISON, dtype=np.uint64).view(np.int64)).to("cuda:0")
    st, total = r.match_device(d_in.data_ptr() + in_offset, n, o_ptr, segs, None if null_arrays else d_seg.data_ptr(),
                               None if null_arrays else d_rule.data_ptr(), capacity, d_first.data_ptr(), check=False)
    torch.cuda.synchronize()
    seg, rule, first = d_seg.cpu().numpy(), d_rule.cpu().numpy(), d_first.cpu().numpy().view(np.uint64)
    k = min(total, capacity)
    assert np.all(seg[k:] == -7) and np.all(rule[k:] == -7), "wrote behind the list or behind capacity"
    assert np.all(first[segs + 1:] == POISON), "wrote behind segFirst"
    assert torch.equal(d_in[in_offset:in_offset + n].cpu(), torch.from_numpy(data.copy())), "the caller's input was modified"
    return st, (seg[:k].copy(), rule[:k].copy(), first[:segs + 1].copy()), total


def check_both_forms(r, want, data, offsets, what, in_offset=0):
    """the device form and the host form on the GPU platform: whole, truncated at half, count query"""
    rc.check_forms(lambda capacity, null: device_fired(r, data, offsets, capacity, null, in_offset), want, what + "/device form")
    rc.check_forms(lambda capacity, null: rc.host_fired(r, data, offsets, capacity, null), want, what + "/host form")


def run_case(workdir, case, in_offset=0):
    name, pats, rules, data, offsets = case
    nocase = rc.is_nocase(name)
    h = gpu_handle(pattern_file(workdir, "rulecond_" + name, pats), api.PFACX_READ_NOCASE if nocase else 0)
    try:
        r = h.rulesOpenEx(*rc.csr(rules))
        check_both_forms(r, rc.fired_py(pats, rules, data, offsets, nocase), data, offsets, name, in_offset)
        assert r.close() == 0
    finally:
        h.destroy()


@pytest.mark.parametrize("case", rc.CASES, ids=[c[0] for c in rc.CASES])
def test_every_case_of_the_host_file(workdir, case):
    run_case(workdir, case, in_offset=5 if len(case[0]) % 2 else 0)        # (5: a misaligned d_input)


def test_rules_beyond_one_window(workdir):
    """a pair whose only membership in window 0 fails its window test must still send the block on to window 1"""
    run_case(workdir, rc.window_case())


def test_more_touched_rules_than_the_list_holds(workdir):
    """the sweep over the whole table, with m == need and negated bits in it"""
    run_case(workdir, rc.touched_case())


def test_what_a_segment_leaves_behind_in_its_block(workdir):
    """more segments than the grid has blocks: segment 0 sets only a negated bit and half a rule; segment `grid` is the same block's next one"""
    probe = gpu_handle(pattern_file(workdir, "rulecond_probe", [b"x"]))
    grid = int(probe.info().multiProcessorCount) * BLOCKS_PER_CU
    probe.destroy()
    case = rc.clean_state_case(grid)
    want = rc.pairs(rc.fired_py(*case[1:]))
    assert want == [(grid, 1), (grid, 2), (grid + 4, 0)]
    run_case(workdir, case)


PLAIN = [c[0] for c in ref.CASES] + ["seed %d" % s for s in ref.RANDOM_SEEDS]


@pytest.mark.parametrize("which", range(len(PLAIN)), ids=PLAIN)
def test_members_without_conditions_give_the_list_of_rules_open(workdir, which):
    if which < len(ref.CASES):
        name, pats, rules, data, offsets = ref.CASES[which]
    else:
        name, (pats, rules, data, offsets) = PLAIN[which], ref.random_case(ref.RANDOM_SEEDS[which - len(ref.CASES)])
    nocase = ref.is_nocase(name)
    h = gpu_handle(pattern_file(workdir, "rulecond_eq", pats), api.PFACX_READ_NOCASE if nocase else 0)
    try:
        want = ref.fired_py(pats, rules, bytes(as_array(data)), offsets, nocase)
        old = h.rulesOpen(*ref.csr(rules))
        new = h.rulesOpenEx(*rc.csr(rc.plain(rules)))
        st, got, n = device_fired(old, data, offsets)
        assert (st, n) == (0, want[0].size)
        ref.same(got, want, name + "/PFACX_rulesOpen")
        check_both_forms(new, want, data, offsets, name + "/PFACX_rulesOpenEx")
        old.close()
        new.close()
    finally:
        h.destroy()


@pytest.mark.parametrize("seed", rc.RANDOM_SEEDS)
def test_random_cases(workdir, seed):
    pats, rules, data, offsets = rc.random_case(seed)
    h = gpu_handle(pattern_file(workdir, "rulecond_rnd%d" % seed, pats))
    try:
        r = h.rulesOpenEx(*rc.csr(rules))
        check_both_forms(r, rc.fired_py(pats, rules, data.tobytes(), offsets), data, offsets, f"seed {seed}", in_offset=seed % 4)
        r.close()
    finally:
        h.destroy()


def test_random_cases_on_the_hashed_table_and_the_naive_kernel(workdir):
    for seed, perf, tex, variant in ((1, api.PFAC_SPACE_DRIVEN, api.PFAC_TEXTURE_ON, api.PFACX_KERNEL_FILTER),
                                     (5, api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_NAIVE)):
        pats, rules, data, offsets = rc.random_case(seed)
        h = make_handle(pattern_file(workdir, "rulecond_rnd%d" % seed, pats), perf, tex, variant)
        try:
            r = h.rulesOpenEx(*rc.csr(rules))
            want = rc.fired_py(pats, rules, data.tobytes(), offsets)
            rc.check_forms(lambda capacity, null: device_fired(r, data, offsets, capacity, null), want, f"seed {seed}")
            r.close()
        finally:
            h.destroy()


def test_device_offsets_beyond_the_buffer_are_clamped(workdir):
    """a last offset beyond `size` gives the list of the offsets clamped to `size`: the segment's end, which a window from the end is measured
    from, is the clamped one"""
    pats = [b"abc", b"zz"]
    rules = [[M(1, FROM_END, 0, 3)], [M(1, FROM_END, 1, 0)], [M(1), M(2, NOT | FROM_END, 0, 2)], [M(1, 0, 4, 5)]]
    data, offsets = ref.cut(rc.at(4), rc.at(9), b"zz" + rc.at(7, n=10))
    n = len(data)
    want = rc.fired_py(pats, rules, data, offsets)
    assert rc.pairs(want) == [(0, 1), (0, 2), (0, 3), (1, 0), (1, 2), (2, 0), (2, 2)]
    h = gpu_handle(pattern_file(workdir, "rulecond_clamp", pats))
    try:
        r = h.rulesOpenEx(*rc.csr(rules))
        for last in (n + 1, n + 100, 2 ** 40, 2 ** 64 - 1):
            st, got, total = device_fired(r, data, np.array(offsets[:-1] + [last], dtype=np.uint64))
            assert (st, total) == (0, want[0].size)
            ref.same(got, want, f"last offset {last}")
        for hostile in ([0, n, n // 2, 5, n], [n + 100, 2 ** 40, 0, n], [7, 3, 2 ** 63, 1, 0], [n, n, n, n]):      # whatever the list: inside the arrays
            st, _, total = device_fired(r, data, np.array(hostile, dtype=np.uint64))
            assert st == 0 and total <= len(rules) * (len(hostile) - 1)
        r.close()
    finally:
        h.destroy()


def test_memory_accounting(workdir):
    """a conditioned set adds 8 bytes per member after resolution to its device tables; a plain one nothing"""
    pats = [b"ab", b"b", b"abc", b"ab"]
    ids = [[1, 2], [3], [4, 2, 2], [2]]                                     # I = 6 ids after resolution: {2, 4}, {3}, {2, 4}, {2}
    members = [[M(1, 0, 0, 2), M(2, NOT)], [M(3)], [M(4, 0, 0, 2), M(1, 0, 0, 2), M(2, FROM_END)], [M(2)]]         # I = 6 members: 1 and 4 are one pattern
    data = as_array(b"abc ab b " * 100)
    h = gpu_handle(pattern_file(workdir, "rulecond_mem", pats))
    try:
        h.trim()
        tables0 = int(h.info().deviceTableBytes)
        plain_bytes = 4 * (len(pats) + 2) + 4 * 6 + 4 * 4
        for opened, extra in ((h.rulesOpen(*ref.csr(ids)), 0), (h.rulesOpenEx(*rc.csr(members)), 8 * 6)):
            assert int(h.info().deviceTableBytes) == tables0                # nothing on the device before the first device call
            device_fired(opened, data, None)                                # (no offsets: a conditioned set stages the pattern lengths all the same)
            assert int(h.info().deviceTableBytes) == tables0 + plain_bytes + extra
            h.trim()                                                        # the scratch goes, the rule tables stay
            assert int(h.info().deviceTableBytes) == tables0 + plain_bytes + extra
            opened.close()
            assert int(h.info().deviceTableBytes) == tables0
        r = h.rulesOpenEx(*rc.csr(members))
        want = rc.fired_py(pats, members, bytes(data), None)
        rc.check_forms(lambda capacity, null: device_fired(r, data, None, capacity, null), want, "after trim")
        r.close()
    finally:
        h.destroy()


def test_example_program_passes_its_self_check():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-C", os.path.join(root, "examples"), "rulecond_example"], check=True, stdout=subprocess.PIPE)
    p = subprocess.run([os.path.join(root, "examples", "rulecond_example")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    assert b"self-check passed" in p.stdout and b"(device form)" in p.stdout
