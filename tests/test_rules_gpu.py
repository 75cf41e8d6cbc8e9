"""PFACX_rulesMatchFromDevice and PFACX_rulesMatchFromHost on the GPU platform against the reference of tests/rules_ref.py: every case of the host
file at two alignments, the random cases in every kernel variant and mode, rule counts around the window of scan_rules.hip, segments that touch
exactly the touched list, one rule more, and fewer right behind it in the same block, a segment of more pairs than a block takes in one go, more
segments than the grid has blocks, empty and one-byte segments, one input above the 32 MiB switch, truncation of a long list, hostile offsets, the
memory accounting and the example program.  All arrays are poisoned, with guard words behind capacity and behind segFirst; the input is compared
after every call."""

import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import rules_ref as ref  # noqa: E402
from tests.gpu_helpers import MODES, VARIANTS, make_handle  # noqa: E402
from tests.spans_helpers import pattern_file  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, TOUCHED, BLOCK_PAIRS = api.PFACX_RULES_WINDOW, api.PFACX_RULES_TOUCHED, api.PFACX_RULES_BLOCK_PAIRS
BLOCKS_PER_CU = 4                               # scan_rules.hip: the grid of a pass is at most this many blocks per compute unit
INVALID, TRUNCATED = api.STATUS.INVALID_PARAMETER, api.STATUS.OUTPUT_TRUNCATED
GUARD = 16
POISON = 0x5A5A5A5A5A5A5A5A


def as_array(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)


def gpu_handle(pf, flags=0, variant=api.PFACX_KERNEL_AUTO, perf=api.PFAC_TIME_DRIVEN, tex=api.PFAC_TEXTURE_OFF):
    h = api.PFAC.create()
    h.setPerfMode(perf)
    h.setTextureMode(tex)
    h.setKernelVariant(variant)
    h.readPatternFromFileEx(pf, flags)
    return h


def device_fired(r, data, offsets, capacity=None, in_offset=0, seg_first=True):
    """match_device over poisoned device arrays with guard words -> (status, (seg, rule, segFirst), full count).  capacity None: the count query
    first, with null arrays, as a caller would.  The input must stay untouched, nothing may be written behind the list, capacity or segFirst"""
    data = as_array(data)
    n = int(data.size)
    d_in = torch.zeros(n + in_offset + 64, dtype=torch.uint8, device="cuda:0")
    d_in[in_offset:in_offset + n] = torch.from_numpy(data.copy()).to("cuda:0")
    segs = 1 if offsets is None else len(offsets) - 1
    d_off = None if offsets is None else torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")
    o_ptr = None if d_off is None else d_off.data_ptr()
    if capacity is None:
        st, capacity = r.match_device(d_in.data_ptr() + in_offset, n, o_ptr, segs, None, None, 0, None, check=False)
        assert st in (0, TRUNCATED) and (st == TRUNCATED) == (capacity > 0)
    d_seg = torch.full((capacity + GUARD,), -7, dtype=torch.int32, device="cuda:0")
    d_rule = torch.full((capacity + GUARD,), -7, dtype=torch.int32, device="cuda:0")
    d_first = torch.from_numpy(np.full(segs + 1 + GUARD, POISON, dtype=np.uint64).view(np.int64)).to("cuda:0")
    st, total = r.match_device(d_in.data_ptr() + in_offset, n, o_ptr, segs, d_seg.data_ptr(), d_rule.data_ptr(), capacity,
                               d_first.data_ptr() if seg_first else None, check=False)
    torch.cuda.synchronize()
    seg, rule, first = d_seg.cpu().numpy(), d_rule.cpu().numpy(), d_first.cpu().numpy().view(np.uint64)
    k = min(total, capacity)
    assert np.all(seg[k:] == -7) and np.all(rule[k:] == -7), "wrote behind the list or behind capacity"
    assert np.all(first[segs + 1:] == POISON), "wrote behind segFirst"
    if not seg_first:
        assert np.all(first == POISON), "wrote a segFirst that was not given"
    assert torch.equal(d_in[in_offset:in_offset + n].cpu(), torch.from_numpy(data.copy())), "the caller's input was modified"
    return st, (seg[:k].copy(), rule[:k].copy(), first[:segs + 1].copy()), total


def check_device(r, want, data, offsets, what, **kw):
    st, got, n = device_fired(r, data, offsets, **kw)
    assert st == 0 and n == want[0].size, f"{what}: status {st}, {n} fired, want {want[0].size}"
    ref.same(got, want, what)


# ---------------------------------------------------------------- the cases of the host file


@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_on_the_device_form_and_the_host_form(workdir, case):
    name, pats, rules, data, offsets = case
    nocase = ref.is_nocase(name)
    h = gpu_handle(pattern_file(workdir, "rules_" + name, pats), api.PFACX_READ_NOCASE if nocase else 0)
    try:
        r = h.rulesOpen(*ref.csr(rules))
        want = ref.fired_py(pats, rules, data, offsets, nocase)
        for off in (0, 5):                                                  # (5: a misaligned d_input)
            check_device(r, want, data, offsets, f"{name}/device/offset {off}", in_offset=off)
        ref.same(r.match_host_array(as_array(data), offsets), want, name + "/host form")      # the GPU platform: the pipelined batch path
        assert r.close() == 0
    finally:
        h.destroy()


def test_one_byte_fires_a_thousand_rules(workdir):
    h = gpu_handle(pattern_file(workdir, "rules_byte", [b"x", b"y"]))
    try:
        rules = [[1]] * 1000 + [[2]] + [[1, 2]]
        r = h.rulesOpen(*ref.csr(rules))
        want = ref.fired_py([b"x", b"y"], rules, b"x", [0, 1])
        check_device(r, want, b"x", [0, 1], "1000 rules from one byte")
        check_device(r, want, b"x", None, "1000 rules from one byte, no offsets", in_offset=3)
        st, got, n = device_fired(r, b"x", [0, 1], capacity=10)
        assert (st, n) == (TRUNCATED, 1000)
        ref.same(got, (want[0][:10], want[1][:10], want[2]), "truncated at 10")
        ref.same(r.match_host_array(as_array(b"x"), [0, 1]), want, "host form")
        r.close()
    finally:
        h.destroy()


# ---------------------------------------------------------------- every kernel variant and mode


@pytest.mark.parametrize("mode", MODES, ids=[m[2] for m in MODES])
@pytest.mark.parametrize("variant", VARIANTS, ids=[v[1] for v in VARIANTS])
def test_random_cases_in_every_variant_and_mode(workdir, variant, mode):
    for seed in (1, 2, 4, 7):
        pats, rules, data, offsets = ref.random_case(seed)
        h = make_handle(pattern_file(workdir, "rules_rnd%d" % seed, pats), mode[0], mode[1], variant[0])
        try:
            r = h.rulesOpen(*ref.csr(rules))
            check_device(r, ref.fired_py(pats, rules, data.tobytes(), offsets), data, offsets, f"seed {seed}/{variant[1]}/{mode[2]}")
            r.close()
        finally:
            h.destroy()


@pytest.mark.parametrize("seed", ref.RANDOM_SEEDS)
def test_random_cases(workdir, seed):
    pats, rules, data, offsets = ref.random_case(seed)
    h = gpu_handle(pattern_file(workdir, "rules_rnd%d" % seed, pats))
    try:
        r = h.rulesOpen(*ref.csr(rules))
        want = ref.fired_py(pats, rules, data.tobytes(), offsets)
        check_device(r, want, data, offsets, f"seed {seed}", in_offset=seed % 4)
        ref.same(r.match_host_array(data, offsets), want, f"seed {seed}/host form")
        r.close()
    finally:
        h.destroy()


# ---------------------------------------------------------------- the window, the touched list, the pairs of a trip, the grid

WINDOW_PATS = [b"p0;", b"p1;", b"p2;", b"p3;", b"p4;", b"p0;p1", b"zz"]


def window_rules(count):
    """rule r names 1 - 3 of the first six patterns by its number: every pattern has memberships in every window, so whatever a window is
    asked about, the same patterns' other memberships lie in its neighbours"""
    return [sorted({1 + r % 5, 1 + (r // 5) % 6, 1 + (r // 7) % 5}) for r in range(count)]


@pytest.mark.parametrize("count", [W - 1, W, W + 1, 2 * W + 1], ids=["W-1", "W", "W+1", "2W+1"])
def test_rule_counts_around_the_window(workdir, count):
    rules = window_rules(count)
    for r in (W - 1, W):                                                    # the last rule of window 0 and the first of window 1 fire together in segment 1
        if r < count:
            rules[r] = [2, 7]
    pieces = [b"p0;p1;p2;p3;p4;", b"zz p1;", b"p3;", b"", b"p0;p1 p4;", b"nothing", b"p2;p4;zz"]
    data, offsets = ref.cut(*pieces)
    want = ref.fired_py(WINDOW_PATS, rules, data, offsets)
    if count > W:
        seg1 = want[1][want[0] == 1]
        assert W - 1 in seg1 and W in seg1, "the case must cross the window edge inside one segment"
    h = gpu_handle(pattern_file(workdir, "rules_window", WINDOW_PATS))
    try:
        r = h.rulesOpen(*ref.csr(rules))
        check_device(r, want, data, offsets, f"{count} rules")
        n = want[0].size                                                    # a list several blocks long: truncated at 0, 1, n - 1 and n
        assert n > 4 * 256
        for cap in (0, 1, n - 1, n):
            st, got, total = device_fired(r, data, offsets, capacity=cap)
            assert (st, total) == (TRUNCATED if cap < n else 0, n)
            ref.same(got, (want[0][:cap], want[1][:cap], want[2]), f"{count} rules/capacity {cap}")
        st, got, total = device_fired(r, data, offsets, capacity=n, seg_first=False)
        assert (st, total) == (0, n)
        ref.same(got[:2], want[:2], f"{count} rules/no segFirst")
        r.close()
    finally:
        h.destroy()


@pytest.mark.parametrize("touch", [TOUCHED, TOUCHED + 1, 3 * TOUCHED], ids=["list-full", "one-more", "three-lists"])
def test_touched_list_and_what_it_leaves_behind(workdir, touch):
    """Segment 0 touches `touch` rules of window 0: half of them fire, half wait for a pattern that is not there.  The next segment the SAME block
    takes -- the grid has at most BLOCKS_PER_CU blocks per compute unit -- holds that other pattern alone: a mask left behind would fire them"""
    pats = [b"x", b"y", b"z"]
    half = touch // 2
    rules = [[1]] * half + [[1, 2]] * (touch - half) + [[3]] * 5 + [[2, 3]]
    h = gpu_handle(pattern_file(workdir, "rules_touched", pats))
    try:
        grid = int(h.info().multiProcessorCount) * BLOCKS_PER_CU
        pieces = [b"x"] + [b""] * (grid - 1) + [b"y", b"zy", b"x"]          # segment `grid` is block 0's second
        data, offsets = ref.cut(*pieces)
        want = ref.fired_py(pats, rules, data, offsets)
        assert want[2][1] == half and want[2][grid + 1] == half             # nothing fires on the lone y
        r = h.rulesOpen(*ref.csr(rules))
        check_device(r, want, data, offsets, f"{touch} rules touched")
        st, got, n = device_fired(r, data, offsets, capacity=half - 1)      # truncated inside the first segment: the state is cleaned all the same
        assert (st, n) == (TRUNCATED, want[0].size)
        ref.same(got, (want[0][:half - 1], want[1][:half - 1], want[2]), f"{touch} rules touched/truncated")
        r.close()
    finally:
        h.destroy()


def test_a_segment_of_more_pairs_than_a_block_takes_in_one_go(workdir):
    pats = [b"ab", b"abc", b"c", b"d", b"q"]
    rules = [[1], [2], [1, 3], [2, 4], [4], [5], [1, 2, 3, 4], [3, 5]]
    body = b"ab" * BLOCK_PAIRS + b"abc" + b"ab" * (2 * BLOCK_PAIRS) + b"d"           # the only abc behind the first trip, the only d in the last
    data, offsets = ref.cut(b"ab" * (BLOCK_PAIRS + 1), body, b"c" * (BLOCK_PAIRS - 1) + b"q", b"ab" * BLOCK_PAIRS + b"d")
    h = gpu_handle(pattern_file(workdir, "rules_trips", pats))
    try:
        r = h.rulesOpen(*ref.csr(rules))
        check_device(r, ref.fired_py(pats, rules, data, offsets), data, offsets, "more pairs than a trip")
        check_device(r, ref.fired_py(pats, rules, body, None), body, None, "more pairs than a trip, one segment")
        r.close()
    finally:
        h.destroy()


def test_more_segments_than_the_grid_has_blocks(workdir):
    rng = np.random.Generator(np.random.PCG64(99))
    letters = np.frombuffer(b"abcd ", dtype=np.uint8)
    pats = sorted({rng.choice(letters[:4], size=int(rng.integers(2, 6))).tobytes() for _ in range(40)})
    rules = [[int(i) for i in rng.integers(1, len(pats) + 1, size=int(rng.integers(1, 4)))] for _ in range(50)]
    h = gpu_handle(pattern_file(workdir, "rules_grid", pats))
    try:
        segs = 3 * int(h.info().multiProcessorCount) * BLOCKS_PER_CU + 17
        data = rng.choice(letters, size=64 * segs).astype(np.uint8)
        offsets = np.arange(segs + 1, dtype=np.uint64) * 64
        r = h.rulesOpen(*ref.csr(rules))
        check_device(r, ref.fired_np(pats, rules, data, offsets), data, offsets, f"{segs} segments of 64 bytes")
        r.close()
    finally:
        h.destroy()


def test_empty_and_one_byte_segments(workdir):
    pats = [b"a", b"b", b"ab"]
    rules = [[1], [2], [3], [1, 2]]
    rng = np.random.Generator(np.random.PCG64(5))
    lens = rng.integers(0, 2, size=3000)
    data = rng.choice(np.frombuffer(b"abc", dtype=np.uint8), size=int(lens.sum())).astype(np.uint8)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    h = gpu_handle(pattern_file(workdir, "rules_tiny", pats))
    try:
        r = h.rulesOpen(*ref.csr(rules))
        check_device(r, ref.fired_py(pats, rules, data.tobytes(), offsets), data, offsets, "empty and one-byte segments")
        ref.same(r.match_host_array(data, offsets), ref.fired_py(pats, rules, data.tobytes(), offsets), "host form")
        r.close()
    finally:
        h.destroy()


def test_an_input_above_the_32_mib_switch(workdir):
    """33 MiB of lowercase filler in 1.5 KiB segments; 300 patterns that start with a capital -- some a prefix of another --, 200 rules of 1 - 3
    of them, the patterns of a rule planted close together at 20 000 places (wherever they fall: across segment borders too)"""
    rng = np.random.Generator(np.random.PCG64(2026))
    n, seg_len = (33 << 20) + 1000, 1536
    alnum = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789", dtype=np.uint8)
    stems = sorted({bytes([65 + int(rng.integers(0, 26))]) + rng.choice(alnum, size=int(rng.integers(3, 9))).tobytes() for _ in range(200)})
    pats = stems + [s + rng.choice(alnum, size=int(rng.integers(1, 5))).tobytes() for s in stems[:100]]
    pats = sorted(set(pats))
    rules = [sorted({int(i) for i in rng.integers(1, len(pats) + 1, size=int(rng.integers(1, 4)))}) for _ in range(200)]
    data = rng.integers(97, 123, size=n, dtype=np.uint8)
    for at in rng.integers(0, n - 200, size=20000):
        at = int(at)
        for i in rules[int(rng.integers(0, len(rules)))]:
            p = np.frombuffer(pats[i - 1], dtype=np.uint8)
            data[at:at + p.size] = p
            at += p.size + int(rng.integers(0, 30))
    offsets = np.append(np.arange(0, n, seg_len, dtype=np.uint64), np.uint64(n))
    want = ref.fired_np(pats, rules, data, offsets)
    assert want[0].size > 10000
    h = gpu_handle(pattern_file(workdir, "rules_big", pats))
    try:
        r = h.rulesOpen(*ref.csr(rules))
        check_device(r, want, data, offsets, "33 MiB")
        r.close()
    finally:
        h.destroy()


# ---------------------------------------------------------------- hostile offsets, statuses, memory


def test_hostile_device_offsets_stay_inside_the_arrays(workdir):
    pats = [b"ab", b"b", b"abc"]
    rules = [[1], [2], [1, 2], [3]]
    data = as_array(b"abc ab b " * 300)
    n = data.size
    h = gpu_handle(pattern_file(workdir, "rules_hostile", pats))
    try:
        r = h.rulesOpen(*ref.csr(rules))
        for offsets in ([0, n, n // 2, 5, n], [n + 100, 2 ** 40, 0, n], [7, 3, 2 ** 63, 1, 0], [n, n, n, n]):
            st, _, total = device_fired(r, data, np.array(offsets, dtype=np.uint64))       # the list is whatever it is: the guards are checked
            assert st == 0 and total <= len(rules) * (len(offsets) - 1)
        r.close()
    finally:
        h.destroy()


def test_statuses_of_the_device_form(workdir):
    h = gpu_handle(pattern_file(workdir, "rules_args", [b"ab", b"b"]))
    try:
        r = h.rulesOpen(*ref.csr([[1], [1, 2]]))
        d_in = torch.from_numpy(as_array(b"abab").copy()).to("cuda:0")
        d_off = torch.tensor([0, 2, 4], dtype=torch.int64, device="cuda:0")
        d_seg, d_rule = (torch.zeros(8, dtype=torch.int32, device="cuda:0") for _ in range(2))
        d_first = torch.full((3,), 77, dtype=torch.int64, device="cuda:0")
        I, O, S, R, F = d_in.data_ptr(), d_off.data_ptr(), d_seg.data_ptr(), d_rule.data_ptr(), d_first.data_ptr()

        def status(*args):
            return r.match_device(*args, check=False)[0]

        assert r.match_device(I, 4, O, 2, S, R, 8, F) == (0, 4)
        assert status(None, 4, O, 2, S, R, 8, F) == INVALID
        assert status(I, 4, O, 2, None, R, 8, F) == INVALID
        assert status(I, 4, O, 2, S, None, 8, F) == INVALID
        assert status(I, 4, None, 2, S, R, 8, F) == INVALID
        assert status(I, 4, O, 0, S, R, 8, F) == INVALID
        assert status(I, 1 << 31, O, 2, S, R, 8, F) == INVALID
        assert status(I, 4, O, 1 << 31, S, R, 8, F) == INVALID
        assert r.match_device(I, 0, O, 2, S, R, 8, F) == (0, 0)             # size == 0: nothing fired, segFirst all zero
        torch.cuda.synchronize()
        assert d_first.cpu().tolist() == [0, 0, 0]
        h.readPatternFromFile(pattern_file(workdir, "rules_args2", [b"zz"]))
        assert status(I, 4, O, 2, S, R, 8, F) == INVALID                    # the rule set belongs to the set that has gone
        assert r.match_host(as_array(b"ab").copy().ctypes.data, 2, None, 1, None, None, 0, None, check=False)[0] == INVALID
        assert r.close() == 0
    finally:
        h.destroy()


def round256(b):
    return (b + 255) & ~255


def test_memory_accounting(workdir):
    pats = [b"ab", b"b", b"abc", b"ab"]
    rules = [[1, 2], [3], [4, 2, 2], [2]]                                   # I = 6 ids after resolution: {2, 4}, {3}, {2, 4}, {2}
    data = as_array(b"abc ab b " * 100)
    n = data.size
    h = gpu_handle(pattern_file(workdir, "rules_mem", pats))
    try:
        h.trim()
        tables0, scratch0 = int(h.info().deviceTableBytes), int(h.info().deviceScratchBytes)
        r = h.rulesOpen(*ref.csr(rules))
        assert int(h.info().deviceTableBytes) == tables0                    # nothing on the device before the first device call
        n1, n2 = 3, 700
        for segs, last in ((n1, None), (n2, n1)):
            offsets = np.minimum(np.arange(segs + 1, dtype=np.uint64) * 4, n)
            offsets[-1] = n
            check_device(r, ref.fired_py(pats, rules, data.tobytes(), offsets), data, offsets, f"{segs} segments")
            scratch = int(h.info().deviceScratchBytes)
            if last is not None:                                            # the same bytes and pairs, more segments: what depends on the segments alone
                assert scratch - before == 4 * (segs - last) + round256(8 * (segs + 1)) - round256(8 * (last + 1))
            before = scratch
        want_tables = 4 * (len(pats) + 2) + 4 * 6 + 4 * len(rules)
        assert int(h.info().deviceTableBytes) == tables0 + want_tables
        h.trim()                                                            # the scratch goes, the rule tables stay
        assert int(h.info().deviceScratchBytes) == scratch0 and int(h.info().deviceTableBytes) == tables0 + want_tables
        check_device(r, ref.fired_py(pats, rules, data.tobytes(), None), data, None, "after trim")
        r.close()
        assert int(h.info().deviceTableBytes) == tables0
    finally:
        h.destroy()


def test_example_program_passes_its_self_check(workdir):
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "rules_example"], check=True, stdout=subprocess.PIPE)
    p = subprocess.run([os.path.join(ROOT, "examples", "rules_example")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    assert b"self-check passed" in p.stdout and b"(device form)" in p.stdout
