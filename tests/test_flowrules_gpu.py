"""Flow-rule sets (PFACX_flowRules*) on the GPU: PFACX_flowsMatchFromDevice and PFACX_flowsFlush feed PFACX_flowRulesPairsFromDevice
(scan_flowrules.hip) on the device, call by call against tests/flowrules_ref.py.  Poisoned arrays with guard words, the pair arrays compared
unchanged, the kernel's edges at their smallest shapes, hostile device arrays, truncation by the repeat, the memory formulas, the example."""

import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import flowrules_ref as fx  # noqa: E402
from tests.test_flowrules_host import EXAMPLE_OUTPUT, PATS, RULES  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 16
INVALID, TRUNCATED = api.STATUS.INVALID_PARAMETER, api.STATUS.OUTPUT_TRUNCATED
W, TOUCHED, BLOCK = api.PFACX_FLOWRULES_WINDOW, api.PFACX_FLOWRULES_TOUCHED, api.PFACX_FLOWRULES_BLOCK_PAIRS


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def device_call(fl, d_ids, num_pairs, d_first, flows, capacity=None, check_status=True):
    """one pairs_device call over device arrays the caller holds: poisoned outputs of EXACTLY `capacity` entries (None: the count query first)
    between guard words, pieceFiredFirst likewise; the pair arrays must stay as they were -> (status, piece[], rule[], firedFirst, full length)"""
    flows = np.ascontiguousarray(flows, np.uint32)
    keep_ids, keep_first, keep_flows = d_ids.clone(), d_first.clone(), flows.copy()
    if capacity is None:
        st, capacity = fl.pairs_device(d_ids.data_ptr(), num_pairs, d_first.data_ptr(), flows.ctypes.data, flows.size, None, None, 0, None)
        assert st == (TRUNCATED if capacity else 0)
    d_piece = torch.full((capacity + 2 * PAD,), -7, dtype=torch.int32, device="cuda:0")
    d_rule = torch.full((capacity + 2 * PAD,), -7, dtype=torch.int32, device="cuda:0")
    d_ff = torch.full((flows.size + 1 + 2 * PAD,), -7, dtype=torch.int64, device="cuda:0")
    st, n = fl.pairs_device(d_ids.data_ptr(), num_pairs, d_first.data_ptr(), flows.ctypes.data, flows.size, d_piece.data_ptr() + 4 * PAD,
                            d_rule.data_ptr() + 4 * PAD, capacity, d_ff.data_ptr() + 8 * PAD, check=check_status)
    torch.cuda.synchronize()
    k = min(n, capacity)
    for arr, used in ((d_piece, k), (d_rule, k), (d_ff, flows.size + 1 if st in (0, TRUNCATED) else 0)):
        assert bool((arr[:PAD] == -7).all()) and bool((arr[PAD + used:] == -7).all()), "wrote outside the list"
    assert bool((d_ids == keep_ids).all()) and bool((d_first == keep_first).all()) and np.array_equal(flows, keep_flows), "the pair arrays were modified"
    return st, d_piece[PAD:PAD + k].cpu().numpy(), d_rule[PAD:PAD + k].cpu().numpy(), d_ff[PAD:PAD + flows.size + 1].cpu().numpy(), n


def host_pairs(fl, ids, first, flows, **kw):
    """device_call over host-made pairs, uploaded between poison"""
    ids, first = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(first, np.int32)
    d_ids = dev(ids if ids.size else np.zeros(1, np.int32), np.int32)
    return device_call(fl, d_ids, ids.size, dev(first, np.int32), flows, **kw)


def same(got, want, what):
    st, piece, rule, first, n = got
    assert st == 0 and n == want[0].size, f"{what}: status {st}, {n} fired, want {want[0].size}"
    assert np.array_equal(piece, want[0]), f"{what}: pieces differ"
    assert np.array_equal(rule, want[1]), f"{what}: rules differ"
    assert np.array_equal(first.astype(np.uint64), want[2]), f"{what}: pieceFiredFirst differs"


def open_set(pats, rules, num_flows):
    h = api.PFAC.create()
    h.readPatternFromMemory(b"".join(p + b"\n" for p in pats))
    off, flat = fx.rr.csr(rules)
    return h, h.flowRulesOpen(off, flat, num_flows), fx.Sets(pats, rules, num_flows)


@pytest.mark.parametrize("nocase", [False, True], ids=["plain", "nocase"])
def test_flows_call_feeds_the_rules_call_on_the_device(workdir, nocase):
    """the 70-flow schedule: the ids and pieceFirst that PFACX_flowsMatchFromDevice / PFACX_flowsFlush leave on the device go straight into
    PFACX_flowRulesPairsFromDevice"""
    pf, raw, pats, rules, m, fm = fx.workload(workdir, nocase=nocase)
    h = api.PFAC.create()
    h.readPatternFromMemoryEx(raw, api.PFACX_READ_NOCASE if nocase else 0)
    off, flat = fx.rr.csr(rules)
    flows, fl = h.flowsOpen(m.F), h.flowRulesOpen(off, flat, m.F)
    M = int(h.info().maxPatternLen)

    def call(s):
        pieces = s.src.flows.size
        if s.flush:
            cap = max(1, pieces * (M - 1))
        else:
            cap = int(s.src.buf.size) + pieces * (M - 1)
        d_ids = torch.full((max(1, cap),), -7, dtype=torch.int32, device="cuda:0")
        d_pos = torch.full((max(1, cap),), -7, dtype=torch.int32, device="cuda:0")
        d_first = torch.full((pieces + 1,), -7, dtype=torch.int32, device="cuda:0")
        fl_ids = s.src.flows.copy()
        if s.flush:
            _, k = flows.flush(fl_ids.ctypes.data, pieces, d_ids.data_ptr(), d_pos.data_ptr(), cap, d_first.data_ptr())
        else:
            d_in = dev(s.src.buf if s.src.buf.size else np.zeros(1, np.uint8), np.uint8)
            offs, offsets = np.zeros(pieces, np.uint64), s.src.offsets.copy()
            _, k = flows.match_device(d_in.data_ptr(), int(s.src.buf.size), offsets.ctypes.data, fl_ids.ctypes.data, pieces, d_ids.data_ptr(),
                                      d_pos.data_ptr(), max(1, cap), d_first.data_ptr(), offs.ctypes.data)
        assert k == s.src.ids.size
        return device_call(fl, d_ids, k, d_first, s.src.flows)[1:]

    def reset(f):
        fl.reset(f)
        if not any(isinstance(s, fx.Call) and s.flush and s.src.flows is f for s in fm.steps):
            flows.reset(f)                                 # (a flush has forgotten its flows already)

    try:
        fx.run(fm, call, reset, "flows -> rules on the device")
    finally:
        fl.close()
        flows.close()
        h.destroy()


def many_rules(count, num_pats=64):
    """rule r names up to three of num_pats patterns, a function of r"""
    return [sorted({1 + r % num_pats, 1 + (r // num_pats) % num_pats, 1 + (r // (num_pats * num_pats) + r) % num_pats}) for r in range(count)]


@pytest.mark.parametrize("count", [W - 1, W, W + 1])
def test_rule_counts_around_the_window(count):
    """W - 1, W, W + 1 rules: the last slot of a window, a full window, a second window of one rule"""
    pats = [b"p%02d;" % i for i in range(64)]
    rules = many_rules(count)
    rules[-1] = [64]                                        # the last rule fires alone
    h, fl, model = open_set(pats, rules, 4)
    rng = np.random.Generator(np.random.PCG64(count))
    try:
        for step in range(4):
            flows = rng.permutation(4)[:3]
            counts = np.array([0, 5, 9]) if step == 0 else rng.integers(0, 12, size=3)      # (an empty piece)
            first = np.concatenate([[0], np.cumsum(counts)])
            ids = rng.integers(1, 65, size=int(first[-1]))
            same(host_pairs(fl, ids, first, flows), model.call(ids, first, flows), f"{count} rules, step {step}")
        everything = np.arange(1, 65)
        same(host_pairs(fl, everything, [0, 64], [3]), model.call(everything, [0, 64], [3]), f"{count} rules: the rest of flow 3")
    finally:
        fl.close()
        h.destroy()


def test_touched_list_exactly_full_and_one_more():
    """a piece that touches exactly the 1024 entries of the touched list, and one that touches more (the sweep of the whole table)"""
    pats = [b"xx", b"yy", b"zz"]
    rules = [[1] if r % 2 == 0 else [1, 3] for r in range(TOUCHED)] + [[2], [2, 3]]
    h, fl, model = open_set(pats, rules, 2)
    try:
        same(host_pairs(fl, [1, 2, 1], [0, 1, 3], [0, 1]), model.call([1, 2, 1], [0, 1, 3], [0, 1]), "1024 touched | 1026 touched")
        same(host_pairs(fl, [3, 3], [0, 1, 2], [1, 0]), model.call([3, 3], [0, 1, 2], [1, 0]), "the second members")
    finally:
        fl.close()
        h.destroy()


def test_pieces_of_257_and_513_pairs_and_more_pieces_than_blocks():
    """more than one trip of a block over a piece's pairs; more pieces than four blocks per compute unit"""
    pats = [b"p%02d;" % i for i in range(64)]
    rules = many_rules(300)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pieces = 4 * cus + 77
    h, fl, model = open_set(pats, rules, pieces)
    rng = np.random.Generator(np.random.PCG64(257))
    try:
        counts = rng.integers(0, 3, size=pieces)
        counts[5], counts[pieces - 2] = BLOCK + 1, 2 * BLOCK + 1
        first = np.concatenate([[0], np.cumsum(counts)])
        for step in range(2):
            ids = rng.integers(1, 65, size=int(first[-1]))
            ids[first[5]:first[5] + BLOCK] = 7                                           # what completes a rule sits in the second trip
            flows = rng.permutation(pieces)
            same(host_pairs(fl, ids, first, flows), model.call(ids, first, flows), f"{pieces} pieces, step {step}")
    finally:
        fl.close()
        h.destroy()


@pytest.mark.parametrize("D", [31, 32, 33])
def test_bitmap_word_edges(D):
    pats = [b"p%02d;" % i for i in range(40)]
    rules = [[i + 1, (i + 1) % D + 1] for i in range(D)] + [list(range(1, min(D, 32) + 1)), [D], [D, 1]]
    h, fl, model = open_set(pats, rules, 3)
    rng = np.random.Generator(np.random.PCG64(D))
    try:
        for _ in range(6):
            flows = rng.permutation(3)[:int(rng.integers(1, 4))]
            first = np.concatenate([[0], np.cumsum(rng.integers(0, 9, size=flows.size))])
            ids = rng.integers(1, 41, size=int(first[-1]))
            same(host_pairs(fl, ids, first, flows), model.call(ids, first, flows), f"D = {D}")
        everything = np.arange(1, 41)
        for f in range(3):
            same(host_pairs(fl, everything, [0, 40], [f]), model.call(everything, [0, 40], [f]), f"D = {D}: the rest of flow {f}")
    finally:
        fl.close()
        h.destroy()


def test_hostile_device_arrays_touch_nothing_outside():
    """ids 0, -1 and F + 1 are skipped; a decreasing pieceFirst is an empty piece, one beyond numPairs is clamped: wrong lists at worst, the guard
    words stay (device_call checks them)"""
    h, fl, model = open_set(PATS, RULES, 4)
    try:
        ids = [0, -1, len(PATS) + 1, 1, 2, 1 << 30, -(1 << 31), 4]
        same(host_pairs(fl, ids, [0, 6, 8], [2, 0]), model.call(ids, [0, 6, 8], [2, 0]), "ids outside [1, F]")
        model.reset()
        fl.reset()
        # first pairs: decreasing (piece 0 is empty), beyond numPairs, negative: every piece is what the clamps make of it
        st, piece, rule, first, n = host_pairs(fl, [1, 2, 4, 3, 5], [4, 2, 1 << 30, -5, 3], [0, 1, 2, 3])
        # piece 0 = [4, 2): empty; piece 1 = [2, 2^30) -> [2, 5): GET /admin, GET, passwd; piece 2 = [5, -5) -> [5, 0): empty; piece 3 = [0, 3)
        assert (st, n, piece.tolist(), rule.tolist()) == (0, 4, [1, 1, 3, 3], [1, 2, 0, 2])
        assert first.tolist() == [0, 0, 2, 2, 4]
    finally:
        fl.close()
        h.destroy()


def test_truncation_leaves_the_device_state_unchanged():
    h, fl, model = open_set(PATS, RULES, 2)
    try:
        ids, first, flows = [1, 2, 4, 5, 1], [0, 4, 5], [1, 0]
        want = model.call(ids, first, flows)
        assert want[0].size == 4
        for capacity in (3, 0, 1):
            st, piece, rule, fired_first, n = host_pairs(fl, ids, first, flows, capacity=capacity)
            assert st == TRUNCATED and n == 4
            assert np.array_equal(piece, want[0][:capacity]) and np.array_equal(rule, want[1][:capacity])
            assert np.array_equal(fired_first.astype(np.uint64), want[2]), "pieceFiredFirst is complete"
        same(host_pairs(fl, ids, first, flows, capacity=4), want, "the repeat with room returns the whole list")
        st, piece, rule, fired_first, n = host_pairs(fl, ids, first, flows)
        assert (st, n) == (0, 0) and not fired_first.any(), "the same pairs twice: an empty second list"
    finally:
        fl.close()
        h.destroy()


def test_mixed_kinds_of_call_and_refusals():
    h, fl, model = open_set(PATS, RULES, 3)
    try:
        same(host_pairs(fl, [1], [0, 1], [0]), model.call([1], [0, 1], [0]), "device-fed")
        assert fl.pairs_host_array([2], [0, 1], [0], capacity=4, check=False)[0] == INVALID          # a device-fed set
        assert host_pairs(fl, [2], [0, 1, 1], [1, 1], capacity=4, check_status=False)[0] == INVALID  # a flow twice
        assert host_pairs(fl, [2], [0, 1], [3], capacity=4, check_status=False)[0] == INVALID        # an id >= numFlows
        same(host_pairs(fl, [2], [0, 1], [0]), model.call([2], [0, 1], [0]), "the refused calls changed nothing")
        fl.reset()
        model.reset()
        st, piece, rule, first, n = fl.pairs_host_array([1, 2], [0, 2], [0])
        assert (st, n, rule.tolist()) == (0, 1, [0])
        assert host_pairs(fl, [2], [0, 1], [0], capacity=4, check_status=False)[0] == INVALID        # a host-fed set
        fl.reset()
        same(host_pairs(fl, [1, 2], [0, 2], [0]), model.call([1, 2], [0, 2], [0]), "after the reset of all flows: device-fed again")
        h.readPatternFromMemory(b"other\nset\n")
        assert host_pairs(fl, [1], [0, 1], [1], capacity=4, check_status=False)[0] == INVALID        # another pattern set
        assert fl.reset(check=False) == INVALID
    finally:
        assert fl.close() == 0
        h.destroy()


def test_memory_formulas():
    """state under deviceTableBytes -- made by the first device call, kept by PFACX_trim, freed by close -- and scratch under
    deviceScratchBytes, given back by PFACX_trim: the formulas of include/pfac_ext.h"""
    pats = [b"p%02d;" % i for i in range(40)]
    rules = [[i + 1, (i + 1) % 33 + 1] for i in range(33)] + [[1, 2, 3], [40]]
    F, R, I, D, flows = 40, len(rules), sum(len(r) for r in rules), 34, 1000
    state = 4 * (F + 2) + 8 * I + 4 * (R + 1) + 4 * (F + 1) + flows * 4 * ((D + 31) // 32)
    up256 = lambda b: (b + 255) // 256 * 256             # noqa: E731
    h, fl, model = open_set(pats, rules, flows)
    try:
        h.trim()
        tables, scratch = h.info().deviceTableBytes, h.info().deviceScratchBytes
        pieces = 300
        first = np.arange(pieces + 1)
        ids = np.arange(pieces) % 40 + 1
        same(host_pairs(fl, ids, first, np.arange(pieces)), model.call(ids, first, np.arange(pieces)), "the first device call")
        assert h.info().deviceTableBytes == tables + state
        assert h.info().deviceScratchBytes == scratch + up256(4 * pieces) + up256(8 * (pieces + 1)) + 8 * (F + 1)
        h.trim()
        assert h.info().deviceScratchBytes == scratch and h.info().deviceTableBytes == tables + state
        ids2 = (np.arange(pieces) + 1) % 40 + 1
        same(host_pairs(fl, ids2, first, np.arange(pieces)), model.call(ids2, first, np.arange(pieces)), "the state survived PFACX_trim")
        fl.close()
        assert h.info().deviceTableBytes == tables
    finally:
        h.destroy()


def test_example_program_feeds_device_arrays():
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "flowrules_example"], check=True, stdout=subprocess.PIPE)
    p = subprocess.run([os.path.join(ROOT, "examples", "flowrules_example")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout.decode().splitlines() == EXAMPLE_OUTPUT
