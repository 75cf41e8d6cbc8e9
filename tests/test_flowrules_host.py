"""Flow-rule sets (PFACX_flowRules*) through the host form, on host-only handles: no device needed.

The schedules of tests/flowrules_ref.py -- 70 flows, flushes and resets midway, a caseless set -- run call by call through
PFACX_flowRulesPairsFromHost against the model; every refused call is followed by the same call done right (the state was untouched); truncation
leaves every flow as it was; guard words stand behind `capacity` and behind pieceFiredFirst; D = 31, 32 and 33 distinct rule patterns; duplicate
pattern lines; the example program on its host path."""

import os
import subprocess

import numpy as np
import pytest

from pfac_amd import api
from tests import flowrules_ref as fx
from tests.test_stream_host import host_handle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 8
INVALID, TRUNCATED = api.STATUS.INVALID_PARAMETER, api.STATUS.OUTPUT_TRUNCATED


def host_call(fl, ids, first, flows, capacity=None, want_first=True):
    """one pairs_host call over arrays of EXACTLY `capacity` entries (None: the count query first) with guard words behind them and behind
    pieceFiredFirst -> (status, piece[], rule[], pieceFiredFirst, full length); the input arrays must stay as they were"""
    ids, first, flows = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(first, np.int32), np.ascontiguousarray(flows, np.uint32)
    keep = ids.copy(), first.copy(), flows.copy()
    idb = ids if ids.size else np.zeros(1, np.int32)
    if capacity is None:
        st, capacity = fl.pairs_host(idb.ctypes.data, ids.size, first.ctypes.data, flows.ctypes.data, flows.size, None, None, 0, None)
        assert st == (TRUNCATED if capacity else 0)
    piece = np.full(capacity + PAD, -7, np.int32)
    rule = np.full(capacity + PAD, -7, np.int32)
    fired_first = np.full(flows.size + 1 + PAD, 0xABCD, np.uintp)
    st, n = fl.pairs_host(idb.ctypes.data, ids.size, first.ctypes.data, flows.ctypes.data, flows.size, piece.ctypes.data, rule.ctypes.data, capacity,
                          fired_first.ctypes.data if want_first else None, check=False)
    assert (piece[capacity:] == -7).all() and (rule[capacity:] == -7).all(), "wrote behind capacity"
    assert (fired_first[flows.size + 1:] == 0xABCD).all(), "wrote behind pieceFiredFirst"
    assert np.array_equal(ids, keep[0]) and np.array_equal(first, keep[1]) and np.array_equal(flows, keep[2]), "the input arrays were modified"
    k = min(n, capacity)
    assert (piece[k:] == -7).all() and (rule[k:] == -7).all(), "wrote behind the list"
    return st, piece[:k].copy(), rule[:k].copy(), fired_first[:flows.size + 1].copy(), n


def feed(h, fm, rules, what):
    off, flat = fx.rr.csr(rules)
    fl = h.flowRulesOpen(off, flat, fm.flows.F)

    def call(s):
        st, piece, rule, first, n = host_call(fl, s.src.ids, s.src.first, s.src.flows)
        assert st == 0
        return piece, rule, first, n

    try:
        fx.run(fm, call, lambda flows: fl.reset(flows), what)
    finally:
        fl.close()


@pytest.fixture(scope="module")
def plain(workdir):
    return fx.workload(workdir)


@pytest.mark.parametrize("platform,pname", [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "omp")])
def test_schedule_of_70_flows_against_the_model(plain, platform, pname):
    pf, raw, pats, rules, m, fm = plain
    assert "PFACX_flowRulesPairsFromHost" in api.EXPORTED_SYMBOLS and fm.cov.fired > 1000
    h = host_handle(pf, platform=platform)
    try:
        feed(h, fm, rules, f"plain/{pname}")
    finally:
        h.destroy()


def test_caseless_set(workdir):
    pf, raw, pats, rules, m, fm = fx.workload(workdir, nocase=True)
    assert raw != open(pf, "rb").read()                    # the handle folds the set itself
    h = host_handle(raw=raw, flags=api.PFACX_READ_NOCASE)
    try:
        feed(h, fm, rules, "nocase")
    finally:
        h.destroy()


def test_the_flows_call_feeds_the_rules_call_on_the_host(plain):
    """the pairs come from PFACX_flowsMatchFromHost and PFACX_flowsFlush themselves, not from the model"""
    pf, raw, pats, rules, m, fm = plain
    h = host_handle(pf)
    off, flat = fx.rr.csr(rules)
    flows, fl = h.flowsOpen(m.F), h.flowRulesOpen(off, flat, m.F)

    def call(s):
        if s.flush:
            _, ids, pos, first = flows.flush_host_array(s.src.flows)
        else:
            _, ids, pos, first, _ = flows.match_host_array(s.src.buf, s.src.offsets, s.src.flows)
        return host_call(fl, ids, first, s.src.flows)[1:]

    def reset(f):
        fl.reset(f)
        if not any(isinstance(s, fx.Call) and s.flush and s.src.flows is f for s in fm.steps):
            flows.reset(f)                                 # (a flush has forgotten its flows already)

    try:
        fx.run(fm, call, reset, "flows -> rules on the host")
    finally:
        fl.close()
        flows.close()
        h.destroy()


def small(pats, rules, num_flows):
    h = host_handle(raw=b"".join(p + b"\n" for p in pats))
    off, flat = fx.rr.csr(rules)
    return h, h.flowRulesOpen(off, flat, num_flows), fx.Sets(pats, rules, num_flows)


PATS = [b"User-Agent:", b"sqlmap", b"GET", b"GET /admin", b"passwd"]
RULES = [[1, 2], [3, 5], [4], [1, 2, 3, 5]]


def same(got, want, what):
    st, piece, rule, first, n = got
    assert st == 0 and n == want[0].size, f"{what}: status {st}, {n} fired, want {want[0].size}"
    assert np.array_equal(piece, want[0]) and np.array_equal(rule, want[1]) and np.array_equal(first.astype(np.uint64), want[2]), what


def test_members_from_different_calls_and_the_same_pairs_twice():
    h, fl, model = small(PATS, RULES, 3)
    try:
        calls = [([1, 4], [0, 1, 2], [2, 0]), ([2], [0, 1], [2]), ([5, 2], [0, 0, 2], [1, 0]), ([1, 5, 2, 4], [0, 4], [1])]
        for ids, first, flows in calls:
            same(host_call(fl, ids, first, flows), model.call(ids, first, flows), f"call {ids}")
            st, piece, rule, fired_first, n = host_call(fl, ids, first, flows)          # fed again: nothing new, nothing fires
            assert st == 0 and n == 0 and piece.size == 0 and not fired_first.any()
        fl.reset([0])
        model.reset([0])
        same(host_call(fl, [4, 5], [0, 2], [0]), model.call([4, 5], [0, 2], [0]), "after the reset of flow 0: its rules fire again")
        assert host_call(fl, [4, 5, 2, 1], [0, 4], [1])[4] == 0                          # flow 1 was not reset
        fl.reset()
        model.reset()
        same(host_call(fl, [4, 5, 2, 1], [0, 4], [1]), model.call([4, 5, 2, 1], [0, 4], [1]), "after the reset of all flows")
    finally:
        fl.close()
        h.destroy()


def test_truncation_changes_no_flow():
    h, fl, model = small(PATS, RULES, 2)
    try:
        ids, first, flows = [1, 2, 4, 5, 1], [0, 4, 5], [1, 0]
        want = model.call(ids, first, flows)
        assert want[0].size == 4
        for capacity in (want[0].size - 1, 0, 1):
            st, piece, rule, fired_first, n = host_call(fl, ids, first, flows, capacity=capacity)
            assert st == TRUNCATED and n == want[0].size
            assert np.array_equal(piece, want[0][:capacity]) and np.array_equal(rule, want[1][:capacity])
            assert np.array_equal(fired_first.astype(np.uint64), want[2]), "pieceFiredFirst is complete"
        st, n = fl.pairs_host(np.array(ids, np.int32).ctypes.data, 5, np.array(first, np.int32).ctypes.data, np.array(flows, np.uint32).ctypes.data, 2,
                              None, None, 0, None)
        assert (st, n) == (TRUNCATED, 4)                                                 # the count query
        same(host_call(fl, ids, first, flows, capacity=4), want, "the repeat with room returns the whole list")
        assert host_call(fl, ids, first, flows, capacity=0)[4] == 0                      # ... and now the flows have moved on
    finally:
        fl.close()
        h.destroy()


def test_every_capacity_with_empty_pieces_and_without_piece_fired_first():
    """the list frame at its edges: an empty first, middle and last piece; every capacity below the length of the list -- inside a piece, exactly at a
    piece's border (pieceFiredFirst = 0, 0, 4, 4, 5, 5), the length - 1 -- truncates and commits nothing, with pieceFiredFirst and with a null one;
    the length itself and the length + 1 return the whole list"""
    ids, first, flows = [1, 2, 4, 5, 3, 5], [0, 0, 4, 4, 6, 6], [4, 1, 3, 0, 2]
    want = fx.Sets(PATS, RULES, 5).call(ids, first, flows)
    assert want[2].tolist() == [0, 0, 4, 4, 5, 5]
    total = int(want[0].size)
    for room in (total, total + 1):
        h, fl, _ = small(PATS, RULES, 5)
        try:
            for capacity in range(total):
                for want_first in (True, False):
                    st, piece, rule, fired_first, n = host_call(fl, ids, first, flows, capacity=capacity, want_first=want_first)
                    assert (st, n) == (TRUNCATED, total), f"capacity {capacity}"
                    assert np.array_equal(piece, want[0][:capacity]) and np.array_equal(rule, want[1][:capacity]), f"capacity {capacity}"
                    assert np.array_equal(fired_first.astype(np.uint64), want[2]) if want_first else (fired_first == 0xABCD).all(), f"capacity {capacity}"
            same(host_call(fl, ids, first, flows, capacity=room), want, f"capacity {room}: every truncated call left the flows as they were")
            assert host_call(fl, ids, first, flows, capacity=0)[4] == 0                  # ... and now they have moved on
        finally:
            fl.close()
            h.destroy()


@pytest.mark.parametrize("D", [31, 32, 33])
def test_bitmap_word_edges(D):
    """D distinct rule patterns: the last bit of a word, a full word, the first bit of the next"""
    pats = [b"p%02d;" % i for i in range(40)]
    rules = [[i + 1, (i + 1) % D + 1] for i in range(D)] + [list(range(1, min(D, 32) + 1)), [D], [D, 1]]
    h, fl, model = small(pats, rules, 3)
    rng = np.random.Generator(np.random.PCG64(D))
    try:
        for _ in range(12):
            flows = rng.permutation(3)[:int(rng.integers(1, 4))]
            counts = rng.integers(0, 9, size=flows.size)
            first = np.concatenate([[0], np.cumsum(counts)])
            ids = rng.integers(1, 41, size=int(first[-1]))
            same(host_call(fl, ids, first, flows), model.call(ids, first, flows), f"D = {D}")
        everything = np.arange(1, 41)
        for f in range(3):
            same(host_call(fl, everything, [0, 40], [f]), model.call(everything, [0, 40], [f]), f"D = {D}: the rest of flow {f}")
    finally:
        fl.close()
        h.destroy()


def test_duplicate_lines_and_ids_outside_the_set():
    pats = [b"dup", b"other", b"dup"]              # id 3 is the one reported
    rules = [[1, 2], [3], [1, 3, 2, 2]]
    h, fl, model = small(pats, rules, 1)
    try:
        ids = [0, -1, 4, 3, 1 << 30]
        same(host_call(fl, ids, [0, 5], [0]), model.call(ids, [0, 5], [0]), "ids outside [1, F] are skipped")
        same(host_call(fl, [2], [0, 1], [0]), model.call([2], [0, 1], [0]), "the lower id named, the reported id fed")
    finally:
        fl.close()
        h.destroy()


def test_refusals_leave_the_state_untouched():
    h, fl, model = small(PATS, RULES, 3)
    i32, u32 = lambda a: np.array(a, np.int32), lambda a: np.array(a, np.uint32)         # noqa: E731
    ids, first, flows = i32([1, 2, 4]), i32([0, 2, 3]), u32([0, 2])
    out_p, out_r = np.zeros(8, np.int32), np.zeros(8, np.int32)

    def raw(ids=ids, num_pairs=3, first=first, flows=flows, pieces=2, piece=out_p, rule=out_r, capacity=8, form="host"):
        f = fl.pairs_host if form == "host" else fl.pairs_device
        return f(ids.ctypes.data if ids is not None else None, num_pairs, first.ctypes.data if first is not None else None,
                 flows.ctypes.data if flows is not None else None, pieces, piece.ctypes.data if piece is not None else None,
                 rule.ctypes.data if rule is not None else None, capacity, None, check=False)

    try:
        assert raw(flows=u32([1, 1]))[0] == INVALID                                     # a flow twice
        assert raw(flows=u32([0, 3]))[0] == INVALID                                     # an id >= numFlows
        assert raw(first=i32([1, 2, 3]))[0] == INVALID                                  # pieceFirst does not start at 0
        assert raw(first=i32([0, 2, 2]))[0] == INVALID                                  # ... does not end at numPairs
        assert raw(first=i32([0, 4, 3]))[0] == INVALID                                  # ... decreases
        assert raw(ids=None)[0] == INVALID and raw(first=None)[0] == INVALID and raw(flows=None)[0] == INVALID
        assert raw(piece=None)[0] == INVALID and raw(rule=None)[0] == INVALID           # null with capacity > 0
        assert raw(num_pairs=1 << 31)[0] == INVALID and raw(pieces=1 << 31)[0] == INVALID
        assert raw(pieces=0)[0] == INVALID                                              # pairs without a piece
        assert raw(num_pairs=0, pieces=0, ids=None, first=None, flows=None) == (0, 0)   # nothing in, nothing out
        assert raw(form="device")[0] == api.STATUS.LIB_NOT_EXIST                        # a host-only handle
        lib = api.load_library()
        assert lib.PFACX_flowRulesPairsFromHost(fl._f, ids.ctypes.data, 3, first.ctypes.data, flows.ctypes.data, 2, None, None, 0, None, None) == INVALID
        assert lib.PFACX_flowRulesPairsFromHost(None, ids.ctypes.data, 3, first.ctypes.data, flows.ctypes.data, 2, None, None, 0, None, None) == \
            api.STATUS.INVALID_HANDLE
        assert fl.reset([3], check=False) == INVALID
        # after all that, the call done right finds every flow empty
        same(host_call(fl, ids, first, flows), model.call(ids, first, flows), "the call done right")
    finally:
        fl.close()
    off, flat = fx.rr.csr(RULES)
    try:
        for bad_rules in ([[]], [[6]], [[0]], [[1], []]):               # no member, an id outside [1, F]
            o, f = fx.rr.csr(bad_rules)
            assert h.flowRulesOpen(o, f, 3, check=False).status == INVALID
        assert h.flowRulesOpen(off, flat, 0, check=False).status == INVALID             # numFlows == 0
        assert h.flowRulesOpen(off, flat, 1 << 31, check=False).status == INVALID
        assert h.flowRulesOpen([0], [1], 3, check=False).status == INVALID              # no rule
    finally:
        h.destroy()


def test_zero_and_thirty_three_members():
    pats = [b"q%02d;" % i for i in range(34)]
    h = host_handle(raw=b"".join(p + b"\n" for p in pats))
    try:
        for rules, ok in (([[]], False), ([list(range(1, 34))], False), ([list(range(1, 33))], True), ([list(range(1, 33)) + [5, 6]], True)):
            off, flat = fx.rr.csr(rules)
            fl = h.flowRulesOpen(off, flat, 2, check=False)
            assert (fl.status == 0) == ok, rules
            if ok:
                everything = np.arange(1, 35)
                assert host_call(fl, everything[:31], [0, 31], [1])[4] == 0
                st, piece, rule, first, n = host_call(fl, everything[31:], [0, 3], [1])
                assert (st, n, piece.tolist(), rule.tolist()) == (0, 1, [0], [0])
                fl.close()
    finally:
        h.destroy()


def test_another_pattern_set_leaves_only_close(plain):
    h, fl, model = small(PATS, RULES, 2)
    try:
        same(host_call(fl, [1], [0, 1], [0]), model.call([1], [0, 1], [0]), "before")
        h.readPatternFromMemory(b"other\nset\n")
        assert host_call(fl, [2], [0, 1], [0], capacity=4)[0] == INVALID
        assert fl.reset(check=False) == INVALID and fl.reset([0], check=False) == INVALID
        assert fl.close() == 0
        empty = api.PFAC.createHostOnly()
        try:
            assert empty.flowRulesOpen([0, 1], [1], 2, check=False).status == api.STATUS.PATTERNS_NOT_READY
        finally:
            empty.destroy()
    finally:
        h.destroy()


def test_destroy_closes_open_sets_and_the_array_helper():
    h, fl, model = small(PATS, RULES, 2)
    st, piece, rule, first, n = fl.pairs_host_array([1, 2, 4], [0, 2, 3], [1, 0])
    want = model.call([1, 2, 4], [0, 2, 3], [1, 0])
    assert st == 0 and n == 2 and np.array_equal(piece, want[0]) and np.array_equal(rule, want[1]) and np.array_equal(first.astype(np.uint64), want[2])
    assert h.info().deviceTableBytes == 0
    h.destroy()                                            # (closes fl)


def test_example_program_on_its_host_path():
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "flowrules_example"], check=True, stdout=subprocess.PIPE)
    p = subprocess.run([os.path.join(ROOT, "examples", "flowrules_example"), "--host"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout.decode().splitlines() == EXAMPLE_OUTPUT


# `User-Agent:` of flow 1 is cut between batch 0 and 1, `sqlmap` between 1 and 2; the members of flows 0 and 2 end in the last bytes: the flush
EXAMPLE_OUTPUT = [
    "batch 0, flow 1: rule 2 fired (admin page)",
    "batch 2, flow 1: rule 0 fired (sqlmap scanner)",
    "flush, flow 0: rule 0 fired (sqlmap scanner)",
    "flush, flow 2: rule 1 fired (GET and passwd)",
]
