"""Flow sets (PFACX_flows*) on the CPU platforms: host-only handles, no device needed.

Every call of a seeded schedule of many flows (tests/flows_ref.py) is compared with the model: the oracle's list over each flow's bytes,
split by the finality rule call by call (tests/stream_ref.py), concatenated in piece order.  Small workloads, the hostile sets of
tests/test_stream_host.py, a caseless set, flushes and resets of some flows in the middle of a schedule, and every refused call
followed by the same call done right -- the state was untouched."""

import os

import numpy as np
import pytest

from pfac_amd import api
from tests import flows_ref as fr
from tests import nocase_ref as nc
from tests import stream_ref as sr
from tests.test_stream_host import GRID, GRID_IDS, PERFS, PLATFORMS, SMALL, folded_model, hostile_case, host_handle

FLOWS = 70          # more than 64: the first batches of a schedule name every flow


def feed(h, m, what):
    """the model's schedule through the host calls of one flow set; the caller's arrays must stay as they were"""
    fl = h.flowsOpen(m.F)

    def piece(b):
        buf, off, flows = b.buf.copy(), b.offsets.copy(), b.flows.copy()
        _, ids, pos, first, offs = fl.match_host_array(buf, off, flows)
        assert np.array_equal(buf, b.buf) and np.array_equal(off, b.offsets) and np.array_equal(flows, b.flows), f"{what}: input arrays were modified"
        return ids, pos, first, offs

    def flush(flows):
        mine = flows.copy()
        _, ids, pos, first = fl.flush_host_array(mine)
        assert np.array_equal(mine, flows)
        return ids, pos, first

    try:
        fr.run(m, piece, flush, lambda flows: fl.reset(flows), what)
    finally:
        fl.close()


def small_model(w, seed, **kw):
    if w.data.size > 16384:
        return fr.build(w.pattern_file, w.data, FLOWS, seed, **kw)
    return fr.build(w.pattern_file, w.data, 3, seed, whole=True, big=False, **kw)      # (c1 and ex2 are a dozen bytes)


@pytest.mark.parametrize("name", SMALL)
def test_small_workloads_in_batches_of_many_flows(workloads, name):
    w = workloads[name]
    m = small_model(w, 4000 + SMALL.index(name))
    for (platform, pname), (perf, fname) in [(a, b) for a in PLATFORMS for b in PERFS]:
        h = host_handle(w.pattern_file, perf=perf, platform=platform)
        try:
            assert h.info().maxPatternLen == m.M
            feed(h, m, f"{name}/{pname}/{fname}")
        finally:
            h.destroy()


def hostile_model(workdir, which, seed):
    """the hostile sets cut as tests/test_stream_host.py cuts them, 70 flows (long and huge: every flow the whole stream, cut its own way)"""
    pf, data, _ = hostile_case(workdir, which)
    from tests.test_stream_host import huge_sizes, short_piece_sizes
    if which == "huge":
        return pf, fr.build(pf, data, FLOWS, seed, whole=True, sizes_of=lambda n, M, p, i, l, s: [0] + huge_sizes(n, M, s))
    lo, hi = {"snort-lengths": (5, 40), "long": (30, 90), "m1": (1, 9)}[which]
    sizes_of = lambda n, M, p, i, l, s: [0, 1] + short_piece_sizes(n - 1, lo, hi, s) if n > 1 else [0, n]      # noqa: E731
    return pf, fr.build(pf, data, FLOWS, seed, whole=(which == "long"), sizes_of=sizes_of)


@pytest.mark.parametrize("platform,perf", GRID, ids=GRID_IDS)
@pytest.mark.parametrize("which", ["snort-lengths", "long", "huge", "m1"])
def test_hostile_sets(workdir, which, platform, perf):
    pf, m = hostile_model(workdir, which, 77)
    if which == "huge":
        assert m.M == 25000 and m.straddling >= 2
    h = host_handle(pf, perf=perf, platform=platform)
    try:
        feed(h, m, which)
    finally:
        h.destroy()


@pytest.mark.parametrize("platform,perf", GRID, ids=GRID_IDS)
def test_caseless_set(workdir, platform, perf):
    for name, (pats, data) in nc.mixed_sets().items():
        pf, _, _ = folded_model(workdir, "flows_" + name, pats, data)
        m = fr.build(pf, data, 5, 91, whole=True, fold=nc.fold_array, big=False)
        assert m.straddling >= min(20, m.longer)
        h = host_handle(raw=nc.pattern_bytes(pats), flags=api.PFACX_READ_NOCASE, perf=perf, platform=platform)
        try:
            feed(h, m, f"nocase {name}")
        finally:
            h.destroy()


def caseless_model(workdir, which):
    """(folded pattern file, pattern bytes as the handle reads them, model) of a caseless set in 70 flows with the model's full coverage:
    `long` -- mixed-case patterns up to 150 bytes (M - 1 > 64) planted case-flipped in mixed-case text; `huge` -- the hostile set of
    25 000 bytes over its stream with half the letters flipped"""
    rng = np.random.Generator(np.random.PCG64(4242))
    if which == "huge":
        from tests.test_stream_host import huge_sizes
        pf, data, _ = hostile_case(workdir, "huge")
        with open(pf, "rb") as f:
            raw = f.read()
        data = nc.flip_array(data, rng)
        return pf, raw, fr.build(pf, data, FLOWS, 79, whole=True, fold=nc.fold_array, sizes_of=lambda n, M, p, i, l, s: [0] + huge_sizes(n, M, s))
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 /._-", dtype=np.uint8)
    pats = {b"Ab", b"xYz", b"PassWD"}
    while len(pats) < 80:
        ln = int(rng.integers(3, 40)) if rng.random() < 0.85 else int(rng.integers(100, 151))
        pats.add(alpha[rng.integers(0, alpha.size, ln)].tobytes())
    pats = sorted(pats)
    pats.append(alpha[rng.integers(0, alpha.size, 150)].tobytes())
    data = alpha[rng.integers(0, alpha.size, 280000)].copy()
    for _ in range(1500):
        p = np.frombuffer(nc.flip_case(pats[int(rng.integers(0, len(pats)))], rng), dtype=np.uint8)
        at = int(rng.integers(0, data.size - 200))
        data[at:at + p.size] = p
    pf = nc.write_patterns(os.path.join(workdir, "flows_nocase_long.pat"), [nc.fold(p) for p in pats])
    m = fr.build(pf, data, FLOWS, 83, fold=nc.fold_array)
    assert m.M == 150
    return pf, nc.pattern_bytes(pats), m


@pytest.mark.parametrize("platform,perf", GRID, ids=GRID_IDS)
@pytest.mark.parametrize("which", ["long", "huge"])
def test_caseless_sets_in_batches_of_70_flows(workdir, which, platform, perf):
    pf, raw, m = caseless_model(workdir, which)
    h = host_handle(raw=raw, flags=api.PFACX_READ_NOCASE, perf=perf, platform=platform)
    try:
        assert h.info().maxPatternLen == m.M
        feed(h, m, f"nocase {which}")
    finally:
        h.destroy()


@pytest.mark.parametrize("platform,perf", GRID, ids=GRID_IDS)
def test_partial_flush_and_partial_reset_in_the_middle_of_a_schedule(workloads, platform, perf):
    w = workloads["c3"]
    restart = {3: ("flush", 0.5), 9: ("reset", 0.3), 10: ("flush", 0.3), 41: ("reset", 0.7), 69: ("flush", 0.9)}
    m = fr.build(w.pattern_file, w.data, FLOWS, 17, restart=restart)
    kinds = [s.kind for s in m.steps[:-1] if isinstance(s, fr.End)]
    assert kinds.count("flush") >= 2 and kinds.count("reset") >= 2
    h = host_handle(w.pattern_file, perf=perf, platform=platform)
    try:
        feed(h, m, "c3 with restarts")
    finally:
        h.destroy()


def test_refused_calls_leave_every_flow_unchanged(workloads):
    """a flow named twice, an id >= numFlows, bad offsets, short capacity, the other kind of call, a new pattern set until a full reset:
    each INVALID_PARAMETER, each followed by the same call done right, which returns what the model expects"""
    w = workloads["c2"]
    m = fr.build(w.pattern_file, w.data[:300000], FLOWS, 5)
    h = host_handle(w.pattern_file)
    fl = h.flowsOpen(m.F)
    M = m.M
    bad = api.STATUS.INVALID_PARAMETER
    refused = 0

    def raw(buf, off, flows, cap, n_pieces=None):
        n_pieces = flows.size if n_pieces is None else n_pieces
        ids = np.full(cap + 1, -7, np.int32)
        pos = np.full(cap + 1, -7, np.int32)
        first = np.full(n_pieces + 1, -7, np.int32)
        offs = np.zeros(max(1, n_pieces), np.uint64)
        b = buf if buf.size else np.zeros(1, np.uint8)
        st, n = fl.match_host(b.ctypes.data, buf.size, off.ctypes.data, flows.ctypes.data, n_pieces, ids.ctypes.data, pos.ctypes.data, cap,
                              first.ctypes.data, offs.ctypes.data, check=False)
        assert ids[cap] == -7 and pos[cap] == -7
        return st

    def piece(b):
        nonlocal refused
        need = b.buf.size + b.flows.size * (M - 1)
        if b.flows.size >= 2:
            twice = b.flows.copy()
            twice[-1] = twice[0]
            assert raw(b.buf, b.offsets, twice, need) == bad
            beyond = b.flows.copy()
            beyond[b.flows.size // 2] = m.F
            assert raw(b.buf, b.offsets, beyond, need) == bad
            refused += 2
        if b.buf.size:
            off = b.offsets.copy()
            off[-1] -= 1
            assert raw(b.buf, off, b.flows, need) == bad                  # the last offset is not the size
            off = b.offsets.copy()
            off[0] = 1
            assert raw(b.buf, off, b.flows, need) == bad                  # the first is not 0
            if b.flows.size >= 3 and b.offsets[1] < b.offsets[2]:
                off = b.offsets.copy()
                off[1], off[2] = off[2], off[1]
                assert raw(b.buf, off, b.flows, need) == bad              # decreasing
            refused += 2
        if need:
            assert raw(b.buf, b.offsets, b.flows, need - 1) == bad
            refused += 1
        if fl_kind[0]:
            # the device form on this host-fed set: the wrong kind before anything else is looked at on a host-only handle ... or no device
            ids = np.zeros(need + 1, np.int32)
            offs = np.zeros(b.flows.size, np.uint64)
            st, _ = fl.match_device(b.buf.ctypes.data if b.buf.size else ids.ctypes.data, b.buf.size, b.offsets.ctypes.data, b.flows.ctypes.data, b.flows.size,
                                    ids.ctypes.data, ids.ctypes.data, need + 1, ids.ctypes.data, offs.ctypes.data, check=False)
            assert st == (bad if b.buf.size else api.STATUS.LIB_NOT_EXIST)
        _, ids, pos, first, offs = fl.match_host_array(b.buf, b.offsets, b.flows)
        fl_kind[0] = fl_kind[0] or b.buf.size > 0
        return ids, pos, first, offs

    def flush(flows):
        nonlocal refused
        cap = max(1, flows.size * (M - 1))
        ids = np.zeros(cap, np.int32)
        first = np.zeros(flows.size + 1, np.int32)
        st, _ = fl.flush(flows.ctypes.data, flows.size, ids.ctypes.data, ids.ctypes.data, cap - 1, first.ctypes.data, check=False)
        assert st == bad
        twice = np.concatenate([flows, flows[:1]])
        st, _ = fl.flush(twice.ctypes.data, twice.size, ids.ctypes.data, ids.ctypes.data, cap + M, np.zeros(twice.size + 1, np.int32).ctypes.data, check=False)
        assert st == bad
        refused += 2
        _, ids, pos, first = fl.flush_host_array(flows)
        return ids, pos, first

    fl_kind = [False]
    try:
        fr.run(m, piece, flush, lambda flows: fl.reset(flows), "c2 with refused calls")
        assert refused > 500
        # a new pattern set: everything is refused until the reset of all flows; a partial reset does not adopt the set
        b = next(s for s in m.steps if isinstance(s, fr.Batch) and s.buf.size > 4 * M)
        h.readPatternFromFile(w.pattern_file)
        assert raw(b.buf, b.offsets, b.flows, b.buf.size + b.flows.size * (M - 1)) == bad
        st, _, _, _ = fl.flush_host_array(b.flows, check=False)
        assert st == bad
        fl.reset(b.flows)
        assert raw(b.buf, b.offsets, b.flows, b.buf.size + b.flows.size * (M - 1)) == bad
        fl.reset()
        feed_again = fr.build(w.pattern_file, w.data[:300000], FLOWS, 5)
        fr.run(feed_again, lambda s: fl.match_host_array(s.buf, s.offsets, s.flows)[1:], lambda f: fl.flush_host_array(f)[1:], lambda f: fl.reset(f), "after the reset")
    finally:
        h.destroy()                                      # closes the flow set


def test_arguments_and_lifetime(golden_dir):
    pf = os.path.join(golden_dir, "example_pattern")
    data = np.fromfile(os.path.join(golden_dir, "example_input"), dtype=np.uint8).copy()      # ABEDEDABG\n, M = 4
    h = host_handle(pf)
    try:
        lib = api.load_library()
        assert lib.PFACX_flowsOpen(h._h, 4, None) == api.STATUS.INVALID_PARAMETER
        assert h.flowsOpen(0, check=False).status == api.STATUS.INVALID_PARAMETER
        assert lib.PFACX_flowsClose(None) == api.STATUS.INVALID_HANDLE
        fl = h.flowsOpen(4)
        before = h.info().deviceTableBytes
        # AB | G across two batches of flow 2, with flow 0 in between and an empty piece for flow 3
        st, ids, pos, first, offs = fl.match_host_array(data[:8], [0, 8, 8], [2, 3])
        assert list(zip(pos.tolist(), ids.tolist())) == [(0, 1), (1, 3), (2, 4), (4, 4)] and list(first) == [0, 4, 4] and list(offs) == [0, 0]
        st, ids, pos, first, offs = fl.match_host_array(np.concatenate([data[:4], data[8:]]), [0, 4, 6], [0, 2])
        assert list(zip(pos.tolist(), ids.tolist())) == [(0, 1), (-2, 2)] and list(first) == [0, 1, 2] and list(offs) == [0, 8]
        assert h.info().deviceTableBytes == before          # a host-fed set carries its bytes in host memory
        h.trim()
        st, ids, pos, first = fl.flush_host_array([3, 0, 2])
        want0 = sr.split(*sr.full_list(pf, data[:4]), [4], 4)[1]          # flow 0 saw ABED, flow 2 the whole input, flow 3 nothing
        want2 = sr.split(*sr.full_list(pf, data), [8, 2], 4)[1]
        assert np.array_equal(ids, np.concatenate([want0[0], want2[0]])) and np.array_equal(pos, np.concatenate([want0[1], want2[1]]))
        assert list(first) == [0, 0, want0[0].size, want0[0].size + want2[0].size] and want0[0].size >= 1
        st, ids, pos, first = fl.flush_host_array([0, 1, 2, 3])      # twice: nothing
        assert ids.size == 0 and list(first) == [0, 0, 0, 0, 0]
        # null pointers
        off = np.array([0, 10], np.uintp)
        flows = np.array([1], np.uint32)
        out = np.zeros(32, np.int32)
        offs = np.zeros(1, np.uint64)
        n = api.C.c_int(0)
        good = [fl._f, data.ctypes.data, 10, off.ctypes.data, flows.ctypes.data, 1, out.ctypes.data, out.ctypes.data, 32, out.ctypes.data, offs.ctypes.data, api.C.byref(n)]
        for k in (1, 3, 4, 6, 7, 9, 10, 11):
            a = list(good)
            a[k] = None
            assert lib.PFACX_flowsMatchFromHost(*a) == api.STATUS.INVALID_PARAMETER, k
        a = list(good)
        a[0] = None
        assert lib.PFACX_flowsMatchFromHost(*a) == api.STATUS.INVALID_HANDLE
        assert lib.PFACX_flowsMatchFromHost(*good) == 0 and n.value == 5      # the five pairs below 10 - 3
        # numPieces == 0: only with size == 0
        a = list(good)
        a[5] = 0
        assert lib.PFACX_flowsMatchFromHost(*a) == api.STATUS.INVALID_PARAMETER
        a[2] = 0
        assert lib.PFACX_flowsMatchFromHost(*a) == 0 and n.value == 0
        # the device form on a host-only handle
        fresh = h.flowsOpen(2)
        a = list(good)
        a[0] = fresh._f
        assert lib.PFACX_flowsMatchFromDevice(*a) == api.STATUS.LIB_NOT_EXIST
        fresh.close()
        empty = api.PFAC.createHostOnly()
        assert empty.flowsOpen(3, check=False).status == api.STATUS.PATTERNS_NOT_READY
        empty.destroy()
    finally:
        h.destroy()                                      # (closes the flow set that is still open)
