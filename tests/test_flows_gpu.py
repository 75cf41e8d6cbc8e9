"""Flow sets (PFACX_flows*) on the GPU: PFACX_flowsMatchFromDevice (one compacted scan of the whole buffer, the seam and merge launches
of scan_flows.hip) and PFACX_flowsMatchFromHost on the GPU platform, call by call against tests/flows_ref.py.  Kernel variants and perf
modes, the wave-per-piece and block-per-piece seam shapes, seams staged in device scratch, caseless sets, misaligned buffers, a batch
above 32 MiB, canaries around every array, memory accounting, two threads, and the same schedule through PFACX_streamMatchFromDevice."""

import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from pfac_amd import workloads as wl  # noqa: E402
from tests import flows_ref as fr  # noqa: E402
from tests import nocase_ref as nc  # noqa: E402
from tests import stream_ref as sr  # noqa: E402
from tests.gpu_helpers import make_handle  # noqa: E402
from tests.test_flows_host import FLOWS, caseless_model, hostile_model, small_model  # noqa: E402
from tests.test_stream_host import SMALL, folded_model  # noqa: E402

PAD = 16            # canary entries in front of and behind the arrays


class DeviceFeeder:
    """one flow set of h through the device calls: the batch uploaded at `misalign` bytes into a poisoned buffer, canaries of PAD
    entries in front of and behind d_ids, d_pos (at capacity) and d_pieceFirst, the input compared byte for byte afterwards"""

    def __init__(self, h, m, what, misalign=0):
        self.h, self.m, self.what, self.misalign = h, m, what, misalign
        self.fl = h.flowsOpen(m.F)
        self.M = int(h.info().maxPatternLen)

    def arrays(self, cap, n_first):
        d_ids = torch.full((cap + 2 * PAD,), -7, dtype=torch.int32, device="cuda:0")
        d_pos = torch.full((cap + 2 * PAD,), -7, dtype=torch.int32, device="cuda:0")
        d_first = torch.full((n_first + 2 * PAD,), -7, dtype=torch.int32, device="cuda:0")
        return d_ids, d_pos, d_first

    def check(self, d_ids, d_pos, d_first, cap, n_first):
        for arr, n in ((d_ids, cap), (d_pos, cap), (d_first, n_first)):
            assert bool((arr[:PAD] == -7).all()) and bool((arr[PAD + n:] == -7).all()), f"{self.what}: wrote outside the {n} entries"

    def piece(self, b):
        n, mis = int(b.buf.size), self.misalign
        d_in = torch.full((n + mis + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        if n:
            d_in[mis:mis + n] = torch.from_numpy(b.buf).to("cuda:0")
        image = d_in.clone()
        cap = n + b.flows.size * (self.M - 1)
        d_ids, d_pos, d_first = self.arrays(cap, b.flows.size + 1)
        off, flows = b.offsets.copy(), b.flows.copy()
        offs = np.zeros(b.flows.size, np.uint64)
        _, k = self.fl.match_device(d_in.data_ptr() + mis, n, off.ctypes.data, flows.ctypes.data, flows.size, d_ids.data_ptr() + 4 * PAD,
                                    d_pos.data_ptr() + 4 * PAD, cap, d_first.data_ptr() + 4 * PAD, offs.ctypes.data)
        torch.cuda.synchronize()
        self.check(d_ids, d_pos, d_first, cap, b.flows.size + 1)
        assert bool((d_in == image).all()), f"{self.what}: the caller's buffer (or the bytes around it) was modified"
        assert np.array_equal(off, b.offsets) and np.array_equal(flows, b.flows)
        return d_ids[PAD:PAD + k].cpu().numpy(), d_pos[PAD:PAD + k].cpu().numpy(), d_first[PAD:PAD + flows.size + 1].cpu().numpy(), offs

    def flush(self, flows):
        cap = max(1, flows.size * (self.M - 1))
        d_ids, d_pos, d_first = self.arrays(cap, flows.size + 1)
        mine = flows.copy()
        _, k = self.fl.flush(mine.ctypes.data, mine.size, d_ids.data_ptr() + 4 * PAD, d_pos.data_ptr() + 4 * PAD, cap, d_first.data_ptr() + 4 * PAD)
        torch.cuda.synchronize()
        self.check(d_ids, d_pos, d_first, cap, flows.size + 1)
        return d_ids[PAD:PAD + k].cpu().numpy(), d_pos[PAD:PAD + k].cpu().numpy(), d_first[PAD:PAD + flows.size + 1].cpu().numpy()

    def run(self):
        try:
            fr.run(self.m, self.piece, self.flush, lambda flows: self.fl.reset(flows), self.what)
        finally:
            self.fl.close()


def feed_device(h, m, what, misalign=0):
    DeviceFeeder(h, m, what, misalign).run()


def feed_host(h, m, what):
    fl = h.flowsOpen(m.F)

    def piece(b):
        buf = b.buf.copy()
        out = fl.match_host_array(buf, b.offsets, b.flows)[1:]
        assert np.array_equal(buf, b.buf)
        return out

    try:
        fr.run(m, piece, lambda flows: fl.flush_host_array(flows)[1:], lambda flows: fl.reset(flows), what)
    finally:
        fl.close()


@pytest.mark.parametrize("variant,vname", [(api.PFACX_KERNEL_FILTER, "filter"), (api.PFACX_KERNEL_NAIVE, "naive"), (api.PFACX_KERNEL_AUTO, "auto"),
                                           (api.PFACX_KERNEL_REFTABLE, "reftable")])
@pytest.mark.parametrize("perf,pname", [(api.PFAC_TIME_DRIVEN, "dense"), (api.PFAC_SPACE_DRIVEN, "hashed")])
def test_c3_flows_under_every_kernel_variant_and_perf_mode(workloads, variant, vname, perf, pname):
    """C3's set has M = 60: the wave-per-piece seam"""
    w = workloads["c3"]
    restart = {3: ("flush", 0.5), 9: ("reset", 0.3), 41: ("reset", 0.7), 69: ("flush", 0.9)}
    m = fr.build(w.pattern_file, w.data, FLOWS, 31, restart=restart)
    assert m.M - 1 <= 64
    h = make_handle(w.pattern_file, perf, api.PFAC_AUTOMATIC, variant)
    try:
        feed_device(h, m, f"c3 device {vname}/{pname}")
        feed_host(h, m, f"c3 host-on-gpu {vname}/{pname}")
    finally:
        h.destroy()


@pytest.mark.parametrize("name", SMALL)
def test_small_workloads_device_and_host_on_the_gpu_platform(workloads, name):
    """... and the memory contract: the carries are state (deviceTableBytes, kept by PFACX_trim, back after close), what a call stages
    is scratch (deviceScratchBytes, back after PFACX_trim)"""
    w = workloads[name]
    m = small_model(w, 4000 + SMALL.index(name))
    h = make_handle(w.pattern_file, api.PFAC_SPACE_DRIVEN, api.PFAC_AUTOMATIC, api.PFACX_KERNEL_AUTO)
    try:
        h.trim()
        tables, scratch = h.info().deviceTableBytes, h.info().deviceScratchBytes
        feeder = DeviceFeeder(h, m, f"{name} device")
        first = next(s for s in m.steps if isinstance(s, fr.Batch) and s.buf.size > 0)
        feeder.piece(first)
        if m.M > 1:
            assert h.info().deviceTableBytes >= tables + 2 * m.F * (m.M - 1)
        assert h.info().deviceScratchBytes > scratch
        h.trim()
        assert h.info().deviceScratchBytes == scratch
        if m.M > 1:
            assert h.info().deviceTableBytes >= tables + 2 * m.F * (m.M - 1)         # the carries are state, not scratch
        feeder.fl.reset()
        feeder.run()                                                              # (closes the set)
        assert h.info().deviceTableBytes == tables
        feed_host(h, m, f"{name} host-on-gpu")
        h.trim()
        assert h.info().deviceScratchBytes == scratch
    finally:
        h.destroy()


@pytest.mark.parametrize("which", ["snort-lengths", "long", "huge", "m1"])
def test_hostile_sets(workdir, which):
    """snort-lengths (M = 243) and long (M = 2000) take the block-per-piece seam; huge (M = 25 000) stages its seams in device scratch;
    m1 has no seams at all"""
    pf, m = hostile_model(workdir, which, 77)
    if which == "huge":
        # seams of more than 48 KiB: [carry | head of the piece] of a flow with a full carry and a piece longer than 48 KiB - (M - 1)
        seen, beyond = {}, 0
        for s in m.steps:
            if isinstance(s, fr.Batch):
                for f, ln in zip(s.flows.tolist(), np.diff(s.offsets.astype(np.int64)).tolist()):
                    beyond += ln > 0 and min(m.M - 1, seen.get(f, 0)) + min(ln, m.M - 1) > (48 << 10)
                    seen[f] = seen.get(f, 0) + ln
        assert beyond >= 2
    h = make_handle(pf, api.PFAC_TIME_DRIVEN, api.PFAC_AUTOMATIC, api.PFACX_KERNEL_AUTO)
    try:
        feed_device(h, m, f"{which} device")
        feed_host(h, m, f"{which} host-on-gpu")
    finally:
        h.destroy()


def test_caseless_set(workdir):
    for name, (pats, data) in nc.mixed_sets().items():
        pf, _, _ = folded_model(workdir, "flows_gpu_" + name, pats, data)
        m = fr.build(pf, data, 5, 91, whole=True, fold=nc.fold_array, big=False)
        assert m.straddling >= min(20, m.longer)
        h = api.PFAC.create()
        try:
            h.readPatternFromMemoryEx(nc.pattern_bytes(pats), api.PFACX_READ_NOCASE)
            feed_device(h, m, f"nocase {name} device")
            feed_device(h, m, f"nocase {name} device + 3", misalign=3)
            feed_host(h, m, f"nocase {name} host-on-gpu")
        finally:
            h.destroy()


@pytest.mark.parametrize("which", ["long", "huge"])
def test_caseless_sets_in_batches_of_70_flows_on_the_block_and_the_scratch_seams(workdir, which):
    """a folding set through the block-per-piece seam (M = 150) and through seams staged in device scratch (M = 25 000), 70 flows, the
    model's full coverage asserted; misaligned too"""
    pf, raw, m = caseless_model(workdir, which)
    h = api.PFAC.create()
    try:
        h.readPatternFromMemoryEx(raw, api.PFACX_READ_NOCASE)
        assert h.info().maxPatternLen == m.M
        feed_device(h, m, f"nocase {which} device", misalign=0 if which == "huge" else 5)
        if which == "long":
            feed_host(h, m, f"nocase {which} host-on-gpu")
    finally:
        h.destroy()


@pytest.mark.parametrize("misalign", [1, 2, 3, 5, 7, 8, 13, 15])
def test_misaligned_buffer_starts(workloads, misalign):
    w = workloads["c2"]
    m = fr.build(w.pattern_file, w.data[:300000], FLOWS, 200 + misalign)
    h = make_handle(w.pattern_file, api.PFAC_TIME_DRIVEN, api.PFAC_AUTOMATIC, api.PFACX_KERNEL_FILTER)
    try:
        feed_device(h, m, f"c2 + {misalign}", misalign=misalign)
    finally:
        h.destroy()


def test_a_batch_above_32_mib_runs_the_filter_kernel_under_the_merge(workdir):
    """three batches of 70 pieces over 3 x 34 MiB of C3-style traffic (odd piece sizes, one piece of 20 MiB): PFACX_KERNEL_AUTO scans a
    buffer of that size with the filter kernel; flow f's stream is its three pieces in a row"""
    pats = wl.snort_patterns(3000)
    pf = wl.write_pattern_file(os.path.join(workdir, "flows_big.pat"), pats)
    M = int(sr.pattern_lengths(pf).max())
    rng = np.random.Generator(np.random.PCG64(8))
    per_batch = (34 << 20) + 4321
    data = np.array(wl.http_stream(3 * per_batch, wl.http_message_pool(pats, pool_size=512, embed_fraction=0.2)), dtype=np.uint8)      # (a writable copy)
    from oracle import binding as ob
    lengths = sr.pattern_lengths(pf)
    batches, streams = [], [[] for _ in range(FLOWS)]
    for b in range(3):
        cuts = np.sort(rng.choice(np.arange(1, per_batch - (20 << 20)), size=FLOWS - 1, replace=False))
        cuts[cuts > (5 << 20)] += 20 << 20                   # one piece of more than 20 MiB
        edges = np.concatenate([[0], cuts, [per_batch]]).astype(np.int64)
        order = rng.permutation(FLOWS)
        batches.append((data[b * per_batch:(b + 1) * per_batch], edges, order))
        for k, f in enumerate(order):
            streams[f].append(data[b * per_batch + edges[k]:b * per_batch + edges[k + 1]])
    # an occurrence across every junction of a flow's pieces: random cuts alone hit none (the pieces are views of `data`)
    long_enough = [p for p in pats if len(p) >= 8]
    for f in range(FLOWS):
        for b in range(2):
            p = np.frombuffer(long_enough[(7 * f + b) % len(long_enough)], dtype=np.uint8)
            head = 1 + (f + b) % (p.size - 1)
            if streams[f][b].size >= head and streams[f][b + 1].size >= p.size - head:
                streams[f][b][streams[f][b].size - head:] = p[:head]
                streams[f][b + 1][:p.size - head] = p[head:]
    o = ob.Oracle(pf, hashed=False)
    expected, straddling = [], 0
    try:
        for f in range(FLOWS):
            whole = np.concatenate(streams[f])
            full = o.match(whole, omp=True)
            pos = np.flatnonzero(full > 0).astype(np.int64)
            ids = full[pos].astype(np.int32)
            sizes = [p.size for p in streams[f]]
            straddling += sr.straddling(pos, ids, lengths, sizes)
            expected.append(sr.split(pos, ids, sizes, M))
    finally:
        o.close()
    assert straddling >= 64
    h = make_handle(pf, api.PFAC_SPACE_DRIVEN, api.PFAC_AUTOMATIC, api.PFACX_KERNEL_AUTO)
    try:
        fl = h.flowsOpen(FLOWS)
        cap = per_batch + FLOWS * (M - 1)
        d_ids = torch.full((cap + 2 * PAD,), -7, dtype=torch.int32, device="cuda:0")
        d_pos = torch.full((cap + 2 * PAD,), -7, dtype=torch.int32, device="cuda:0")
        d_first = torch.full((FLOWS + 1 + 2 * PAD,), -7, dtype=torch.int32, device="cuda:0")
        for b, (buf, edges, order) in enumerate(batches):
            d_in = torch.from_numpy(np.ascontiguousarray(buf)).to("cuda:0")
            off, flows, offs = edges.astype(np.uintp), order.astype(np.uint32), np.zeros(FLOWS, np.uint64)
            _, k = fl.match_device(d_in.data_ptr(), per_batch, off.ctypes.data, flows.ctypes.data, FLOWS, d_ids.data_ptr() + 4 * PAD, d_pos.data_ptr() + 4 * PAD,
                                   cap, d_first.data_ptr() + 4 * PAD, offs.ctypes.data)
            torch.cuda.synchronize()
            want = [expected[f][0][b] for f in order]
            assert k == sum(wn[0].size for wn in want)
            assert np.array_equal(d_ids[PAD:PAD + k].cpu().numpy(), np.concatenate([wn[0] for wn in want]))
            assert np.array_equal(d_pos[PAD:PAD + k].cpu().numpy(), np.concatenate([wn[1] for wn in want]))
            assert np.array_equal(d_first[PAD:PAD + FLOWS + 1].cpu().numpy(), np.concatenate([[0], np.cumsum([wn[0].size for wn in want])]))
            assert np.array_equal(offs, np.array([wn[2] for wn in want], np.uint64))
            assert bool((d_in.cpu() == torch.from_numpy(np.ascontiguousarray(buf))).all())
            for arr, n in ((d_ids, cap), (d_pos, cap), (d_first, FLOWS + 1)):
                assert bool((arr[:PAD] == -7).all()) and bool((arr[PAD + n:] == -7).all())
        every = np.arange(FLOWS, dtype=np.uint32)
        _, k = fl.flush(every.ctypes.data, FLOWS, d_ids.data_ptr() + 4 * PAD, d_pos.data_ptr() + 4 * PAD, cap, d_first.data_ptr() + 4 * PAD)
        assert np.array_equal(d_ids[PAD:PAD + k].cpu().numpy(), np.concatenate([expected[f][1][0] for f in range(FLOWS)]))
        assert np.array_equal(d_pos[PAD:PAD + k].cpu().numpy(), np.concatenate([expected[f][1][1] for f in range(FLOWS)]))
        fl.close()
    finally:
        h.destroy()


def test_two_threads_drive_two_flow_sets_of_one_handle(workloads):
    w = workloads["c3"]
    models = [fr.build(w.pattern_file, w.data[:400000], FLOWS, 61), fr.build(w.pattern_file, w.data[400000:800000], FLOWS, 62)]
    h = make_handle(w.pattern_file, api.PFAC_SPACE_DRIVEN, api.PFAC_AUTOMATIC, api.PFACX_KERNEL_AUTO)
    errors = []

    def work(k):
        try:
            torch.cuda.set_device(0)
            feed_device(h, models[k], f"thread {k}")
        except BaseException as e:              # noqa: BLE001
            errors.append(e)

    try:
        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
    finally:
        h.destroy()


def test_the_same_schedule_piece_by_piece_through_the_stream_calls_gives_the_identical_arrays(workloads):
    """the cross-check against the existing code: F streams fed with PFACX_streamMatchFromDevice, concatenated per batch"""
    w = workloads["c5"]
    m = fr.build(w.pattern_file, w.data, FLOWS, 73)
    h = make_handle(w.pattern_file, api.PFAC_TIME_DRIVEN, api.PFAC_AUTOMATIC, api.PFACX_KERNEL_AUTO)
    try:
        M = int(h.info().maxPatternLen)
        streams = [h.streamOpen() for _ in range(m.F)]
        feeder = DeviceFeeder(h, m, "c5 flows")
        biggest = max(int(np.diff(s.offsets.astype(np.int64)).max()) for s in m.steps if isinstance(s, fr.Batch))
        cap = biggest + M
        s_ids = torch.empty(cap, dtype=torch.int32, device="cuda:0")
        s_pos = torch.empty(cap, dtype=torch.int32, device="cuda:0")
        for step in m.steps:
            if isinstance(step, fr.Batch):
                ids, pos, first, offs = feeder.piece(step)
                d_in = torch.from_numpy(step.buf if step.buf.size else np.zeros(1, np.uint8)).to("cuda:0")
                got_ids, got_pos, got_first, got_offs = [], [], [0], []
                for k, f in enumerate(step.flows.tolist()):
                    a, b = int(step.offsets[k]), int(step.offsets[k + 1])
                    _, n, off = streams[f].match_device(d_in.data_ptr() + a, b - a, s_ids.data_ptr(), s_pos.data_ptr(), cap)
                    got_ids.append(s_ids[:n].cpu().numpy())
                    got_pos.append(s_pos[:n].cpu().numpy())
                    got_first.append(got_first[-1] + n)
                    got_offs.append(off)
                assert np.array_equal(ids, np.concatenate(got_ids)) and np.array_equal(pos, np.concatenate(got_pos))
                assert np.array_equal(first, np.array(got_first)) and np.array_equal(offs, np.array(got_offs, np.uint64))
            elif step.kind == "flush":
                ids, pos, first = feeder.flush(step.flows)
                got_ids, got_pos = [], []
                for f in step.flows.tolist():
                    _, n = streams[f].flush(s_ids.data_ptr(), s_pos.data_ptr(), cap)
                    got_ids.append(s_ids[:n].cpu().numpy())
                    got_pos.append(s_pos[:n].cpu().numpy())
                assert np.array_equal(ids, np.concatenate(got_ids)) and np.array_equal(pos, np.concatenate(got_pos))
        feeder.fl.close()
    finally:
        h.destroy()


def test_refused_device_calls_leave_every_flow_unchanged_and_kinds_do_not_mix(workloads):
    w = workloads["c2"]
    m = fr.build(w.pattern_file, w.data[:300000], FLOWS, 5)
    h = make_handle(w.pattern_file, api.PFAC_TIME_DRIVEN, api.PFAC_AUTOMATIC, api.PFACX_KERNEL_AUTO)
    bad = api.STATUS.INVALID_PARAMETER
    try:
        feeder = DeviceFeeder(h, m, "c2 device with refused calls")
        M = feeder.M
        plain = feeder.piece
        fed = [False]

        def piece(b):
            n = int(b.buf.size)
            d_in = torch.from_numpy(b.buf if n else np.zeros(1, np.uint8)).to("cuda:0")
            cap = n + b.flows.size * (M - 1)
            d_ids, d_pos, d_first = feeder.arrays(cap, b.flows.size + 1)
            offs = np.zeros(b.flows.size, np.uint64)

            def call(off, flows, capacity):
                st, _ = feeder.fl.match_device(d_in.data_ptr(), n, off.ctypes.data, flows.ctypes.data, flows.size, d_ids.data_ptr() + 4 * PAD,
                                               d_pos.data_ptr() + 4 * PAD, capacity, d_first.data_ptr() + 4 * PAD, offs.ctypes.data, check=False)
                return st

            if b.flows.size >= 2:
                twice = b.flows.copy()
                twice[-1] = twice[0]
                assert call(b.offsets, twice, cap) == bad
                beyond = b.flows.copy()
                beyond[0] = m.F
                assert call(b.offsets, beyond, cap) == bad
            if n:
                off = b.offsets.copy()
                off[-1] -= 1
                assert call(off, b.flows, cap) == bad
            if cap:
                assert call(b.offsets, b.flows, cap - 1) == bad
            if fed[0] and n:
                st = feeder.fl.match_host_array(b.buf, b.offsets, b.flows, check=False)[0]
                assert st == bad                          # a host call on a device-fed set
            fed[0] = fed[0] or n > 0
            return plain(b)

        feeder.piece = piece
        feeder.run()
        # a new pattern set: refused until the reset of all flows
        b = next(s for s in m.steps if isinstance(s, fr.Batch) and s.buf.size > 4 * M)
        feeder2 = DeviceFeeder(h, m, "after a new set")
        h.readPatternFromFile(w.pattern_file)
        d_in = torch.from_numpy(b.buf).to("cuda:0")
        cap = b.buf.size + b.flows.size * (M - 1)
        d_ids, d_pos, d_first = feeder2.arrays(cap, b.flows.size + 1)
        offs = np.zeros(b.flows.size, np.uint64)
        st, _ = feeder2.fl.match_device(d_in.data_ptr(), b.buf.size, b.offsets.ctypes.data, b.flows.ctypes.data, b.flows.size, d_ids.data_ptr() + 4 * PAD,
                                        d_pos.data_ptr() + 4 * PAD, cap, d_first.data_ptr() + 4 * PAD, offs.ctypes.data, check=False)
        assert st == bad
        feeder2.fl.reset()
        feeder2.run()
    finally:
        h.destroy()
