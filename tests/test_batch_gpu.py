"""PFACX_matchBatchFromDevice / ...FromDeviceReduce / ...FromHost on the GPU against the oracle run on every segment separately
(include/pfac_ext.h: the batch result IS the concatenation of the per-segment results) -- in every kernel variant, walker, perf
mode and texture mode, with guards around the result, misaligned pointers, both sides of the 32 MiB line of PFACX_KERNEL_AUTO."""

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from pfac_amd import workloads as wl  # noqa: E402
from tests.gpu_helpers import MODES, VARIANTS, make_handle, perf_asserts  # noqa: E402

SENTINEL = -5
GUARD = 64


def per_segment_oracle(o, data, offsets):
    want = np.zeros(data.size, dtype=np.int32)
    for k in range(len(offsets) - 1):
        s, e = int(offsets[k]), int(offsets[k + 1])
        if e > s:
            want[s:e] = o.match(data[s:e], omp=e - s > (1 << 20))
    return want


def device_batch(h, data, offsets, in_offset=0, out_offset=0):
    """matchBatchFromDevice with the result in a sentinel-filled buffer between guard words; every element must be written and no
    guard touched.  in_offset / out_offset misalign the input (bytes) and result (ints) pointers."""
    n = int(data.size)
    d_in = torch.zeros(n + in_offset + GUARD, dtype=torch.uint8, device="cuda:0")
    d_in[in_offset:in_offset + n] = torch.from_numpy(np.array(data, dtype=np.uint8)).to("cuda:0")
    d_out = torch.full((GUARD + out_offset + n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    d_off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64)).to("cuda:0")
    h.matchBatchFromDevice(d_in.data_ptr() + in_offset, n, d_off.data_ptr(), len(offsets) - 1, d_out.data_ptr() + 4 * (GUARD + out_offset))
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(out[:GUARD + out_offset] == SENTINEL) and np.all(out[GUARD + out_offset + n:] == SENTINEL), "a guard word was written"
    got = out[GUARD + out_offset:GUARD + out_offset + n]
    return got


def check(got, want, what):
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"{what}: {bad.size} mismatches; first at {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}")


def http_segments(pool, count, seed):
    """`count` messages of the C3 pool (placeholders filled) as one buffer + its offsets"""
    rng = np.random.Generator(np.random.PCG64(seed))
    url = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789-._~/", dtype=np.uint8)
    parts, offs = [], [0]
    for i in rng.integers(0, len(pool), count):
        m = np.frombuffer(pool[int(i)], dtype=np.uint8).copy()
        z = m == 0
        m[z] = rng.choice(url, size=int(z.sum()))
        parts.append(m)
        offs.append(offs[-1] + m.size)
    return np.concatenate(parts), np.asarray(offs, dtype=np.uint64)


def random_cuts(n, max_len, seed, min_len=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = rng.integers(min_len, max_len + 1, n // max(1, (min_len + max_len) // 2) + 16)
    offs = np.concatenate([[0], np.cumsum(lens)])
    offs = offs[offs < n]
    return np.concatenate([offs, [n]]).astype(np.uint64)


@pytest.fixture(scope="module")
def shapes(workloads):
    """{set: [(shape name, data, offsets)]} over the small C2 / C3 / C5 workloads"""
    out = {}
    pool = wl.http_message_pool(wl.snort_patterns(3000), pool_size=512, embed_fraction=0.2)
    for name in ("c2", "c3", "c5"):
        w = workloads[name]
        d = w.data[:1 << 20]
        items = [("random-0..4096", d, random_cuts(d.size, 4096, seed=7)),
                 ("1-byte", d[:4096], np.arange(4097, dtype=np.uint64))]
        if name == "c3":
            hd, ho = http_segments(pool, 1500, seed=3)
            items.append(("http-messages", hd, ho))
        out[name] = items
    return out


@pytest.fixture(scope="module")
def expected(workloads, shapes):
    from oracle import binding as ob
    res = {}
    for name, items in shapes.items():
        o = ob.Oracle(workloads[name].pattern_file, hashed=False)
        for shape, data, offs in items:
            res[(name, shape)] = per_segment_oracle(o, data, offs)
        o.close()
    return res


@pytest.mark.parametrize("perf,tex,mode_name", MODES)
@pytest.mark.parametrize("variant,vname", VARIANTS)
@pytest.mark.parametrize("name", ["c2", "c3", "c5"])
def test_batch_from_device_equals_per_segment_oracle(workloads, shapes, expected, name, variant, vname, perf, tex, mode_name):
    h = make_handle(workloads[name].pattern_file, perf, tex, variant)
    try:
        for shape, data, offs in shapes[name]:
            check(device_batch(h, data, offs), expected[(name, shape)], f"{name}/{vname}/{mode_name}/{shape}")
        shape, data, offs = shapes[name][0]
        check(device_batch(h, data, offs, in_offset=3, out_offset=1), expected[(name, shape)], f"{name}/{vname}/{mode_name}/misaligned")
    finally:
        h.destroy()


@pytest.mark.parametrize("walker", [api.PFACX_WALKER_AUTO, api.PFACX_WALKER_WINDOW, api.PFACX_WALKER_STAGE, api.PFACX_WALKER_VETO])
def test_batch_every_walker(workloads, shapes, expected, walker):
    for name in ("c3", "c5"):
        h = make_handle(workloads[name].pattern_file, api.PFAC_SPACE_DRIVEN, api.PFAC_AUTOMATIC, api.PFACX_KERNEL_FILTER)
        h.setWalker(walker)
        try:
            for shape, data, offs in shapes[name]:
                check(device_batch(h, data, offs), expected[(name, shape)], f"{name}/walker {walker}/{shape}")
        finally:
            h.destroy()


@pytest.fixture(scope="module")
def big(workloads):
    """C3-set input of 40 MiB + a few KiB: one 40 MiB segment among tiny ones (the AUTO path above 32 MiB), and its first 24 MiB
    as a batch of HTTP-sized segments (below the line)"""
    from oracle import binding as ob
    pool = wl.http_message_pool(wl.snort_patterns(3000), pool_size=512, embed_fraction=0.2)
    data = wl.http_stream((40 << 20) + 5000, pool, seed=99)
    rng = np.random.Generator(np.random.PCG64(4))
    tiny = np.cumsum(rng.integers(0, 9, 300))
    offs = np.concatenate([[0], tiny, tiny[-1] + (40 << 20) + tiny, [data.size]])
    offs = np.minimum(offs, data.size).astype(np.uint64)
    small = data[:24 << 20]
    small_offs = random_cuts(small.size, 3000, seed=8, min_len=60)
    o = ob.Oracle(workloads["c3"].pattern_file, hashed=False)
    out = {"above": (data, offs, per_segment_oracle(o, data, offs)), "below": (small, small_offs, per_segment_oracle(o, small, small_offs))}
    o.close()
    return out


@pytest.mark.parametrize("perf,tex,mode_name", MODES)
@pytest.mark.parametrize("variant", [api.PFACX_KERNEL_AUTO, api.PFACX_KERNEL_FILTER, api.PFACX_KERNEL_NAIVE])
def test_batch_both_sides_of_the_auto_line(workloads, big, variant, perf, tex, mode_name):
    h = make_handle(workloads["c3"].pattern_file, perf, tex, variant)
    try:
        for side, (data, offs, want) in big.items():
            check(device_batch(h, data, offs), want, f"variant {variant}/{mode_name}/{side} 32 MiB")
    finally:
        h.destroy()


@pytest.mark.parametrize("perf,tex,mode_name", MODES)
def test_one_segment_is_the_plain_call(workloads, perf, tex, mode_name):
    for name in ("c2", "c3", "c5", "dense_hits", "binary"):
        w = workloads[name]
        h = make_handle(w.pattern_file, perf, tex, api.PFACX_KERNEL_AUTO)
        try:
            n = int(w.data.size)
            d_in = torch.from_numpy(w.data.copy()).to("cuda:0")
            plain = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda:0")
            h.matchFromDevice(d_in.data_ptr(), n, plain.data_ptr())
            got = device_batch(h, w.data, np.array([0, n], dtype=np.uint64))
            torch.cuda.synchronize()
            assert np.array_equal(got, plain.cpu().numpy()), f"{name}/{mode_name}"
        finally:
            h.destroy()


@pytest.mark.parametrize("variant,vname", VARIANTS)
def test_hostile_every_position_matches(workdir, variant, vname):
    """Every position matches and segments are 1-7 bytes: every zone position is re-walked."""
    from oracle import binding as ob
    pats = [b"a" * k for k in range(1, 9)] + [b"ab", b"aab"]
    pf = wl.write_pattern_file(os.path.join(workdir, "batch_hostile.pat"), pats)
    data = np.frombuffer(b"a" * 200000 + b"ab" * 1000 + b"a" * 3001, dtype=np.uint8)
    offs = random_cuts(data.size, 7, seed=1, min_len=1)
    o = ob.Oracle(pf, hashed=False)
    want = per_segment_oracle(o, data, offs)
    o.close()
    assert np.all(want[data == ord('a')] != 0)
    for perf, tex, mode_name in MODES:
        h = make_handle(pf, perf, tex, variant)
        try:
            check(device_batch(h, data, offs), want, f"hostile/{vname}/{mode_name}")
        finally:
            h.destroy()


def reduce_batch(h, data, offs):
    n = int(data.size)
    nseg = len(offs) - 1
    d_in = torch.from_numpy(np.array(data, dtype=np.uint8)).to("cuda:0")
    d_ids = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    d_pos = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    d_first = torch.full((nseg + 1 + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    d_off = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.uint64).view(np.int64)).to("cuda:0")
    _, count = h.matchBatchFromDeviceReduce(d_in.data_ptr(), n, d_off.data_ptr(), nseg, d_ids.data_ptr(), d_pos.data_ptr(), d_first.data_ptr())
    torch.cuda.synchronize()
    ids, pos, first = d_ids.cpu().numpy(), d_pos.cpu().numpy(), d_first.cpu().numpy()
    assert np.all(ids[n:] == SENTINEL) and np.all(pos[n:] == SENTINEL) and np.all(first[nseg + 1:] == SENTINEL), "wrote past an array"
    return count, ids[:count], pos[:count], first[:nseg + 1]


def check_reduce(h, data, offs, want, what):
    count, ids, pos, first = reduce_batch(h, data, offs)
    nz = np.nonzero(want)[0]
    assert count == nz.size, f"{what}: count {count} != {nz.size}"
    assert np.array_equal(pos, nz), f"{what}: positions"
    assert np.array_equal(ids, want[nz]), f"{what}: ids"
    want_first = np.searchsorted(nz, offs.astype(np.int64), side="left")
    assert np.array_equal(first, want_first), f"{what}: segFirst"


@pytest.mark.parametrize("perf,tex,mode_name", MODES)
def test_batch_reduce_equals_per_segment_oracle(workloads, shapes, expected, workdir, perf, tex, mode_name):
    from oracle import binding as ob
    for name in ("c2", "c3", "c5"):
        for variant in (api.PFACX_KERNEL_AUTO, api.PFACX_KERNEL_FILTER):
            h = make_handle(workloads[name].pattern_file, perf, tex, variant)
            try:
                for shape, data, offs in shapes[name]:
                    check_reduce(h, data, offs, expected[(name, shape)], f"{name}/{variant}/{mode_name}/{shape}")
            finally:
                h.destroy()
    # drops: the straddling pattern has no shorter one inside the segment; empty segments first, inside and last
    pats = [b"GET /admin", b"min.php", b"qq"]
    pf = wl.write_pattern_file(os.path.join(workdir, "batch_drop.pat"), pats)
    rng = np.random.Generator(np.random.PCG64(6))
    segs, offs = [b"", b""], [0, 0, 0]
    for k in range(3000):
        seg = b"admin" + bytes(rng.choice(np.frombuffer(b"qrs", dtype=np.uint8), size=int(rng.integers(0, 12)))) + b"GET /"
        segs.append(seg)
        offs.append(offs[-1] + len(seg))
        if k % 100 == 0:
            offs.append(offs[-1])
    offs += [offs[-1], offs[-1]]
    data = np.frombuffer(b"".join(segs), dtype=np.uint8)
    offs = np.asarray(offs, dtype=np.uint64)
    o = ob.Oracle(pf, hashed=False)
    want = per_segment_oracle(o, data, offs)
    plain = o.match(data)
    o.close()
    assert np.count_nonzero(plain == 1) > 2000 and np.count_nonzero(want == 1) == 0
    for variant in (api.PFACX_KERNEL_AUTO, api.PFACX_KERNEL_FILTER, api.PFACX_KERNEL_NAIVE):
        h = make_handle(pf, perf, tex, variant)
        try:
            check_reduce(h, data, offs, want, f"drops/{variant}/{mode_name}")
            check(device_batch(h, data, offs), want, f"drops full/{variant}/{mode_name}")
        finally:
            h.destroy()


@pytest.mark.parametrize("perf", [api.PFAC_TIME_DRIVEN, api.PFAC_SPACE_DRIVEN])
def test_batch_from_host_on_gpu_platform(workloads, perf):
    """80 MiB through the 32 Mi-position pieces: segments straddle the pieces, one segment is longer than a piece."""
    from oracle import binding as ob
    pf = workloads["c2"].pattern_file
    pats = wl.random_patterns()
    n = 80 << 20
    data = wl.random_bytes(n, seed=123).copy()
    rng = np.random.Generator(np.random.PCG64(12))
    for at in list(rng.integers(0, n - 64, 5000)) + [(32 << 20) - 3, (64 << 20) - 5, (32 << 20) - 20]:
        p = pats[int(rng.integers(0, len(pats)))]
        data[int(at):int(at) + len(p)] = np.frombuffer(p, dtype=np.uint8)
    cuts = list(np.cumsum(rng.integers(0, 1 << 20, 30)))
    cuts = [c for c in cuts if c < (20 << 20)] + [20 << 20, (20 << 20) + (40 << 20), (32 << 20) + (40 << 20) - 2]   # [20, 60) MiB: longer than a piece
    cuts += [(64 << 20) - 1, (64 << 20) + 7, (64 << 20) + 7]
    offs = np.asarray(sorted(set([0] + [int(c) for c in cuts])) + [n], dtype=np.uint64)
    # segment ends right behind planted patterns: walks that the end cuts short
    o = ob.Oracle(pf, hashed=False)
    want = per_segment_oracle(o, data, offs)
    o.close()
    h = make_handle(pf, perf, api.PFAC_AUTOMATIC, api.PFACX_KERNEL_AUTO)
    try:
        got = h.match_batch_host_array(data, offs)
        check(got, want, "GPU host form")
        small, so = data[:100000], random_cuts(100000, 300, seed=2)
        o = ob.Oracle(pf, hashed=False)
        check(h.match_batch_host_array(small, so), per_segment_oracle(o, small, so), "GPU host form, one piece")
        o.close()
    finally:
        h.destroy()


def test_trim_and_table_bytes(workloads, shapes, expected):
    w = workloads["c3"]
    h = make_handle(w.pattern_file, api.PFAC_SPACE_DRIVEN, api.PFAC_AUTOMATIC, api.PFACX_KERNEL_AUTO)
    try:
        shape, data, offs = shapes["c3"][0]
        before = h.info().deviceTableBytes
        check(device_batch(h, data, offs), expected[("c3", shape)], "first")
        assert h.info().deviceTableBytes == before, "a batch call leaves the table bytes alone"
        assert h.info().deviceScratchBytes > 0
        count, *_ = reduce_batch(h, data, offs)
        h.trim()
        assert h.info().deviceScratchBytes == 0
        check(device_batch(h, data, offs), expected[("c3", shape)], "after trim")
        h.trim()
        assert reduce_batch(h, data, offs)[0] == count
        assert h.info().deviceTableBytes == before
    finally:
        h.destroy()


def test_batch_rate(workloads):
    """Batch call vs plain call over the same 16 MiB (C3 stream, 1.5 KiB segments); asserted only under PFAC_PERF_FLOORS."""
    from pfac_amd import hiprt
    pool = wl.http_message_pool(wl.snort_patterns(3000), pool_size=512, embed_fraction=0.2)
    n = 16 << 20
    data = wl.http_stream(n, pool, seed=5)
    offs = np.arange(0, n, 1536, dtype=np.uint64).tolist() + [n]
    h = make_handle(workloads["c3"].pattern_file, api.PFAC_SPACE_DRIVEN, api.PFAC_AUTOMATIC, api.PFACX_KERNEL_AUTO)
    try:
        d_in = torch.from_numpy(data).to("cuda:0")
        d_out = torch.empty(n, dtype=torch.int32, device="cuda:0")
        d_off = torch.tensor(offs, dtype=torch.int64, device="cuda:0")

        def rate(fn, steps=20):
            fn()
            torch.cuda.synchronize()
            a, b = hiprt.Event(), hiprt.Event()
            a.record(0)
            for _ in range(steps):
                fn()
            b.record(0)
            torch.cuda.synchronize()
            return n / (a.elapsed_ms(b) / steps / 1e3) / 1e9
        plain = rate(lambda: h.matchFromDevice(d_in.data_ptr(), n, d_out.data_ptr()))
        batch = rate(lambda: h.matchBatchFromDevice(d_in.data_ptr(), n, d_off.data_ptr(), len(offs) - 1, d_out.data_ptr()))
        print(f"16 MiB C3, 1.5 KiB segments: batch {batch:.0f} GB/s, plain {plain:.0f} GB/s, ratio {batch / plain:.3f}")
        if perf_asserts():
            assert batch >= 0.8 * plain
    finally:
        h.destroy()
