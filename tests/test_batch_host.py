"""PFACX_matchBatchFromHost on the CPU platforms (host-only handles: no device needed) against the oracle run on every segment
separately -- the definition of a batch result (include/pfac_ext.h) -- and the argument checks of the three batch calls."""

import os

import numpy as np
import pytest

from pfac_amd import api
from pfac_amd import workloads as wl

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
PERFS = [(api.PFAC_TIME_DRIVEN, "dense"), (api.PFAC_SPACE_DRIVEN, "hashed")]


def per_segment_oracle(oracle, data, offsets):
    """The expected batch result: the oracle on each segment alone, concatenated."""
    want = np.zeros(data.size, dtype=np.int32)
    for k in range(len(offsets) - 1):
        s, e = int(offsets[k]), int(offsets[k + 1])
        if e > s:
            want[s:e] = oracle.match(data[s:e])
    return want


def _sets(workdir):
    short = [b"a", b"ab", b"b", b"ba", b"abc", b"xyz", b"cab", b"zz"]
    c2 = wl.random_patterns(300)
    out = {}
    for name, pats in (("example", wl.example_patterns()), ("c2", c2), ("short", short)):
        out[name] = (wl.write_pattern_file(os.path.join(workdir, "batch_" + name + ".pat"), pats), pats)
    return out


def _data(name, pats, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    if name == "short":
        data = rng.choice(np.frombuffer(b"abcxyz", dtype=np.uint8), size=n)
    elif name == "example":
        base = np.frombuffer(wl.example_input(), dtype=np.uint8)
        data = np.resize(base, n).copy()
    else:
        data = wl.random_bytes(n, seed=seed).copy()
    for _ in range(max(1, n // 64)):                 # plant patterns everywhere, boundaries included
        p = pats[int(rng.integers(0, len(pats)))]
        at = int(rng.integers(0, max(1, n - len(p))))
        data[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)[:n - at]
    return np.ascontiguousarray(data, dtype=np.uint8)


def _shapes(n, pats, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    shortest = min(len(p) for p in pats)
    cuts = {
        "all-length-1": np.arange(n + 1),
        "empty-first-inside-last": np.concatenate([[0, 0, 0], np.sort(np.concatenate([rng.integers(1, n, 40), [n // 2] * 3])), [n, n, n]]),
        "one-segment": np.array([0, n]),
        "shorter-than-shortest": np.arange(0, n, max(1, shortest - 1)).tolist() + [n],
        "random": np.concatenate([[0], np.sort(rng.integers(0, n + 1, 200)), [n]]),
    }
    return {k: np.ascontiguousarray(np.asarray(v, dtype=np.uint64)) for k, v in cuts.items()}


@pytest.fixture(scope="module")
def sets(workdir):
    return _sets(workdir)


def _handle(pf, platform, perf):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    h.setPerfMode(perf)
    h.readPatternFromFile(pf)
    return h


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("perf,perfname", PERFS)
@pytest.mark.parametrize("setname", ["example", "c2", "short"])
def test_batch_from_host_equals_per_segment_oracle(sets, monkeypatch, setname, platform, pname, perf, perfname):
    from oracle import binding as ob
    if platform == api.PFAC_PLATFORM_CPU_OMP:
        monkeypatch.setenv("OMP_NUM_THREADS", "4")   # CPU_OMP runs threads only with it set (as PFAC_matchFromHost)
    pf, pats = sets[setname]
    data = _data(setname, pats, 3001, seed=17)
    o = ob.Oracle(pf, hashed=False)
    h = _handle(pf, platform, perf)
    try:
        for shape, offs in _shapes(data.size, pats, seed=5).items():
            got = h.match_batch_host_array(data, offs)
            want = per_segment_oracle(o, data, offs)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, f"{setname}/{pname}/{perfname}/{shape}: {bad.size} mismatches, first at {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"
            if shape == "one-segment":
                assert np.array_equal(got, h.match_host_array(data)), "a batch of one segment is the plain call"
    finally:
        h.destroy()
        o.close()


@pytest.mark.parametrize("platform,pname", PLATFORMS)
def test_many_small_segments_in_parallel(sets, monkeypatch, platform, pname):
    """Many short segments: CPU_OMP spreads the segments over its threads."""
    from oracle import binding as ob
    monkeypatch.setenv("OMP_NUM_THREADS", "4")
    pf, pats = sets["c2"]
    data = _data("c2", pats, 1 << 16, seed=3)
    rng = np.random.Generator(np.random.PCG64(9))
    offs = np.concatenate([[0], np.sort(rng.integers(0, data.size, 2000)), [data.size]]).astype(np.uint64)
    o = ob.Oracle(pf, hashed=False)
    h = _handle(pf, platform, api.PFAC_SPACE_DRIVEN)
    try:
        assert np.array_equal(h.match_batch_host_array(data, offs), per_segment_oracle(o, data, offs))
    finally:
        h.destroy()
        o.close()


@pytest.mark.parametrize("perf,perfname", PERFS)
def test_pattern_across_every_boundary_reports_the_shorter_one_inside(workdir, perf, perfname):
    """A long pattern planted across every segment end must not be reported; its prefix, which is a pattern and lies wholly inside
    the segment, must be.  Over the concatenation the long one would win at every one of these positions."""
    from oracle import binding as ob
    pats = [b"GET /admin", b"GET /", b"admin.php", b"min"]
    pf = wl.write_pattern_file(os.path.join(workdir, "batch_straddle.pat"), pats)
    segs, offs = [], [0]
    rng = np.random.Generator(np.random.PCG64(2))
    for k in range(50):
        filler = bytes(rng.choice(np.frombuffer(b"qrstuvw", dtype=np.uint8), size=int(rng.integers(0, 20))))
        seg = (b"admin" if k else b"") + filler + b"GET /"     # the segment ends in "GET /"; the next one begins with "admin"
        segs.append(seg)
        offs.append(offs[-1] + len(seg))
    data = np.frombuffer(b"".join(segs), dtype=np.uint8)
    offs = np.asarray(offs, dtype=np.uint64)
    o = ob.Oracle(pf, hashed=False)
    for platform, _ in PLATFORMS:
        h = _handle(pf, platform, perf)
        try:
            got = h.match_batch_host_array(data, offs)
            plain = h.match_host_array(data)
        finally:
            h.destroy()
        want = per_segment_oracle(o, data, offs)
        assert np.array_equal(got, want)
        ends = [int(e) - 5 for e in offs[1:]]
        assert all(got[p] == 2 for p in ends), "the shorter pattern inside the segment is reported"
        assert all(plain[p] == 1 for p in ends[:-1]), "(over the concatenation the straddling pattern wins)"
    o.close()


def test_invalid_parameters_and_no_ops(sets):
    pf, _ = sets["example"]
    h = _handle(pf, api.PFAC_PLATFORM_CPU, api.PFAC_TIME_DRIVEN)
    lib = api.load_library()
    INV = api.STATUS.INVALID_PARAMETER
    data = np.frombuffer(b"abcdefgh" * 4, dtype=np.uint8).copy()
    n = data.size
    out = np.zeros(n, dtype=np.int32)
    seg_first = np.zeros(8, dtype=np.int32)
    pos = np.zeros(n, dtype=np.int32)

    def offsets(*v):
        return np.asarray(v, dtype=np.uint64)

    good = offsets(0, 10, n)
    try:
        # null pointers
        assert h.matchBatchFromHost(0, n, good.ctypes.data, 2, out.ctypes.data, check=False) == INV
        assert h.matchBatchFromHost(data.ctypes.data, n, 0, 2, out.ctypes.data, check=False) == INV
        assert h.matchBatchFromHost(data.ctypes.data, n, good.ctypes.data, 2, 0, check=False) == INV
        # numSegments == 0 with size > 0
        assert h.matchBatchFromHost(data.ctypes.data, n, good.ctypes.data, 0, out.ctypes.data, check=False) == INV
        # host offsets that break the rules
        for bad in (offsets(1, 10, n), offsets(0, 10, n - 1), offsets(0, 10, n + 1), offsets(0, 20, 10, n)):
            st = h.matchBatchFromHost(data.ctypes.data, n, bad.ctypes.data, bad.size - 1, out.ctypes.data, check=False)
            assert st == INV, bad
        # size == 0: a successful no-op, whatever numSegments says
        out[:] = -3
        assert h.matchBatchFromHost(data.ctypes.data, 0, good.ctypes.data, 0, out.ctypes.data, check=False) == 0
        assert np.all(out == -3)
        # the device forms: the same checks, then a host-only handle has no GPU path
        assert h.matchBatchFromDevice(0, n, good.ctypes.data, 2, out.ctypes.data, check=False) == INV
        assert h.matchBatchFromDevice(data.ctypes.data, n, 0, 2, out.ctypes.data, check=False) == INV
        assert h.matchBatchFromDevice(data.ctypes.data, n, good.ctypes.data, 2, 0, check=False) == INV
        assert h.matchBatchFromDevice(data.ctypes.data, n, good.ctypes.data, 0, out.ctypes.data, check=False) == INV
        assert h.matchBatchFromDevice(data.ctypes.data, 0, good.ctypes.data, 0, out.ctypes.data, check=False) == 0
        assert h.matchBatchFromDevice(data.ctypes.data, n, good.ctypes.data, 2, out.ctypes.data, check=False) == api.STATUS.LIB_NOT_EXIST
        args = [data.ctypes.data, n, good.ctypes.data, 2, out.ctypes.data, pos.ctypes.data, seg_first.ctypes.data]
        for k in (0, 2, 4, 5, 6):
            a = list(args)
            a[k] = 0
            assert h.matchBatchFromDeviceReduce(*a, check=False)[0] == INV, k
        assert lib.PFACX_matchBatchFromDeviceReduce(h._h, *args, None) == INV          # h_num_matched
        a = list(args)
        a[3] = 0
        assert h.matchBatchFromDeviceReduce(*a, check=False)[0] == INV
        a[1] = 0
        assert h.matchBatchFromDeviceReduce(*a, check=False)[0] == 0
        assert h.matchBatchFromDeviceReduce(*args, check=False)[0] == api.STATUS.LIB_NOT_EXIST
        # the host form on the GPU platform of a host-only handle: no silent CPU fallback
        h.setPlatform(api.PFAC_PLATFORM_GPU)
        assert h.matchBatchFromHost(data.ctypes.data, n, good.ctypes.data, 2, out.ctypes.data, check=False) == api.STATUS.LIB_NOT_EXIST
    finally:
        h.destroy()
    # no handle / no patterns
    assert lib.PFACX_matchBatchFromHost(None, data.ctypes.data, n, good.ctypes.data, 2, out.ctypes.data) == api.STATUS.INVALID_HANDLE
    h2 = api.PFAC.createHostOnly()
    try:
        assert h2.matchBatchFromHost(data.ctypes.data, n, good.ctypes.data, 2, out.ctypes.data, check=False) == api.STATUS.PATTERNS_NOT_READY
    finally:
        h2.destroy()
