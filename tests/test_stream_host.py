"""Streams (PFACX_stream*) on the CPU platforms: host-only handles, no device needed.

The contract of include/pfac_ext.h is checked call by call against tests/stream_ref.py: the oracle's list over the whole stream S,
split by the finality rule into what each piece call and the flush return.  The reference's known answer cut everywhere, every small
workload under placed and mixed cuts, hostile sets whose occurrences span dozens of calls, caseless handles, state and arguments."""

import os

import numpy as np
import pytest

from pfac_amd import api
from pfac_amd import workloads as wl
from tests import nocase_ref as nc
from tests import stream_ref as sr

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
PERFS = [(api.PFAC_TIME_DRIVEN, "dense"), (api.PFAC_SPACE_DRIVEN, "hashed")]
GRID = [(pl, pf) for pl, _ in PLATFORMS for pf, _ in PERFS]
GRID_IDS = [f"{a}-{b}" for _, a in PLATFORMS for _, b in PERFS]
SMALL = ["c1", "ex2", "c2", "c3", "c5", "dense_hits", "binary"]


def host_handle(pattern_file=None, raw=None, flags=0, perf=api.PFAC_TIME_DRIVEN, platform=api.PFAC_PLATFORM_CPU):
    h = api.PFAC.createHostOnly()
    h.setPerfMode(perf)
    h.setPlatform(platform)
    if raw is None:
        with open(pattern_file, "rb") as f:
            raw = f.read()
    h.readPatternFromMemoryEx(raw, flags)
    return h


def feed(h, data, sizes, calls, flush, what):
    """one stream of h through the host calls, compared call by call; the caller's bytes must stay as they were"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    before = data.copy()
    s = h.streamOpen()
    try:
        sr.run(lambda off, size: s.match_host_array(data[off:off + size]), s.flush_host_array, data, sizes, calls, flush, what)
    finally:
        s.close()
    assert np.array_equal(data, before), f"{what}: the caller's pieces were modified"


@pytest.mark.parametrize("platform,perf", GRID, ids=GRID_IDS)
def test_known_answer_cut_everywhere(golden_dir, platform, perf):
    """example_pattern x example_input (ABEDEDABG\\n) cut at each of its 9 inner positions and into 10 pieces of one byte: AB|G gives
    ABG at the position of A and never AB (id 1) -- which is what a caller gets today from one PFAC_matchFromHostReduce per piece
    (asserted too: the bug this feature closes).  ABG is the second line of the committed example_pattern, so its id is 2 here (the
    oracle's list below says so), not 3."""
    pf = os.path.join(golden_dir, "example_pattern")
    data = np.fromfile(os.path.join(golden_dir, "example_input"), dtype=np.uint8)
    assert data.tobytes() == b"ABEDEDABG\n"
    with open(pf, "rb") as f:
        assert f.read().split(b"\n")[:4] == [b"AB", b"ABG", b"BEDE", b"ED"]       # ids 1..4 by line: ABG is 2
    pos, ids = sr.full_list(pf, data)
    assert list(zip(pos.tolist(), ids.tolist())) == [(0, 1), (1, 3), (2, 4), (4, 4), (6, 2)]
    h = host_handle(pf, perf=perf, platform=platform)
    try:
        M = h.info().maxPatternLen
        assert M == 4
        for cut in range(1, data.size):
            sizes = [cut, data.size - cut]
            calls, flush = sr.split(pos, ids, sizes, M)
            feed(h, data, sizes, calls, flush, f"cut at {cut}")
        sizes = [1] * data.size
        calls, flush = sr.split(pos, ids, sizes, M)
        feed(h, data, sizes, calls, flush, "one byte per piece")
        # AB|G: the stream reports ABG (id 2) at the position of A ...
        s = h.streamOpen()
        got = []
        for a, b in ((0, 8), (8, 10)):
            i, p, off = s.match_host_array(data[a:b])
            got += [(int(off) + int(q), int(k)) for q, k in zip(p, i)]
        i, p = s.flush_host_array()
        got += [(data.size + int(q), int(k)) for q, k in zip(p, i)]
        s.close()
        assert (6, 2) in got and (6, 1) not in got and got == list(zip(pos.tolist(), ids.tolist()))
        # ... where one plain call per piece reports AB (id 1): silently wrong for a stream
        out_ids = np.zeros(8, np.int32)
        out_pos = np.zeros(8, np.int32)
        piece = data[:8].copy()
        _, n = h.matchFromHostReduce(piece.ctypes.data, 8, out_ids.ctypes.data, out_pos.ctypes.data)
        assert (6, 1) in list(zip(out_pos[:n].tolist(), out_ids[:n].tolist()))
    finally:
        h.destroy()


@pytest.mark.parametrize("name", SMALL)
def test_small_workloads_under_placed_and_mixed_cuts(workloads, name):
    """every small workload, cuts placed inside occurrences + the sizes 0, 1, M-2 .. M+1, KiB pieces and runs of pieces shorter than
    M; both CPU platforms, dense and hashed.  The model says how many occurrences straddle a cut: a test whose cuts miss every
    occurrence proves nothing."""
    w = workloads[name]
    pos, ids = sr.full_list(w.pattern_file, w.data)
    lengths = sr.pattern_lengths(w.pattern_file)
    M = int(lengths.max())
    sizes = sr.make_sizes(w.data.size, M, pos, ids, lengths, seed=1000 + SMALL.index(name))
    crossing = sr.straddling(pos, ids, lengths, sizes)
    longer = int(np.count_nonzero(lengths[ids] >= 2))
    assert crossing >= min(20, longer), (name, crossing, longer)
    if name == "dense_hits":
        # positions that one plain call per piece would give another id (the oracle over the bytes up to the piece's end says which)
        assert sr.per_piece_differs(w.pattern_file, w.data, pos, ids, lengths, sizes) >= 5
    if w.data.size > 16384:            # (c1 and ex2 are a dozen bytes: cut everywhere in the test above)
        assert 0 in sizes and 1 in sizes and M - 2 in sizes and M - 1 in sizes and M in sizes and M + 1 in sizes and max(sizes) > 4096
        assert max(len(run) for run in "".join("s" if 0 < x < M else "L" for x in sizes).split("L")) >= 20      # a run of many pieces shorter than M
    calls, flush = sr.split(pos, ids, sizes, M)
    assert sum(c[0].size for c in calls) + flush[0].size == pos.size
    for (platform, pname), (perf, fname) in [(a, b) for a in PLATFORMS for b in PERFS]:
        h = host_handle(w.pattern_file, perf=perf, platform=platform)
        try:
            assert h.info().maxPatternLen == M
            feed(h, w.data, sizes, calls, flush, f"{name}/{pname}/{fname}")
        finally:
            h.destroy()


def hostile_snort_lengths(workdir):
    """a set with lengths 1..243, 1- and 2-byte patterns included, over text with long patterns planted"""
    rng = np.random.Generator(np.random.PCG64(2431))
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789 /.-_=&%:", dtype=np.uint8)
    pats = {b"q", b"Z", b"zq", b"0x", b"%%"}
    while len(pats) < 300:
        u = rng.random()
        ln = int(rng.integers(1, 3)) if u < 0.01 else int(rng.integers(3, 40)) if u < 0.8 else int(rng.integers(40, 244))
        pats.add(alpha[rng.integers(0, alpha.size, ln)].tobytes())
    pats = sorted(pats)
    pats.append(alpha[rng.integers(0, alpha.size, 243)].tobytes())
    n = 48 << 10
    data = alpha[rng.integers(0, alpha.size, n)].copy()
    for k in range(60):
        p = np.frombuffer(pats[int(rng.integers(0, len(pats)))], dtype=np.uint8)
        at = int(rng.integers(0, n - 300))
        data[at:at + p.size] = p
    data[n - 400:n - 400 + 243] = np.frombuffer(pats[-1], dtype=np.uint8)
    return wl.write_pattern_file(os.path.join(workdir, "stream_snortlen.pat"), pats), data


def hostile_long(workdir):
    """600- and 2000-byte patterns (and their prefixes' neighbours) over a stream that holds them and near misses of them"""
    rng = np.random.Generator(np.random.PCG64(77))
    long2000 = rng.integers(97, 123, 2000).astype(np.uint8)
    long600 = rng.integers(97, 123, 600).astype(np.uint8)
    pats = [long2000.tobytes(), long600.tobytes(), long2000[:50].tobytes() + b"#", b"xyz", long600[100:130].tobytes()]
    n = 24 << 10
    data = rng.integers(97, 123, n).astype(np.uint8)
    data[1000:3000] = long2000
    data[5000:5600] = long600
    data[7000:8990] = long2000[:1990]              # a near miss, ten bytes short
    data[12000:14000] = long2000
    data[n - 2000:] = long2000                     # ends with the stream
    data[16000:16599] = long600[:599]
    return wl.write_pattern_file(os.path.join(workdir, "stream_long.pat"), pats), data


def short_piece_sizes(n, lo, hi, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    sizes = []
    left = n
    while left:
        s = min(left, int(rng.integers(lo, hi + 1)))
        sizes.append(s)
        left -= s
    return sizes


def hostile_huge(workdir):
    """one pattern of 25 000 bytes (and short ones): 2 (M - 1) bytes do not fit the seam launch's LDS stage, which a device-fed stream
    then keeps in device scratch; two occurrences and a near miss"""
    rng = np.random.Generator(np.random.PCG64(78))
    huge = rng.integers(97, 123, 25000).astype(np.uint8)
    pats = [huge.tobytes(), huge[:40].tobytes() + b"#", b"xyz", huge[20000:20030].tobytes()]
    n = 150000
    data = rng.integers(97, 123, n).astype(np.uint8)
    data[3000:28000] = huge
    data[40000:64990] = huge[:24990]               # a near miss, ten bytes short
    data[70000:95000] = huge
    data[n - 24000:] = huge[:24000]                # cut off by the end of the stream
    return wl.write_pattern_file(os.path.join(workdir, "stream_huge.pat"), pats), data


def huge_sizes(n, M, seed):
    """small pieces and pieces of about M bytes in turn: with a full carry, a piece of more than 48 KiB - (M - 1) bytes makes the
    seam longer than the LDS stage"""
    rng = np.random.Generator(np.random.PCG64(seed))
    sizes, left, k = [], n, 0
    while left:
        s = int(rng.integers(300, 3000)) if k % 6 != 5 else int(rng.integers(M - 700, M + 6000))
        s = min(s, left)
        sizes.append(s)
        left -= s
        k += 1
    return sizes


def seams_beyond(sizes, M, limit):
    """how many piece calls stage more than `limit` bytes of [carry | first min(size, M - 1) bytes of the piece]"""
    T = count = 0
    for size in sizes:
        count += size > 0 and min(M - 1, T) + min(size, M - 1) > limit
        T += size
    return count


def hostile_case(workdir, which):
    """(pattern file, stream, piece sizes) of the hostile sets"""
    if which == "snort-lengths":
        pf, data = hostile_snort_lengths(workdir)
        return pf, data, short_piece_sizes(data.size, 5, 40, 1)
    if which == "long":
        pf, data = hostile_long(workdir)
        return pf, data, short_piece_sizes(data.size, 30, 90, 2)
    if which == "huge":
        pf, data = hostile_huge(workdir)
        return pf, data, huge_sizes(data.size, 25000, 5)
    pf = wl.write_pattern_file(os.path.join(workdir, "stream_m1.pat"), [b"a", b"b", b"\xff"])
    data = np.frombuffer(b"abcab\xffcc" * 300, dtype=np.uint8)
    return pf, data, [0, 1, 2, 0, 700] + short_piece_sizes(data.size - 703, 1, 9, 3)


@pytest.mark.parametrize("platform,perf", GRID, ids=GRID_IDS)
@pytest.mark.parametrize("which", ["snort-lengths", "long", "huge", "m1"])
def test_hostile_sets_in_pieces_far_shorter_than_the_longest_pattern(workdir, which, platform, perf):
    """M = 243 with 1-byte patterns in pieces of 5..40 bytes; M = 2000 in pieces of 30..90 bytes (one occurrence spans dozens of
    calls); M = 25 000 in small and pattern-sized pieces; a set with M == 1 (nothing is ever pending: every call reports its own
    positions, the flush nothing).  Both CPU platforms, dense and hashed."""
    pf, data, sizes = hostile_case(workdir, which)
    pos, ids = sr.full_list(pf, data)
    lengths = sr.pattern_lengths(pf)
    M = int(lengths.max())
    calls, flush = sr.split(pos, ids, sizes, M)
    cuts = np.cumsum(sizes)
    longest = int(np.argmax(lengths[ids])) if pos.size else 0
    inside_longest = int(np.count_nonzero((cuts > pos[longest]) & (cuts < pos[longest] + M)))
    if which == "m1":
        assert M == 1 and flush[0].size == 0 and all(np.all(c[1] >= 0) for c in calls)
    elif which == "huge":
        assert M == 25000 and inside_longest >= 3 and sr.straddling(pos, ids, lengths, sizes) >= 2      # (both occurrences of the long pattern)
        assert seams_beyond(sizes, M, 48 << 10) >= 2          # calls whose [carry | head of the piece] exceeds the seam launch's LDS stage
    else:
        assert M > 4 * max(sizes)
        assert sr.straddling(pos, ids, lengths, sizes) >= (20 if which == "snort-lengths" else 4)      # (the long set has six occurrences)
        assert inside_longest >= (6 if which == "snort-lengths" else 24)      # one occurrence, that many calls
    h = host_handle(pf, perf=perf, platform=platform)
    try:
        feed(h, data, sizes, calls, flush, which)
    finally:
        h.destroy()


def folded_model(workdir, name, pats, data):
    pf = nc.write_patterns(os.path.join(workdir, "stream_nocase_" + name + ".pat"), [nc.fold(p) for p in pats])
    pos, ids = sr.full_list(pf, nc.fold_array(data))
    return pf, pos, ids


@pytest.mark.parametrize("platform,perf", GRID, ids=GRID_IDS)
def test_caseless_streams(workdir, platform, perf):
    """a PFACX_READ_NOCASE handle: the folded set over the folded stream (tests/nocase_ref.py), same cuts; the caller's pieces stay"""
    for name, (pats, data) in nc.mixed_sets().items():
        pf, pos, ids = folded_model(workdir, name, pats, data)
        lengths = sr.pattern_lengths(pf)
        M = int(lengths.max())
        sizes = sr.make_sizes(data.size, M, pos, ids, lengths, seed=55)
        assert sr.straddling(pos, ids, lengths, sizes) >= min(20, int(np.count_nonzero(lengths[ids] >= 2)))
        calls, flush = sr.split(pos, ids, sizes, M)
        h = host_handle(raw=nc.pattern_bytes(pats), flags=api.PFACX_READ_NOCASE, perf=perf, platform=platform)
        try:
            feed(h, data, sizes, calls, flush, f"nocase {name}")
        finally:
            h.destroy()


@pytest.mark.parametrize("platform,perf", GRID, ids=GRID_IDS)
def test_caseless_cut_between_an_upper_and_a_lower_case_byte(workdir, platform, perf):
    pats = [b"HeLLo", b"hell", b"LOW"]
    data = np.frombuffer(b"..hEllO..HELlow", dtype=np.uint8).copy()
    pf, pos, ids = folded_model(workdir, "cut", pats, data)
    assert (2 in pos) and (9 in pos)
    h = host_handle(raw=nc.pattern_bytes(pats), flags=api.PFACX_READ_NOCASE, perf=perf, platform=platform)
    try:
        for cut in range(1, data.size):               # 3|4 is between 'h' 'E', 4|5 between 'E' 'l', ...
            sizes = [cut, data.size - cut]
            calls, flush = sr.split(pos, ids, sizes, 5)
            feed(h, data, sizes, calls, flush, f"nocase cut {cut}")
    finally:
        h.destroy()


def test_two_streams_of_one_handle_do_not_see_each_others_bytes(golden_dir):
    pf = os.path.join(golden_dir, "example_pattern")
    h = host_handle(pf)
    try:
        a, b = h.streamOpen(), h.streamOpen()
        x = np.frombuffer(b"..AB", dtype=np.uint8)
        y = np.frombuffer(b"G...AB", dtype=np.uint8)
        got_a, got_b = [], []
        for piece_a, piece_b in ((x, y), (y, x)):
            i, p, off = a.match_host_array(piece_a)
            got_a += [(off + int(q), int(k)) for q, k in zip(p, i)]
            i, p, off = b.match_host_array(piece_b)
            got_b += [(off + int(q), int(k)) for q, k in zip(p, i)]
        i, p = a.flush_host_array()
        got_a += [(10 + int(q), int(k)) for q, k in zip(p, i)]
        i, p = b.flush_host_array()
        got_b += [(10 + int(q), int(k)) for q, k in zip(p, i)]
        assert got_a == [(2, 2), (8, 1)]              # ..ABG...AB
        assert got_b == [(4, 1), (8, 1)]              # G...AB..AB
    finally:
        h.destroy()


def test_reset_flush_twice_and_reuse(golden_dir):
    pf = os.path.join(golden_dir, "example_pattern")
    data = np.fromfile(os.path.join(golden_dir, "example_input"), dtype=np.uint8)
    pos, ids = sr.full_list(pf, data)
    h = host_handle(pf)
    try:
        s = h.streamOpen()
        s.match_host_array(data[:8])
        s.reset()                                        # the carried AB is forgotten
        i, p, off = s.match_host_array(data[8:])
        assert off == 0 and i.size == 0
        i, p = s.flush_host_array()
        assert i.size == 0
        i, p = s.flush_host_array()                      # twice: nothing
        assert i.size == 0
        calls, flush = sr.split(pos, ids, [3, 7], 4)     # reuse after the flush: a fresh stream
        sr.run(lambda off, size: s.match_host_array(data[off:off + size]), s.flush_host_array, data, [3, 7], calls, flush, "reuse")
        s.close()
    finally:
        h.destroy()


def test_a_new_pattern_set_invalidates_until_reset(golden_dir):
    pf = os.path.join(golden_dir, "example_pattern")
    data = np.fromfile(os.path.join(golden_dir, "example_input"), dtype=np.uint8)
    h = host_handle(pf)
    try:
        s = h.streamOpen()
        s.match_host_array(data[:8])
        h.readPatternFromMemory(b"BG\nEDAB\n")
        cap = 64
        ids = np.zeros(cap, np.int32)
        pos = np.zeros(cap, np.int32)
        piece = data[8:].copy()
        st, _, _ = s.match_host(piece.ctypes.data, piece.size, ids.ctypes.data, pos.ctypes.data, cap, check=False)
        assert st == api.STATUS.INVALID_PARAMETER
        st, _ = s.flush(ids.ctypes.data, pos.ctypes.data, cap, check=False)
        assert st == api.STATUS.INVALID_PARAMETER
        s.reset()
        i, p, off = s.match_host_array(data)             # the new set, from the start: EDAB at 4, BG at 7
        j, q = s.flush_host_array()
        assert off == 0 and list(zip(np.concatenate([p, q + data.size]).tolist(), np.concatenate([i, j]).tolist())) == [(4, 2), (7, 1)]
        s.close()
    finally:
        h.destroy()


def test_arguments(golden_dir):
    pf = os.path.join(golden_dir, "example_pattern")
    data = np.fromfile(os.path.join(golden_dir, "example_input"), dtype=np.uint8).copy()
    h = host_handle(pf)
    try:
        s = h.streamOpen()
        M = h.info().maxPatternLen
        cap = data.size + M
        ids = np.full(cap + 4, -7, np.int32)
        pos = np.full(cap + 4, -7, np.int32)
        args = (data.ctypes.data, data.size, ids.ctypes.data, pos.ctypes.data)
        # capacity one short: refused, the stream unchanged -- the repeated call gives the model's answer
        st, n, _ = s.match_host(*args, cap - 1, check=False)
        assert st == api.STATUS.INVALID_PARAMETER
        st, n, off = s.match_host(*args, cap)
        assert (st, n, off) == (0, 5, 0) and np.all(ids[cap:] == -7) and np.all(pos[cap:] == -7)
        st, _ = s.flush(ids.ctypes.data, pos.ctypes.data, M - 1, check=False)
        assert st == api.STATUS.INVALID_PARAMETER
        # null pointers
        lib = api.load_library()
        n_out, off_out = api.C.c_int(0), api.C.c_ulonglong(0)
        for k in range(4):
            a = [data.ctypes.data, ids.ctypes.data, pos.ctypes.data]
            if k < 3:
                a[k] = None
            st = lib.PFACX_streamMatchFromHost(s._s, a[0], data.size, a[1], a[2], cap, api.C.byref(n_out) if k < 3 else None, api.C.byref(off_out))
            assert st == api.STATUS.INVALID_PARAMETER
        assert lib.PFACX_streamMatchFromHost(s._s, data.ctypes.data, data.size, ids.ctypes.data, pos.ctypes.data, cap, api.C.byref(n_out), None) == api.STATUS.INVALID_PARAMETER
        assert lib.PFACX_streamMatchFromHost(None, data.ctypes.data, data.size, ids.ctypes.data, pos.ctypes.data, cap, api.C.byref(n_out), api.C.byref(off_out)) == api.STATUS.INVALID_HANDLE
        assert lib.PFACX_streamFlush(s._s, None, pos.ctypes.data, cap, api.C.byref(n_out)) == api.STATUS.INVALID_PARAMETER
        assert lib.PFACX_streamOpen(h._h, None) == api.STATUS.INVALID_PARAMETER
        # size 0: success, nothing reported, the stream unchanged
        st, n, off = s.match_host(data.ctypes.data, 0, ids.ctypes.data, pos.ctypes.data, 0)
        assert (st, n, off) == (0, 0, data.size)
        # size >= 2^31
        st, _, _ = s.match_host(data.ctypes.data, 1 << 31, ids.ctypes.data, pos.ctypes.data, (1 << 31) + M, check=False)
        assert st == api.STATUS.INVALID_PARAMETER
        # a device call on this host-fed stream: the wrong kind; on a fresh stream of a host-only handle: no device
        st, _, _ = s.match_device(data.ctypes.data, data.size, ids.ctypes.data, pos.ctypes.data, cap, check=False)
        assert st == api.STATUS.INVALID_PARAMETER
        t = h.streamOpen()
        st, _, _ = t.match_device(data.ctypes.data, data.size, ids.ctypes.data, pos.ctypes.data, cap, check=False)
        assert st == api.STATUS.LIB_NOT_EXIST
        t.close()
        s.close()
        empty = api.PFAC.createHostOnly()
        assert empty.streamOpen(check=False).status == api.STATUS.PATTERNS_NOT_READY
        empty.destroy()
    finally:
        h.destroy()                                      # (closes the streams that are still open)


def test_destroy_closes_open_streams_and_info_counts_nothing_for_host_streams(golden_dir):
    h = host_handle(os.path.join(golden_dir, "example_pattern"))
    before = h.info().deviceTableBytes
    s = h.streamOpen()
    s.match_host_array(np.frombuffer(b"xxAB", dtype=np.uint8))
    assert h.info().deviceTableBytes == before          # a host-fed stream carries its bytes in host memory
    h.trim()
    i, p, off = s.match_host_array(np.frombuffer(b"G", dtype=np.uint8))     # the carry survives PFACX_trim
    j, q = s.flush_host_array()
    assert off == 4 and list(q + 5) == [2] and list(j) == [2] and i.size == 0
    h.destroy()


@pytest.mark.parametrize("platform,perf", GRID, ids=GRID_IDS)
def test_a_loaded_compiled_set_streams_like_the_read_one(workloads, workdir, platform, perf):
    w = workloads["c2"]
    data = w.data[:200000]
    pos, ids = sr.full_list(w.pattern_file, data)
    lengths = sr.pattern_lengths(w.pattern_file)
    M = int(lengths.max())
    sizes = sr.make_sizes(data.size, M, pos, ids, lengths, seed=9)
    calls, flush = sr.split(pos, ids, sizes, M)
    h = host_handle(w.pattern_file, perf=perf)
    saved = os.path.join(workdir, f"stream_c2_{perf}.pfac")
    h.saveCompiled(saved)
    h.destroy()
    g = api.PFAC.createHostOnly()
    try:
        g.setPlatform(platform)
        g.loadCompiled(saved)                            # (sets the perf mode the set was saved with)
        assert g.info().perfMode == perf
        feed(g, data, sizes, calls, flush, "loaded compiled set")
    finally:
        g.destroy()
