"""Streams (PFACX_stream*) on the GPU: PFACX_streamMatchFromDevice (the seam launch of scan_stream.hip + the compacted scan of the piece
in place) and PFACX_streamMatchFromHost on the GPU platform, call by call against tests/stream_ref.py -- the oracle's list over the
whole stream split by the finality rule.  Kernel variants and perf modes, the 32 MiB switch between the tiled and the filter kernel,
misaligned piece pointers, hostile and caseless sets, the 1 GiB C3 stream against the committed reference digest, a failed call that
leaves the stream where it was, canaries around every array."""

import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api, sharding  # noqa: E402
from pfac_amd import workloads as wl  # noqa: E402
from tests import nocase_ref as nc  # noqa: E402
from tests import stream_ref as sr  # noqa: E402
from tests.gpu_helpers import digest_record, make_handle  # noqa: E402
from tests.test_stream_host import SMALL, folded_model, hostile_case, seams_beyond, short_piece_sizes  # noqa: E402

PAD = 16            # canary entries in front of and behind the pair arrays


def feed_device(h, data, sizes, calls, flush, what, misalign=0):
    """one stream of h through the device calls, compared call by call; canaries around d_ids / d_pos[capacity] and the piece"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = int(data.size)
    M = int(h.info().maxPatternLen)
    d_s = torch.full((n + misalign + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
    d_s[misalign:misalign + n] = torch.from_numpy(data).to("cuda:0")
    image = d_s.clone()
    cap = max(sizes) + M
    d_ids = torch.full((cap + 2 * PAD,), -7, dtype=torch.int32, device="cuda:0")
    d_pos = torch.full((cap + 2 * PAD,), -7, dtype=torch.int32, device="cuda:0")
    s = h.streamOpen()

    def piece(off, size):
        _, k, poff = s.match_device(d_s.data_ptr() + misalign + off, size, d_ids.data_ptr() + 4 * PAD, d_pos.data_ptr() + 4 * PAD, cap)
        return d_ids[PAD:PAD + k].cpu().numpy(), d_pos[PAD:PAD + k].cpu().numpy(), poff

    def end():
        _, k = s.flush(d_ids.data_ptr() + 4 * PAD, d_pos.data_ptr() + 4 * PAD, cap)
        return d_ids[PAD:PAD + k].cpu().numpy(), d_pos[PAD:PAD + k].cpu().numpy()

    try:
        sr.run(piece, end, data, sizes, calls, flush, what)
    finally:
        s.close()
    torch.cuda.synchronize()
    for arr in (d_ids, d_pos):
        assert bool((arr[:PAD] == -7).all()) and bool((arr[PAD + cap:] == -7).all()), f"{what}: wrote outside the {cap} entries"
    assert bool((d_s == image).all()), f"{what}: the caller's pieces (or the bytes around them) were modified"


def feed_host(h, data, sizes, calls, flush, what):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    before = data.copy()
    s = h.streamOpen()
    try:
        sr.run(lambda off, size: s.match_host_array(data[off:off + size]), s.flush_host_array, data, sizes, calls, flush, what)
    finally:
        s.close()
    assert np.array_equal(data, before)


def model(w, seed, n=None):
    data = w.data if n is None else w.data[:n]
    pos, ids = sr.full_list(w.pattern_file, data)
    lengths = sr.pattern_lengths(w.pattern_file)
    M = int(lengths.max())
    sizes = sr.make_sizes(data.size, M, pos, ids, lengths, seed=seed)
    assert sr.straddling(pos, ids, lengths, sizes) >= min(20, int(np.count_nonzero(lengths[ids] >= 2)))
    calls, flush = sr.split(pos, ids, sizes, M)
    return data, sizes, calls, flush


@pytest.mark.parametrize("variant,vname", [(api.PFACX_KERNEL_FILTER, "filter"), (api.PFACX_KERNEL_NAIVE, "naive"), (api.PFACX_KERNEL_AUTO, "auto"),
                                           (api.PFACX_KERNEL_REFTABLE, "reftable")])
@pytest.mark.parametrize("perf,pname", [(api.PFAC_TIME_DRIVEN, "dense"), (api.PFAC_SPACE_DRIVEN, "hashed")])
def test_c3_stream_under_every_kernel_variant_and_perf_mode(workloads, variant, vname, perf, pname):
    data, sizes, calls, flush = model(workloads["c3"], seed=31)
    h = make_handle(workloads["c3"].pattern_file, perf, api.PFAC_AUTOMATIC, variant)
    try:
        feed_device(h, data, sizes, calls, flush, f"c3 device {vname}/{pname}")
        feed_host(h, data, sizes, calls, flush, f"c3 host-on-gpu {vname}/{pname}")
    finally:
        h.destroy()


@pytest.mark.parametrize("name", SMALL)
def test_small_workloads_device_and_host_on_the_gpu_platform(workloads, name):
    data, sizes, calls, flush = model(workloads[name], seed=1000 + SMALL.index(name))
    h = make_handle(workloads[name].pattern_file, api.PFAC_SPACE_DRIVEN, api.PFAC_AUTOMATIC, api.PFACX_KERNEL_AUTO)
    try:
        before = h.info().deviceTableBytes
        feed_device(h, data, sizes, calls, flush, f"{name} device")
        feed_host(h, data, sizes, calls, flush, f"{name} host-on-gpu")
        assert h.info().deviceTableBytes == before          # the closed streams gave their carry buffers back
    finally:
        h.destroy()


@pytest.mark.parametrize("which", ["snort-lengths", "long", "huge", "m1"])
def test_hostile_sets_in_pieces_far_shorter_than_the_longest_pattern(workdir, which):
    """the hostile sets of tests/test_stream_host.py, whole streams, through the device form AND the host form on the GPU platform,
    in their short pieces (snort-lengths: some 2 000 calls of 5..40 bytes with M = 243, nearly every carried position a 1-byte match)
    and again in pieces longer than M.  `huge` (M = 25 000): some calls stage more than the seam launch's 48 KiB of LDS, so the seam
    is staged in the stream's device scratch."""
    pf, data, sizes = hostile_case(workdir, which)
    pos, ids = sr.full_list(pf, data)
    M = int(sr.pattern_lengths(pf).max())
    if which == "huge":
        assert seams_beyond(sizes, M, 48 << 10) >= 2
    coarse = short_piece_sizes(data.size, M + 1, 3 * M + 50, 4)
    h = make_handle(pf, api.PFAC_TIME_DRIVEN, api.PFAC_AUTOMATIC, api.PFACX_KERNEL_AUTO)
    try:
        for cut, cname in ((sizes, "short pieces"), (coarse, "pieces longer than M")):
            calls, flush = sr.split(pos, ids, cut, M)
            feed_device(h, data, cut, calls, flush, f"{which} device, {cname}")
            feed_host(h, data, cut, calls, flush, f"{which} host-on-gpu, {cname}")
    finally:
        h.destroy()


def test_caseless_streams(workdir):
    for name, (pats, data) in nc.mixed_sets().items():
        pf, pos, ids = folded_model(workdir, "gpu_" + name, pats, data)
        lengths = sr.pattern_lengths(pf)
        M = int(lengths.max())
        sizes = sr.make_sizes(data.size, M, pos, ids, lengths, seed=55)
        assert sr.straddling(pos, ids, lengths, sizes) >= min(20, int(np.count_nonzero(lengths[ids] >= 2)))
        calls, flush = sr.split(pos, ids, sizes, M)
        h = api.PFAC.create()
        try:
            h.readPatternFromMemoryEx(nc.pattern_bytes(pats), api.PFACX_READ_NOCASE)
            feed_device(h, data, sizes, calls, flush, f"nocase {name} device")
            feed_device(h, data, sizes, calls, flush, f"nocase {name} device + 3", misalign=3)
            feed_host(h, data, sizes, calls, flush, f"nocase {name} host-on-gpu")
        finally:
            h.destroy()
    # a cut between an upper- and a lower-case byte of one occurrence
    pats = [b"HeLLo", b"hell", b"LOW"]
    data = np.frombuffer(b"..hEllO..HELlow", dtype=np.uint8).copy()
    pf, pos, ids = folded_model(workdir, "gpu_cut", pats, data)
    h = api.PFAC.create()
    try:
        h.readPatternFromMemoryEx(nc.pattern_bytes(pats), api.PFACX_READ_NOCASE)
        for cut in range(1, data.size):
            calls, flush = sr.split(pos, ids, [cut, data.size - cut], 5)
            feed_device(h, data, [cut, data.size - cut], calls, flush, f"nocase cut {cut}")
    finally:
        h.destroy()


@pytest.mark.parametrize("misalign", list(range(1, 16)))
def test_misaligned_piece_pointers(workloads, misalign):
    data, sizes, calls, flush = model(workloads["c2"], seed=200 + misalign, n=150000)
    h = make_handle(workloads["c2"].pattern_file, api.PFAC_TIME_DRIVEN, api.PFAC_AUTOMATIC, api.PFACX_KERNEL_FILTER)
    try:
        feed_device(h, data, sizes, calls, flush, f"c2 + {misalign}", misalign=misalign)
    finally:
        h.destroy()


@pytest.mark.parametrize("variant,vname", [(api.PFACX_KERNEL_AUTO, "auto"), (api.PFACX_KERNEL_FILTER, "filter")])
def test_a_40_mib_piece_between_small_ones_crosses_the_kernel_switch(workdir, variant, vname):
    """pieces below 32 MiB take the tiled kernel, the 40 MiB piece the filter kernel (with its read-ahead behind the last position it
    reports); odd sizes, so no cut is 16-byte aligned"""
    pats = wl.snort_patterns(3000)
    pf = wl.write_pattern_file(os.path.join(workdir, "stream_switch.pat"), pats)
    n = (41 << 20) + 12345
    data = wl.http_stream(n, wl.http_message_pool(pats, pool_size=512, embed_fraction=0.2))
    from oracle import binding as ob
    o = ob.Oracle(pf, hashed=False)
    try:
        full = o.match(data, omp=True)
    finally:
        o.close()
    pos = np.flatnonzero(full > 0).astype(np.int64)
    ids = full[pos].astype(np.int32)
    M = int(sr.pattern_lengths(pf).max())
    sizes = [70001, 17, (40 << 20) + 3, M - 1, 1]
    sizes.append(n - sum(sizes))
    calls, flush = sr.split(pos, ids, sizes, M)
    h = make_handle(pf, api.PFAC_SPACE_DRIVEN, api.PFAC_AUTOMATIC, variant)
    try:
        feed_device(h, data, sizes, calls, flush, f"switch {vname}", misalign=5)
    finally:
        h.destroy()


def test_the_c3_gib_stream_in_16_odd_pieces_has_the_reference_digest(workdir):
    """BASELINE's C3 stream (1 GiB) fed as 16 pieces of 64 MiB minus odd sizes: the pairs of all calls and the flush, scattered into a
    result vector, have the committed digest of the reference's own result (tests/golden/full_digests.json)"""
    n = 1 << 30
    rec = digest_record("c3", 0, 1024)
    want = rec["last"]
    cfg = wl.make_config("c3")
    pf = wl.write_pattern_file(f"{workdir}/stream_digest_c3.pat", cfg.patterns)
    assert wl.fnv1a(np.fromfile(pf, dtype=np.uint8)) == rec["pattern_file_fnv1a"], "pattern generator drifted"
    host = cfg.input_slice(n, 0)
    assert wl.fnv1a(host) == rec["input_fnv1a"], "input generator drifted"
    d_in = torch.from_numpy(host).to("cuda:0")
    sizes = [(64 << 20) - odd for odd in (3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53)]
    sizes.append(n - sum(sizes))
    assert all(sum(sizes[:k]) % 16 for k in range(1, 16))
    h = make_handle(pf, api.PFAC_SPACE_DRIVEN, api.PFAC_AUTOMATIC, api.PFACX_KERNEL_AUTO)
    d_out = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    try:
        M = int(h.info().maxPatternLen)
        cap = max(sizes) + M
        d_ids = torch.empty(cap, dtype=torch.int32, device="cuda:0")
        d_pos = torch.empty(cap, dtype=torch.int32, device="cuda:0")
        s = h.streamOpen()
        off = 0
        total = 0
        for size in sizes:
            _, k, poff = s.match_device(d_in.data_ptr() + off, size, d_ids.data_ptr(), d_pos.data_ptr(), cap)
            assert poff == off
            at = d_pos[:k].to(torch.int64) + off
            assert k == 0 or (int(at.min()) >= 0 and bool((at[1:] > at[:-1]).all()))
            d_out[at] = d_ids[:k]
            off += size
            total += k
        _, k = s.flush(d_ids.data_ptr(), d_pos.data_ptr(), cap)
        d_out[d_pos[:k].to(torch.int64) + n] = d_ids[:k]
        total += k
        s.close()
    finally:
        h.destroy()
    got = d_out.cpu().numpy()
    del d_in, d_out
    pos = np.flatnonzero(got)
    assert total == want["match_count"] and int(pos.size) == want["match_count"]
    assert sharding.position_checksum(pos, got[pos], base=0) == want["checksum"]
    assert wl.fnv1a_sparse_i32(pos, got[pos], n) == want["fnv1a64"]
    assert hashlib.sha256(got.view(np.uint8)).hexdigest() == want["sha256"]


def test_a_refused_call_leaves_the_stream_where_it_was_and_kinds_do_not_mix(workloads):
    w = workloads["c2"]
    data = w.data[:100000]
    pos, ids = sr.full_list(w.pattern_file, data)
    M = int(sr.pattern_lengths(w.pattern_file).max())
    sizes = [40000, 7, 59993]
    calls, flush = sr.split(pos, ids, sizes, M)
    h = make_handle(w.pattern_file, api.PFAC_TIME_DRIVEN, api.PFAC_AUTOMATIC, api.PFACX_KERNEL_AUTO)
    try:
        d_s = torch.from_numpy(data).to("cuda:0")
        cap = max(sizes) + M
        d_ids = torch.full((cap + PAD,), -7, dtype=torch.int32, device="cuda:0")
        d_pos = torch.full((cap + PAD,), -7, dtype=torch.int32, device="cuda:0")
        tables = h.info().deviceTableBytes
        s = h.streamOpen()
        off = 0
        for k, size in enumerate(sizes):
            st, _, _ = s.match_device(d_s.data_ptr() + off, size, d_ids.data_ptr(), d_pos.data_ptr(), size + M - 1, check=False)   # one short
            assert st == api.STATUS.INVALID_PARAMETER
            if k == 1:                                   # a host call on a device-fed stream
                piece = data[off:off + size].copy()
                hi = np.zeros(size + M, np.int32)
                st, _, _ = s.match_host(piece.ctypes.data, size, hi.ctypes.data, hi.ctypes.data, size + M, check=False)
                assert st == api.STATUS.INVALID_PARAMETER
                h.trim()                                 # the carried bytes are state, not scratch
                assert h.info().deviceTableBytes >= tables + 2 * (M - 1)
            _, got, poff = s.match_device(d_s.data_ptr() + off, size, d_ids.data_ptr(), d_pos.data_ptr(), size + M)
            assert poff == off and got == calls[k][0].size
            assert np.array_equal(d_ids[:got].cpu().numpy(), calls[k][0]) and np.array_equal(d_pos[:got].cpu().numpy(), calls[k][1])
            off += size
        st, _ = s.flush(d_ids.data_ptr(), d_pos.data_ptr(), M - 1, check=False)
        assert st == api.STATUS.INVALID_PARAMETER
        _, got = s.flush(d_ids.data_ptr(), d_pos.data_ptr(), M)
        assert np.array_equal(d_ids[:got].cpu().numpy(), flush[0]) and np.array_equal(d_pos[:got].cpu().numpy(), flush[1])
        assert bool((d_ids[cap:] == -7).all()) and bool((d_pos[cap:] == -7).all())
        # after the flush the stream is free again: now host-fed; then a device call is the wrong kind
        piece = data[:5000].copy()
        s.match_host_array(piece)
        st, _, _ = s.match_device(d_s.data_ptr(), 100, d_ids.data_ptr(), d_pos.data_ptr(), cap, check=False)
        assert st == api.STATUS.INVALID_PARAMETER
        # another pattern set: refused until reset
        h.readPatternFromFile(w.pattern_file)
        st, _, _ = s.match_device(d_s.data_ptr(), 100, d_ids.data_ptr(), d_pos.data_ptr(), cap, check=False)
        assert st == api.STATUS.INVALID_PARAMETER
        s.reset()
        _, got, poff = s.match_device(d_s.data_ptr(), sizes[0], d_ids.data_ptr(), d_pos.data_ptr(), cap)
        assert poff == 0 and np.array_equal(d_ids[:got].cpu().numpy(), calls[0][0])
    finally:
        h.destroy()                                      # closes the stream
