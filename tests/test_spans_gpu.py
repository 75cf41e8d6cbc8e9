"""PFACX_matchSpansFromDevice / PFACX_redactSpansFromDevice / PFACX_matchSpansFromHost (GPU platform) against the two references of
tests/spans_ref.py: every edge case of the host file, the seeded random cases, every kernel variant and mode, both sides of the 32 MiB switch,
the running maximum across blocks of pairs, pairs == size, 2 Mi spans, pair counts around the block of pairs, misaligned pointers, caseless
sets, the scratch accounting; the redaction: every misalignment of both pointers, sizes around the 16-byte step and the tile, spans on tile
boundaries, more spans in a tile than its staging holds, hostile span arrays, overlap, the round trip, the example program.  All arrays are
poisoned and carry GUARD words behind capacity."""

import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import spans_ref as ref  # noqa: E402
from tests.gpu_helpers import MODES, VARIANTS, make_handle, oracle_match  # noqa: E402
from tests.spans_helpers import GUARD, RANDOM_SEEDS, host_spans, pattern_file, random_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR_BLOCK = 512                # scan_spans.hip: kSpanBlock, the pairs one block of the pair-space passes takes
TILE = 4096                     # scan_spans.hip: kTile, the output bytes of one tile of the redaction
INVALID = api.STATUS.INVALID_PARAMETER


def as_array(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)


def device_spans(h, data, in_offset=0, keep=False):
    """matchSpansFromDevice over poisoned arrays of capacity == size (+ GUARD) -> ((start, len), covered bytes); the guard words behind capacity
    and the input must stay untouched.  keep: also return the device tensors (input, offset, start, len) for a redaction"""
    data = as_array(data)
    n = int(data.size)
    d_in = torch.zeros(n + in_offset + 64, dtype=torch.uint8, device="cuda:0")
    d_in[in_offset:in_offset + n] = torch.from_numpy(data.copy()).to("cuda:0")
    d_start, d_len = (torch.full((n + GUARD,), -5, dtype=torch.int32, device="cuda:0") for _ in range(2))
    st, ns, cb = h.matchSpansFromDevice(d_in.data_ptr() + in_offset, n, d_start.data_ptr(), d_len.data_ptr(), n)
    torch.cuda.synchronize()
    assert st == 0 and ns <= (n + 1) // 2
    assert bool((d_start[n:] == -5).all()) and bool((d_len[n:] == -5).all()), "wrote behind capacity"
    assert torch.equal(d_in[in_offset:in_offset + n].cpu(), torch.from_numpy(data.copy())), "the caller's input was modified"
    got = (d_start[:ns].cpu().numpy().copy(), d_len[:ns].cpu().numpy().copy())
    assert cb == int(got[1].astype(np.int64).sum()), "coveredBytes is the sum of the lengths"
    return ((got, cb), (d_in, in_offset, d_start, d_len)) if keep else (got, cb)


def device_redact(h, data, start, length, fill, in_offset=0, out_offset=0, in_place=False, num_spans=None):
    """redactSpansFromDevice with guard bytes on both sides of d_out -> (status, d_out[0, size) as bytes)"""
    data = as_array(data)
    n = int(data.size)
    start, length = np.ascontiguousarray(start, dtype=np.int32), np.ascontiguousarray(length, dtype=np.int32)
    count = int(start.size) if num_spans is None else num_spans
    d_start = torch.from_numpy(np.append(start, [-5] * 4).astype(np.int32)).to("cuda:0")
    d_len = torch.from_numpy(np.append(length, [-5] * 4).astype(np.int32)).to("cuda:0")
    host = torch.from_numpy(data.copy())
    if in_place:
        d_out = torch.full((GUARD + out_offset + n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
        at = GUARD + out_offset
        d_out[at:at + n] = host.to("cuda:0")
        I = O = d_out.data_ptr() + at
    else:
        d_in = torch.zeros(n + in_offset + 64, dtype=torch.uint8, device="cuda:0")
        d_in[in_offset:in_offset + n] = host.to("cuda:0")
        d_out = torch.full((GUARD + out_offset + n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
        at = GUARD + out_offset
        I, O = d_in.data_ptr() + in_offset, d_out.data_ptr() + at
    st = h.redactSpansFromDevice(I, n, d_start.data_ptr(), d_len.data_ptr(), count, fill, O, check=False)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(out[:at] == 0xEE) and np.all(out[at + n:] == 0xEE), "wrote outside d_out[0, size)"
    if not in_place:
        assert torch.equal(d_in[in_offset:in_offset + n].cpu(), host), "the input was modified"
    return st, out[at:at + n].tobytes()


def check_redact(h, data, start, length, what, fills=(0x2A,), **kw):
    data = as_array(data)
    for fill in fills:
        want = ref.redact_py(data.tobytes(), start, length, fill)
        for in_place in (False, True):
            st, got = device_redact(h, data, start, length, fill, in_place=in_place, **kw)
            assert st == 0, f"{what}: status {st}"
            if got != want:
                g, w = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
                bad = np.flatnonzero(g != w)
                raise AssertionError(f"{what}/fill {fill:#x}/in place {in_place}: {bad.size} bytes differ, first at {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}")


def gpu_handle(pf, flags=0, variant=api.PFACX_KERNEL_AUTO, perf=api.PFAC_TIME_DRIVEN, tex=api.PFAC_TEXTURE_OFF):
    h = api.PFAC.create()
    h.setPerfMode(perf)
    h.setTextureMode(tex)
    h.setKernelVariant(variant)
    h.readPatternFromFileEx(pf, flags)
    return h


@pytest.fixture(scope="module")
def plain(workdir):
    """a handle whose pattern set does not matter: the redaction needs none"""
    h = gpu_handle(pattern_file(workdir, "plain", [b"needle"]))
    yield h
    h.destroy()


# ---------------------------------------------------------------- the cases of the host file


@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_on_the_device_form_and_the_host_form(workdir, case):
    name, pats, data = case
    nocase = name.startswith("nocase")
    h = gpu_handle(pattern_file(workdir, name, pats), api.PFACX_READ_NOCASE if nocase else 0)
    try:
        want = ref.spans_py(pats, data, nocase)
        if not data:
            d = torch.full((GUARD,), -5, dtype=torch.int32, device="cuda:0")
            assert h.matchSpansFromDevice(d.data_ptr(), 0, d.data_ptr(), d.data_ptr(), 0) == (0, 0, 0)
            torch.cuda.synchronize()
            assert bool((d == -5).all()), "size == 0 touches nothing"
            assert h.redactSpansFromDevice(d.data_ptr(), 0, None, None, 0, 0, d.data_ptr()) == 0 and bool((d == -5).all())
        else:
            (got, covered), kept = device_spans(h, data, keep=True)
            ref.same(got, want, f"{name}/device")
            assert covered == int(want[1].sum())
            check_redact(h, data, got[0], got[1], name)
        got, covered, after = host_spans(h, data)                 # the GPU platform: the pipelined host path, merged on the host
        ref.same(got, want, f"{name}/host form")
        assert covered == int(want[1].sum()) and after == data
    finally:
        h.destroy()


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_cases_on_the_device_form(workdir, seed):
    pats, data = random_case(seed)
    pf = pattern_file(workdir, f"random{seed}", pats)
    want = ref.spans_from_result(oracle_match(pf, data), ref.pattern_lengths(pats))
    h = gpu_handle(pf)
    try:
        got, covered = device_spans(h, data)
        ref.same(got, want, f"seed {seed}")
        assert covered == int(want[1].sum())
        check_redact(h, data, got[0], got[1], f"seed {seed}")
    finally:
        h.destroy()


# ---------------------------------------------------------------- workloads: every variant and mode, both sides of the 32 MiB switch


@pytest.fixture(scope="module")
def text_200k(workloads):
    w = workloads["c3"]
    data = w.data[:200000].copy()
    want = ref.spans_from_result(oracle_match(w.pattern_file, data), ref.pattern_lengths_of_file(w.pattern_file))
    assert want[0].size > 100
    return w.pattern_file, data, want


@pytest.mark.parametrize("perf,tex,mode_name", MODES)
@pytest.mark.parametrize("variant,vname", VARIANTS)
def test_200_kb_every_variant_and_mode(text_200k, variant, vname, perf, tex, mode_name):
    pf, data, want = text_200k
    h = make_handle(pf, perf, tex, variant)
    try:
        got, covered = device_spans(h, data)
        ref.same(got, want, f"{vname}/{mode_name}")
        assert covered == int(want[1].sum())
    finally:
        h.destroy()


@pytest.mark.parametrize("mib", [31, 33])
def test_each_side_of_the_32_mib_switch(workloads, mib):
    w = workloads["c3"]
    data = np.tile(w.data, (mib << 20) // w.data.size + 1)[:mib << 20].copy()
    want = ref.spans_from_result(oracle_match(w.pattern_file, data, omp=True), ref.pattern_lengths_of_file(w.pattern_file))
    h = make_handle(w.pattern_file, api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        (got, covered), kept = device_spans(h, data, keep=True)
        ref.same(got, want, f"{mib} MiB")
        assert covered == int(want[1].astype(np.int64).sum())
        d_in, _, d_start, d_len = kept                             # ... and the redaction of the whole buffer, in place
        h.redactSpansFromDevice(d_in.data_ptr(), data.size, d_start.data_ptr(), d_len.data_ptr(), got[0].size, 0, d_in.data_ptr())
        torch.cuda.synchronize()
        mark = np.zeros(data.size + 1, dtype=np.int32)
        np.add.at(mark, want[0], 1)
        np.add.at(mark, want[0] + want[1], -1)
        expect = np.where(np.cumsum(mark[:-1]) > 0, 0, data).astype(np.uint8)
        assert np.array_equal(d_in[:data.size].cpu().numpy(), expect), f"{mib} MiB: redacted text differs"
    finally:
        h.destroy()


# ---------------------------------------------------------------- the running maximum, the pair-space passes


LONG = b"L" + b"x" * 1998 + b"R"                                # 2000 bytes; the 1998 one-byte matches inside it are more than three blocks of pairs


@pytest.mark.parametrize("lead", [0, PAIR_BLOCK - 1, PAIR_BLOCK, 3 * PAIR_BLOCK + 7, 8191 * PAIR_BLOCK - 100])
def test_running_maximum_across_blocks_of_pairs(workdir, lead):
    """`lead` one-byte spans in front make the long match pair number `lead`: the last pair of a block, the first of the next.  Every x inside the
    long match lies under an end that comes from up to four blocks back; the x behind the gap does not.  The last lead puts the long match into
    block 8190 and the pairs under it into blocks 8191 .. 8194: block 8192 is the first value of the second block of the block-value scan, so what
    it carries in comes from that scan's fold over the values in front of it alone, and the largest end lies two values back, not in the last"""
    assert 1998 > 3 * PAIR_BLOCK
    data = b"x." * lead + LONG + b".x"
    pf = pattern_file(workdir, "runmax", [LONG, b"x"])
    h = gpu_handle(pf)
    try:
        got, covered = device_spans(h, data)
        at = 2 * lead
        want = (np.append(np.arange(0, at, 2), [at, at + 2001]).astype(np.int32), np.append(np.ones(lead), [2000, 1]).astype(np.int32))
        ref.same(got, want, f"lead {lead}")
        assert got[0].size == lead + 2 and covered == lead + 2001
        if lead < 8192:
            ref.same(got, ref.spans_py([LONG, b"x"], data), f"lead {lead}/pure python")
        else:                                                      # minutes of pure Python: the host engine instead
            ho = api.PFAC.createHostOnly()
            try:
                ho.readPatternFromFile(pf)
                host, host_covered, _ = host_spans(ho, data)
            finally:
                ho.destroy()
            ref.same(got, host, f"lead {lead}/host engine")
            assert covered == host_covered
    finally:
        h.destroy()


def test_every_byte_covered_and_every_second_byte(workdir):
    n = 4 << 20
    h = gpu_handle(pattern_file(workdir, "justa", [b"a"]))
    try:
        got, covered = device_spans(h, np.full(n, ord("a"), dtype=np.uint8))            # pairs == size: one span
        assert (got[0].tolist(), got[1].tolist(), covered) == ([0], [n], n)
        for text, first in ((b"ab", 0), (b"ba", 1)):
            data = np.tile(np.frombuffer(text, dtype=np.uint8), n // 2)
            (got, covered), kept = device_spans(h, data, keep=True)
            assert got[0].size == n // 2 == covered, "2 Mi spans of one byte"
            assert np.array_equal(got[0], np.arange(first, n, 2, dtype=np.int32)) and np.all(got[1] == 1)
            d_in, _, d_start, d_len = kept                         # the redaction: more spans in every tile than its staging holds
            d_out = torch.full((n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
            h.redactSpansFromDevice(d_in.data_ptr(), n, d_start.data_ptr(), d_len.data_ptr(), n // 2, ord("#"), d_out.data_ptr())
            torch.cuda.synchronize()
            want = np.tile(np.frombuffer(text.replace(b"a", b"#"), dtype=np.uint8), n // 2)
            assert np.array_equal(d_out[:n].cpu().numpy(), want) and bool((d_out[n:] == 0xEE).all())
    finally:
        h.destroy()


@pytest.mark.parametrize("pairs", [0, 1, PAIR_BLOCK - 1, PAIR_BLOCK, PAIR_BLOCK + 1, 8192 * PAIR_BLOCK + 1])
def test_pair_counts_around_the_block_of_pairs(workdir, pairs):
    """(the last count: one pair more than one block of the block-value scan takes)"""
    h = gpu_handle(pattern_file(workdir, "justx", [b"x"]))
    try:
        data = np.tile(np.frombuffer(b".x", dtype=np.uint8), max(pairs, 4))
        data[2 * pairs:] = ord(".")
        got, covered = device_spans(h, data)
        assert got[0].size == pairs == covered
        assert np.array_equal(got[0], np.arange(1, 2 * pairs, 2, dtype=np.int32)) and np.all(got[1] == 1)
    finally:
        h.destroy()


@pytest.mark.parametrize("offset", [1, 5, 15])
def test_input_pointers_off_alignment(workdir, offset):
    pats = [b"NEEDLE", b"QQ", b"Z", b"EDLEQ"]
    rng = np.random.Generator(np.random.PCG64(offset))
    h = gpu_handle(pattern_file(workdir, "align", pats))
    try:
        for n in (5000, 70000):
            data = rng.integers(97, 123, size=n, dtype=np.uint8)
            for _ in range(n // 100):
                p = pats[int(rng.integers(0, len(pats)))]
                at = int(rng.integers(0, n - len(p) + 1))
                data[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
            got, _ = device_spans(h, data, in_offset=offset)
            ref.same(got, ref.spans_py(pats, data.tobytes()), f"offset {offset}/{n} bytes")
    finally:
        h.destroy()


def test_caseless_handle_keeps_the_case_outside_the_spans(workdir):
    name, pats, data = next(c for c in ref.CASES if c[0] == "nocase-mixed")
    for d, variant in ((data, api.PFACX_KERNEL_AUTO), (data * 4000, api.PFACX_KERNEL_FILTER)):
        h = gpu_handle(pattern_file(workdir, name, pats), api.PFACX_READ_NOCASE, variant)
        try:
            want = ref.spans_py(pats, d, nocase=True)
            assert want[0].size != ref.spans_py(pats, d)[0].size, "the case is meant to matter here"
            for off in (0, 5):
                got, _ = device_spans(h, d, in_offset=off)
                ref.same(got, want, f"{name}/{len(d)} bytes/offset {off}")
            check_redact(h, d, got[0], got[1], f"{name}/{len(d)} bytes")           # redact_py works on the original bytes
            _, text = device_redact(h, d, got[0], got[1], ord("*"))
            assert b"GeT" not in text and b"a *" in text and b"HTTP" in text
        finally:
            h.destroy()


def test_scratch_accounting_and_trim(workdir):
    pats = [b"NEEDLE", b"Z"]
    rng = np.random.Generator(np.random.PCG64(4))
    data = rng.integers(97, 123, size=300000, dtype=np.uint8)
    data[rng.random(data.size) < 0.01] = ord("Z")
    want = ref.spans_py(pats, data.tobytes())
    h = gpu_handle(pattern_file(workdir, "scratch", pats))
    try:
        d_in = torch.from_numpy(data.copy()).to("cuda:0")
        d_ids, d_pos = (torch.full((data.size,), -5, dtype=torch.int32, device="cuda:0") for _ in range(2))
        h.matchFromDeviceReduce(d_in.data_ptr(), data.size, d_ids.data_ptr(), d_pos.data_ptr())        # the scan's own scratch is there already
        torch.cuda.synchronize()
        before = h.info().deviceScratchBytes
        ref.same(device_spans(h, data)[0], want, "first call")
        grown = h.info().deviceScratchBytes
        assert grown > before, "the spans scratch is counted under deviceScratchBytes"
        ref.same(device_spans(h, data)[0], want, "second call")
        assert h.info().deviceScratchBytes == grown, "a second call of the same shape allocates nothing"
        h.trim()
        assert h.info().deviceScratchBytes < before, "trim gives the scratch back"
        trimmed = h.info().deviceScratchBytes
        ref.same(device_spans(h, data)[0], want, "after trim")
        assert h.info().deviceScratchBytes > trimmed, "the call works again after the trim, on scratch of its own"
    finally:
        h.destroy()


def test_error_rows_on_a_device_handle(workdir):
    h = gpu_handle(pattern_file(workdir, "errors", [b"ab"]))
    try:
        d_in = torch.from_numpy(np.frombuffer(b"ab.ab.", dtype=np.uint8).copy()).to("cuda:0")
        d = [torch.full((6 + GUARD,), -5, dtype=torch.int32, device="cuda:0") for _ in range(2)]
        I, (S, L) = d_in.data_ptr(), (t.data_ptr() for t in d)
        call = lambda *a: h.matchSpansFromDevice(*a, check=False)[0]  # noqa: E731
        assert call(I, 6, S, L, 5) == INVALID and call(I, 1 << 31, S, L, 1 << 31) == INVALID
        assert call(None, 6, S, L, 6) == INVALID and call(I, 6, None, L, 6) == INVALID and call(I, 6, S, None, 6) == INVALID
        torch.cuda.synchronize()
        assert all(bool((t == -5).all()) for t in d), "a refused call wrote"
        assert h.matchSpansFromDevice(I, 6, S, L, 6) == (0, 2, 4), "the handle is usable after refused calls"
    finally:
        h.destroy()
    bare = api.PFAC.create()
    try:
        assert bare.matchSpansFromDevice(I, 6, S, L, 6, check=False)[0] == api.STATUS.PATTERNS_NOT_READY
    finally:
        bare.destroy()


# ---------------------------------------------------------------- the redaction alone


def _spans_for(rng, n, density=0.02):
    """an ascending, disjoint, never adjacent list over [0, n)"""
    start, length, at = [], [], int(rng.integers(0, 3))
    while at < n:
        l = int(min(n - at, rng.integers(1, 40)))
        start.append(at)
        length.append(l)
        at += l + 1 + int(rng.geometric(density))
    return np.array(start, dtype=np.int32), np.array(length, dtype=np.int32)


def test_redact_every_misalignment_of_both_pointers(plain):
    rng = np.random.Generator(np.random.PCG64(16))
    n = 5000
    data = rng.integers(97, 123, size=n, dtype=np.uint8)
    start, length = _spans_for(rng, n)
    start[0], length[-1] = 0, n - start[-1]                     # the first and the last byte are covered
    want = ref.redact_py(data.tobytes(), start, length, 0x2A)
    for out_off in range(16):
        for in_off in range(16):
            st, got = device_redact(plain, data, start, length, 0x2A, in_offset=in_off, out_offset=out_off)
            assert st == 0 and got == want, f"input + {in_off}, output + {out_off}"
        st, got = device_redact(plain, data, start, length, 0x2A, out_offset=out_off, in_place=True)
        assert st == 0 and got == want, f"in place + {out_off}"


@pytest.mark.parametrize("n", [1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 3 * TILE + 7])
def test_redact_sizes_around_the_steps(plain, n):
    rng = np.random.Generator(np.random.PCG64(n))
    data = rng.integers(97, 123, size=n, dtype=np.uint8)
    for k, (start, length) in enumerate((_spans_for(rng, n, 0.2), ([0], [n]), ([n - 1], [1]), ([0], [1]))):
        for off in (0, 3):
            check_redact(plain, data, start, length, f"{n} bytes/list {k}/offset {off}", fills=(0x00, 0xFF), in_offset=off, out_offset=(off * 5) % 16)


def test_redact_spans_on_tile_boundaries_and_over_five_tiles(plain):
    rng = np.random.Generator(np.random.PCG64(7))
    n = 8 * TILE + 100
    data = rng.integers(97, 123, size=n, dtype=np.uint8)
    lists = {
        "ends on a boundary": ([TILE - 10, 2 * TILE + 5], [10, TILE - 5]),
        "starts on a boundary": ([TILE, 3 * TILE], [7, 1]),
        "boundary to boundary": ([TILE, 4 * TILE], [TILE, 2 * TILE]),
        "one byte on each side of a boundary": ([TILE - 1, TILE + 1], [1, 1]),
        "one span over five tiles": ([TILE // 2], [5 * TILE]),
        "one span over everything": ([0], [n]),
    }
    for what, (start, length) in lists.items():
        for off in (0, 9):                                     # the tiles are cut on the output ADDRESS: both with and without an offset
            check_redact(plain, data, start, length, f"{what}/offset {off}", fills=(0x00, 0xFF), out_offset=off, in_offset=(off + 3) % 16)


def test_redact_more_spans_in_a_tile_than_its_staging_holds(plain):
    n = 3 * TILE + 77
    data = np.tile(np.frombuffer(b"ab", dtype=np.uint8), n // 2 + 1)[:n]
    for first in (0, 1):
        start = np.arange(first, n, 2, dtype=np.int32)
        for off in (0, 1, 6):
            check_redact(plain, data, start, np.ones(start.size, dtype=np.int32), f"every second byte from {first}/offset {off}", out_offset=off, in_offset=off // 2)


def test_redact_without_spans_is_a_copy(plain):
    rng = np.random.Generator(np.random.PCG64(8))
    data = rng.integers(0, 256, size=3 * TILE + 5, dtype=np.uint8)
    empty = np.zeros(0, dtype=np.int32)
    for off in (0, 7):
        st, got = device_redact(plain, data, empty, empty, 0x2A, in_offset=off, out_offset=(off * 3) % 16)
        assert st == 0 and got == data.tobytes()
    st, got = device_redact(plain, data, empty, empty, 0x2A, in_place=True)
    assert st == 0 and got == data.tobytes(), "in place leaves the buffer alone"
    d = torch.from_numpy(data.copy()).to("cuda:0")
    d_out = torch.full((data.size,), 0xEE, dtype=torch.uint8, device="cuda:0")
    assert plain.redactSpansFromDevice(d.data_ptr(), data.size, None, None, 0, 0x2A, d_out.data_ptr()) == 0, "no spans: the arrays may be null"
    torch.cuda.synchronize()
    assert torch.equal(d_out, d)
    assert plain.redactSpansFromDevice(d.data_ptr(), data.size, None, None, 1, 0x2A, d_out.data_ptr(), check=False) == INVALID


def test_redact_hostile_span_arrays_stay_inside_the_buffers(plain):
    """the arrays are the caller's contract: unspecified text is allowed, an access outside the buffers is not"""
    rng = np.random.Generator(np.random.PCG64(9))
    n = 2 * TILE + 50
    data = rng.integers(97, 123, size=n, dtype=np.uint8)
    big = (1 << 31) - 1
    lists = {
        "start = -7": ([-7, 100], [10, 5]),
        "len = 2^31 - 1": ([50, 200], [big, big]),
        "start > size": ([n + 1, big, 10], [5, 5, -3]),
        "descending": (list(range(n - 10, 0, -37)), [20] * len(range(n - 10, 0, -37))),
        "all the same": ([5] * 3000, [big] * 3000),
    }
    for what, (start, length) in lists.items():
        for in_place in (False, True):
            for off in (0, 11):
                st, got = device_redact(plain, data, start, length, 0x2A, out_offset=off, in_offset=off // 2, in_place=in_place)
                assert st == 0, what                            # (device_redact has checked the guard bytes on both sides)
                g = np.frombuffer(got, dtype=np.uint8)
                assert np.all((g == 0x2A) | (g == data)), f"{what}: a byte that is neither the input's nor the fill"


def test_redact_refuses_partial_overlap(plain):
    n = 1000
    buf = torch.full((3 * n,), 0x61, dtype=torch.uint8, device="cuda:0")
    s = torch.tensor([0], dtype=torch.int32, device="cuda:0")
    l = torch.tensor([n], dtype=torch.int32, device="cuda:0")
    base = buf.data_ptr() + n
    for delta in (1, -1, n - 1, 1 - n, 16, -16):
        assert plain.redactSpansFromDevice(base, n, s.data_ptr(), l.data_ptr(), 1, 0x2A, base + delta, check=False) == INVALID, f"d_out = d_input + {delta}"
    torch.cuda.synchronize()
    assert bool((buf == 0x61).all()), "a refused call wrote"
    for delta in (n, -n):                                       # ranges that touch do not overlap
        assert plain.redactSpansFromDevice(base, n, s.data_ptr(), l.data_ptr(), 1, 0x2A, base + delta) == 0
    torch.cuda.synchronize()
    assert bool((buf[n:2 * n] == 0x61).all()) and bool((buf[:n] == 0x2A).all()) and bool((buf[2 * n:] == 0x2A).all())


def test_round_trip_leaves_no_match(workloads):
    w = workloads["c3"]
    data = w.data[:1 << 20].copy()
    fill = 0x0A                                                 # the pattern format ends a pattern at '\n': it occurs in none
    h = make_handle(w.pattern_file, api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        ((start, length), covered), kept = device_spans(h, data, keep=True)
        assert start.size > 100
        d_in, _, d_start, d_len = kept
        d_out = torch.full((data.size,), 0xEE, dtype=torch.uint8, device="cuda:0")
        h.redactSpansFromDevice(d_in.data_ptr(), data.size, d_start.data_ptr(), d_len.data_ptr(), start.size, fill, d_out.data_ptr())
        torch.cuda.synchronize()
        red = d_out.cpu().numpy()
        assert int(np.count_nonzero(red == fill)) == covered + int(np.count_nonzero(data == fill))
        got, covered2 = device_spans(h, red)
        assert got[0].size == 0 and covered2 == 0, "the redacted buffer holds no match"
    finally:
        h.destroy()


def test_example_program_passes_its_self_check(workdir):
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "redact_example"], check=True, stdout=subprocess.PIPE)
    p = subprocess.run([os.path.join(ROOT, "examples", "redact_example")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    assert b"self-check passed" in p.stdout
