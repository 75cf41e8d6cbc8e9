"""PFACX_matchLinesFromDevice / PFACX_gatherLinesFromDevice / PFACX_matchLinesFromHost (GPU platform) against references that use none of
the library's line code (tests/lines_ref.py): every edge case of the host file on the device form, every kernel variant, walker, perf and
texture mode, both sides of the 32 MiB switch, misaligned pointers, sizes around the 16-byte and 2 KiB steps of the newline pass, an
all-newline input, one 3 MiB line, line starts on block boundaries, the shared ordering state, trim and the scratch accounting, caseless
sets; the gather: text, truncation, guard bytes, the example program.  All arrays are poisoned and carry GUARD words behind capacity."""

import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import lines_ref as ref  # noqa: E402
from tests.gpu_helpers import MODES, VARIANTS, make_handle, oracle_match  # noqa: E402
from tests.lines_helpers import host_lines, pattern_file  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
TRUNCATED = api.STATUS.OUTPUT_TRUNCATED


def as_array(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)


def device_lines(h, data, invert, in_offset=0, with_index=True, keep=False):
    """matchLinesFromDevice over poisoned arrays of capacity == size (+ GUARD) -> (numLines, start, len, index); the guard words behind
    capacity and the input must stay untouched.  keep: also return the device tensors (input, start, len) for a gather"""
    data = as_array(data)
    n = int(data.size)
    cap = n
    d_in = torch.zeros(n + in_offset + 64, dtype=torch.uint8, device="cuda:0")
    d_in[in_offset:in_offset + n] = torch.from_numpy(data.copy()).to("cuda:0")
    d_start, d_len, d_index = (torch.full((cap + GUARD,), -5, dtype=torch.int32, device="cuda:0") for _ in range(3))
    st, nl, ns = h.matchLinesFromDevice(d_in.data_ptr() + in_offset, n, api.PFACX_LINES_INVERT if invert else 0, d_start.data_ptr(),
                                        d_len.data_ptr(), d_index.data_ptr() if with_index else None, cap)
    torch.cuda.synchronize()
    assert st == 0 and ns <= nl <= n
    start, length, index = d_start.cpu().numpy(), d_len.cpu().numpy(), d_index.cpu().numpy()
    assert np.all(start[cap:] == -5) and np.all(length[cap:] == -5) and np.all(index[cap:] == -5), "wrote behind capacity"
    assert np.array_equal(d_in[in_offset:in_offset + n].cpu().numpy(), data), "the caller's input was modified"
    if not with_index:
        assert np.all(index == -5)
    got = (nl, start[:ns].copy(), length[:ns].copy(), index[:ns].copy())
    return (got, (d_in, in_offset, d_start, d_len)) if keep else got


def device_gather(h, kept, n, num_selected, out_capacity=None, out_offset=0):
    """gatherLinesFromDevice into a poisoned buffer of out_capacity (+ GUARD) bytes -> (status, outBytes, the bytes below capacity)"""
    d_in, in_offset, d_start, d_len = kept
    cap = n + 1 if out_capacity is None else int(out_capacity)
    d_out = torch.full((cap + out_offset + GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
    st, total = h.gatherLinesFromDevice(d_in.data_ptr() + in_offset, n, d_start.data_ptr(), d_len.data_ptr(), num_selected,
                                        d_out.data_ptr() + out_offset, cap, check=False)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(out[:out_offset] == 0xEE) and np.all(out[out_offset + cap:] == 0xEE), "wrote outside [0, outCapacity)"
    return st, total, out[out_offset:out_offset + cap].tobytes()


def gpu_handle(pf, flags=0, variant=api.PFACX_KERNEL_AUTO, perf=api.PFAC_TIME_DRIVEN, tex=api.PFAC_TEXTURE_OFF):
    h = api.PFAC.create()
    h.setPerfMode(perf)
    h.setTextureMode(tex)
    h.setKernelVariant(variant)
    h.readPatternFromFileEx(pf, flags)
    return h


def check_both_flags_and_text(h, pats, data, what, nocase=False, want=None, **kw):
    """the device form with and without INVERT against the reference, and the gathered text of each list"""
    data = as_array(data)
    for invert in (False, True):
        w = want[invert] if want is not None else ref.lines_py(pats, data.tobytes(), invert, nocase)
        got, kept = device_lines(h, data, invert, keep=True, **kw)
        ref.same(got, w, f"{what}/invert {invert}")
        st, total, text = device_gather(h, kept, data.size, got[1].size)
        expect = ref.gather_py(data.tobytes(), w[1], w[2])
        assert (st, total) == (0, len(expect)), f"{what}/invert {invert}: gather status {st}, {total} bytes, want {len(expect)}"
        assert text[:total] == expect, f"{what}/invert {invert}: gathered text differs"


# ---------------------------------------------------------------- the cases of the host file, on the device form


@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_small_cases_on_the_device_form(workdir, case):
    name, pats, data = case
    h = gpu_handle(pattern_file(workdir, name, pats))
    try:
        if not data:
            d = torch.full((GUARD,), -5, dtype=torch.int32, device="cuda:0")
            st, nl, ns = h.matchLinesFromDevice(d.data_ptr(), 0, 0, d.data_ptr(), d.data_ptr(), None, 0)
            assert (st, nl, ns) == (0, 0, 0) and bool((d == -5).all()), "size == 0 touches nothing"
            return
        check_both_flags_and_text(h, pats, data, name)
        got = device_lines(h, data, True, with_index=False)
        w = ref.lines_py(pats, data, True)
        assert got[0] == w[0] and np.array_equal(got[1], w[1]) and np.array_equal(got[2], w[2]), f"{name}: lineIndex NULL"
    finally:
        h.destroy()


@pytest.mark.parametrize("case", ref.CASES + ref.NOCASE_CASES, ids=[c[0] for c in ref.CASES + ref.NOCASE_CASES])
def test_host_form_on_the_gpu_platform(workdir, case):
    name, pats, data = case
    nocase = name.startswith("nocase")
    h = gpu_handle(pattern_file(workdir, name, pats), api.PFACX_READ_NOCASE if nocase else 0)
    try:
        for invert in (False, True):
            got, after = host_lines(h, data, invert)
            ref.same(got, ref.lines_py(pats, data, invert, nocase), f"{name}/invert {invert}")
            assert after == data
    finally:
        h.destroy()


def test_caseless_handle(workdir):
    name, pats, data = ref.NOCASE_CASES[0]
    big = data * 3000                                        # 200 KB: the filter kernel's side too
    for d, variant in ((data, api.PFACX_KERNEL_AUTO), (big, api.PFACX_KERNEL_FILTER)):
        h = gpu_handle(pattern_file(workdir, name, pats), api.PFACX_READ_NOCASE, variant)
        try:
            check_both_flags_and_text(h, pats, d, f"{name}/{len(d)} bytes", nocase=True)
            check_both_flags_and_text(h, pats, d, f"{name}/{len(d)} bytes/misaligned", nocase=True, in_offset=5)
        finally:
            h.destroy()


def test_error_rows_on_a_device_handle(workdir):
    pf = pattern_file(workdir, "errors", ref.PATS)
    h = gpu_handle(pf)
    try:
        d_in = torch.from_numpy(np.frombuffer(b"ab\ncd\n", dtype=np.uint8).copy()).to("cuda:0")
        d = [torch.full((6 + GUARD,), -5, dtype=torch.int32, device="cuda:0") for _ in range(3)]
        I, (S, L, X) = d_in.data_ptr(), (t.data_ptr() for t in d)
        call = lambda *a: h.matchLinesFromDevice(*a, check=False)[0]  # noqa: E731
        INVALID = api.STATUS.INVALID_PARAMETER
        assert call(I, 6, 0, S, L, X, 5) == INVALID and call(I, 1 << 31, 0, S, L, X, 1 << 31) == INVALID and call(I, 6, 4, S, L, X, 6) == INVALID
        assert call(None, 6, 0, S, L, X, 6) == INVALID and call(I, 6, 0, None, L, X, 6) == INVALID and call(I, 6, 0, S, None, X, 6) == INVALID
        torch.cuda.synchronize()
        assert all(bool((t == -5).all()) for t in d), "a refused call wrote"
        assert call(I, 6, 0, S, L, X, 6) == 0, "the handle is usable after refused calls"
    finally:
        h.destroy()
    bare = api.PFAC.create()
    try:
        assert bare.matchLinesFromDevice(I, 6, 0, S, L, X, 6, check=False)[0] == api.STATUS.PATTERNS_NOT_READY
    finally:
        bare.destroy()


# ---------------------------------------------------------------- workloads: every variant, mode and walker


@pytest.fixture(scope="module")
def mib_workloads(workloads):
    """1 MiB of C3 and of C5 with the expected lists for both flag values, from the oracle's longest-match vector (computed once)"""
    out = {}
    for name in ("c3", "c5"):
        w = workloads[name]
        data = w.data[:1 << 20].copy()
        if int(np.count_nonzero(data == 10)) < 1000:          # a stream without line ends: cut it into lines of 30 .. 150 bytes
            rng = np.random.Generator(np.random.PCG64(11))
            data[np.cumsum(rng.integers(30, 150, size=data.size // 90))[:-1] % data.size] = 10
        result = oracle_match(w.pattern_file, data)
        out[name] = (w.pattern_file, data, {inv: ref.lines_from_result(result, data, inv) for inv in (False, True)})
    return out


@pytest.mark.parametrize("perf,tex,mode_name", MODES)
@pytest.mark.parametrize("variant,vname", VARIANTS)
@pytest.mark.parametrize("name", ["c3", "c5"])
def test_one_mib_every_variant_and_mode(mib_workloads, name, variant, vname, perf, tex, mode_name):
    pf, data, want = mib_workloads[name]
    h = make_handle(pf, perf, tex, variant)
    try:
        for invert in (False, True):
            ref.same(device_lines(h, data, invert), want[invert], f"{name}/{vname}/{mode_name}/invert {invert}")
    finally:
        h.destroy()


@pytest.mark.parametrize("walker", [api.PFACX_WALKER_AUTO, api.PFACX_WALKER_WINDOW, api.PFACX_WALKER_STAGE, api.PFACX_WALKER_VETO])
def test_one_mib_every_walker(mib_workloads, walker):
    for name in ("c3", "c5"):
        pf, data, want = mib_workloads[name]
        h = make_handle(pf, api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
        try:
            h.setWalker(walker)
            for invert in (False, True):
                ref.same(device_lines(h, data, invert), want[invert], f"{name}/walker {walker}/invert {invert}")
        finally:
            h.destroy()


def test_48_mib_on_the_filter_kernel_side_of_the_switch(workloads):
    w = workloads["c3"]
    data = np.tile(w.data, (48 << 20) // w.data.size + 1)[:48 << 20].copy()
    result = oracle_match(w.pattern_file, data, omp=True)
    h = make_handle(w.pattern_file, api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        for invert in (False, True):
            want = ref.lines_from_result(result, data, invert)
            got, kept = device_lines(h, data, invert, keep=True)
            ref.same(got, want, f"48 MiB/invert {invert}")
            if not invert:
                st, total, text = device_gather(h, kept, data.size, got[1].size)
                assert (st, total) == (0, int(want[2].sum()) + want[2].size)
                assert text[:total] == ref.gather_py(data.tobytes(), want[1], want[2])
    finally:
        h.destroy()


# ---------------------------------------------------------------- alignment, sizes, block boundaries


def _text(rng, n, pats, newline_every=40):
    """n bytes of lower-case noise with line ends and a sprinkling of the patterns"""
    data = rng.integers(97, 123, size=n, dtype=np.uint8)
    data[rng.random(n) < 1.0 / newline_every] = 10
    for _ in range(max(1, n // 200)):
        p = pats[int(rng.integers(0, len(pats)))]
        if len(p) <= n:
            at = int(rng.integers(0, n - len(p) + 1))
            data[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
    return data


@pytest.mark.parametrize("offset", [1, 7, 15])
def test_input_pointers_off_alignment(workdir, offset):
    pats = [b"NEEDLE", b"QQ", b"Z"]
    rng = np.random.Generator(np.random.PCG64(offset))
    h = gpu_handle(pattern_file(workdir, "align", pats))
    try:
        for n in (5000, 2048 - offset, 2049 - offset, 70000):
            check_both_flags_and_text(h, pats, _text(rng, n, pats), f"offset {offset}/{n} bytes", in_offset=offset)
    finally:
        h.destroy()


@pytest.mark.parametrize("n", [1, 15, 16, 17, 2047, 2048, 2049])
def test_sizes_around_the_steps_of_the_newline_pass(workdir, n):
    pats = [b"NEEDLE", b"QQ", b"Z"]
    rng = np.random.Generator(np.random.PCG64(n))
    h = gpu_handle(pattern_file(workdir, "sizes", pats))
    try:
        for tail in (b"Z", b"\n", b"a"):                     # a match, a newline and neither in the last byte
            data = _text(rng, n, pats, newline_every=12)
            data[-1] = tail[0]
            check_both_flags_and_text(h, pats, data, f"{n} bytes/last byte {tail!r}")
    finally:
        h.destroy()


def test_one_mib_of_newlines(workdir):
    """numLines == size: the largest line index, every line empty"""
    pats = [b"a"]
    n = 1 << 20
    data = np.full(n, 10, dtype=np.uint8)
    h = gpu_handle(pattern_file(workdir, "allnl", pats))
    try:
        z, every = np.zeros(0, dtype=np.int32), np.arange(n, dtype=np.int32)
        ref.same(device_lines(h, data, False), (n, z, z, z), "all newlines")
        got, kept = device_lines(h, data, True, keep=True)
        ref.same(got, (n, every, np.zeros(n, dtype=np.int32), every), "all newlines/invert")
        st, total, text = device_gather(h, kept, n, n)           # only empty lines under INVERT
        assert (st, total) == (0, n) and text[:n] == b"\n" * n
    finally:
        h.destroy()


def test_one_3_mib_line_whose_only_match_starts_at_its_last_byte(workdir):
    pats = [b"Z", b"needle"]
    n = 3 << 20
    rng = np.random.Generator(np.random.PCG64(3))
    line = rng.integers(97, 123, size=n, dtype=np.uint8)
    line[-1] = ord("Z")
    data = np.concatenate([np.frombuffer(b"short\n", dtype=np.uint8), line, np.frombuffer(b"\nlast\n", dtype=np.uint8)])
    h = gpu_handle(pattern_file(workdir, "long", pats))
    try:
        got, kept = device_lines(h, data, False, keep=True)
        ref.same(got, (3, np.array([6], dtype=np.int32), np.array([n], dtype=np.int32), np.array([1], dtype=np.int32)), "3 MiB line")
        st, total, text = device_gather(h, kept, data.size, 1, out_offset=3)
        assert (st, total) == (0, n + 1) and text[:total] == line.tobytes() + b"\n"
        ref.same(device_lines(h, data, True), ref.lines_py(pats, data.tobytes(), True), "3 MiB line/invert")
    finally:
        h.destroy()


def test_line_starts_on_block_boundaries(workdir):
    """lines that start exactly at multiples of 64, 2048 and 65536 (the newline in the last bit of a bitmap word, of a block, ...)"""
    pats = [b"NEEDLE", b"Z"]
    n = 3 * 65536 + 100
    rng = np.random.Generator(np.random.PCG64(5))
    data = rng.integers(97, 123, size=n, dtype=np.uint8)
    for m in (64, 128, 2048, 4096, 65536, 131072, 196608):
        data[m - 1] = 10                                     # a line starts at m ...
        data[m] = ord("Z") if (m // 64) % 2 else ord("a")    # ... some with a match in their first byte
    data[2047 - 6:2047] = np.frombuffer(b"NEEDLE", dtype=np.uint8)   # a match that ends in front of a block's last byte
    h = gpu_handle(pattern_file(workdir, "bounds", pats))
    try:
        check_both_flags_and_text(h, pats, data, "block boundaries")
        check_both_flags_and_text(h, pats, data, "block boundaries/misaligned", in_offset=1)
    finally:
        h.destroy()


def test_a_million_lines(workdir):
    pats = [b"NEEDLE", b"QQ"]
    rng = np.random.Generator(np.random.PCG64(9))
    data = _text(rng, 20 << 20, pats, newline_every=20)
    want = {inv: ref.lines_from_result(ref.brute_result(pats, data.tobytes()), data, inv) for inv in (False, True)}
    assert want[False][0] > 1000000
    h = gpu_handle(pattern_file(workdir, "million", pats))
    try:
        check_both_flags_and_text(h, pats, data, "a million lines", want=want)
    finally:
        h.destroy()


def long_line_behind_a_block_of_the_block_scan():
    """(patterns, input): 16 MiB + 16 KiB of short lines with one line that runs from block 8189 into block 8194 of the newline bitmap.  Blocks
    8190 .. 8193 hold no newline, so the start of the line that ends in block 8194 -- the third value of the second block of the block-value scan
    -- is the running maximum that this scan folds over the values in front of its block, and the largest lies at entry 8189, not in the last"""
    pats = [b"NEEDLE"]
    n = (16 << 20) + (16 << 10)
    rng = np.random.Generator(np.random.PCG64(8194))
    data = rng.integers(97, 123, size=n, dtype=np.uint8)
    data[rng.random(n) < 1.0 / 60] = 10
    lo, hi = 8190 * 2048, 8194 * 2048 + 100
    data[lo - 700:hi + 1][data[lo - 700:hi + 1] == 10] = ord("a")
    data[lo - 700] = 10                                      # the long line: [lo - 699, hi + 50)
    data[hi + 50] = 10
    for at in (1000, 5 << 20, lo + 4000, n - 3000):          # once inside the long line, and in a few short ones
        data[at:at + 6] = np.frombuffer(b"NEEDLE", dtype=np.uint8)
    ends = np.flatnonzero(data == 10)
    k = int(np.searchsorted(ends, lo))
    assert ends[k - 1] // 2048 == 8189 and ends[k] // 2048 == 8194 and ends[k] > hi
    return pats, data


def test_a_line_that_starts_in_front_of_a_block_of_the_block_scan(workdir):
    pats, data = long_line_behind_a_block_of_the_block_scan()
    pf = pattern_file(workdir, "scanblock", pats)
    ho = api.PFAC.createHostOnly()
    try:
        ho.readPatternFromFile(pf)
        want = {inv: host_lines(ho, data, inv)[0] for inv in (False, True)}
    finally:
        ho.destroy()
    result = ref.brute_result(pats, data.tobytes())
    for inv in (False, True):
        ref.same(want[inv], ref.lines_from_result(result, data, inv), f"host engine/invert {inv}")
    assert 8 * 1024 < want[False][2].max() < 9 * 1024 and want[False][1].size == 4
    h = gpu_handle(pf)
    try:
        for inv in (False, True):
            ref.same(device_lines(h, data, inv), want[inv], f"long line/invert {inv}")
    finally:
        h.destroy()


# ---------------------------------------------------------------- shared state, trim, scratch accounting


def test_other_calls_between_lines_calls_and_trim(workdir):
    pats = [b"NEEDLE", b"QQ", b"Z", b"NEE"]
    pf = pattern_file(workdir, "mixed", pats)
    rng = np.random.Generator(np.random.PCG64(21))
    big, small = _text(rng, 300000, pats), _text(rng, 7000, pats)
    h = gpu_handle(pf)
    try:
        before = h.info().deviceScratchBytes
        check_both_flags_and_text(h, pats, big, "first call")
        grown = h.info().deviceScratchBytes
        assert grown > before, "the lines scratch is counted under deviceScratchBytes"
        check_both_flags_and_text(h, pats, small, "a smaller call on the same handle")
        # the ordered compacted call and the all-match call in between: the ordering state they share with the scan survives
        want = oracle_match(pf, big)
        pos = np.flatnonzero(want).astype(np.int32)
        d_in = torch.from_numpy(big.copy()).to("cuda:0")
        d_ids, d_pos = (torch.full((big.size,), -5, dtype=torch.int32, device="cuda:0") for _ in range(2))
        for round_ in range(2):
            _, cnt = h.matchFromDeviceReduce(d_in.data_ptr(), big.size, d_ids.data_ptr(), d_pos.data_ptr())
            torch.cuda.synchronize()
            assert cnt == pos.size and np.array_equal(d_pos.cpu().numpy()[:cnt], pos) and np.array_equal(d_ids.cpu().numpy()[:cnt], want[pos])
            check_both_flags_and_text(h, pats, big, f"behind the compacted call {round_}")
        cap = big.size * h.info().maxMatchesPerPosition
        a_ids, a_pos = (torch.full((cap,), -5, dtype=torch.int32, device="cuda:0") for _ in range(2))
        st, total = h.matchAllFromDevice(d_in.data_ptr(), big.size, a_ids.data_ptr(), a_pos.data_ptr(), cap)
        torch.cuda.synchronize()
        got_pos = a_pos.cpu().numpy()[:total]
        assert st == 0 and np.array_equal(np.unique(got_pos), pos) and total > pos.size, "NEE is a prefix of NEEDLE: more pairs than positions"
        check_both_flags_and_text(h, pats, big, "behind the all-match call")
        h.trim()
        assert h.info().deviceScratchBytes == before, "trim gives the lines scratch back"
        check_both_flags_and_text(h, pats, big, "after trim")
        h.trim()
        check_both_flags_and_text(h, pats, small, "after trim again")
    finally:
        h.destroy()


# ---------------------------------------------------------------- the gather alone


def test_gather_capacity_exact_and_one_byte_short(workdir):
    name, pats, data = next(c for c in ref.CASES if c[0] == "no-trailing-newline")
    data = data * 500
    h = gpu_handle(pattern_file(workdir, name, pats))
    try:
        for invert in (False, True):
            want = ref.lines_py(pats, data, invert)
            expect = ref.gather_py(data, want[1], want[2])
            got, kept = device_lines(h, data, invert, keep=True)
            for off in (0, 5):
                st, total, text = device_gather(h, kept, len(data), got[1].size, out_capacity=len(expect), out_offset=off)
                assert (st, total) == (0, len(expect)) and text == expect, "outCapacity exact"
                st, total, _ = device_gather(h, kept, len(data), got[1].size, out_capacity=len(expect) - 1, out_offset=off)
                assert (st, total) == (TRUNCATED, len(expect)), "one byte short: truncated, the full size reported"
            st, total, _ = device_gather(h, kept, len(data), got[1].size, out_capacity=1)
            assert (st, total) == (TRUNCATED, len(expect))
        # zero selected: success, nothing written, d_out may be null
        st, total, text = device_gather(h, kept, len(data), 0, out_capacity=16)
        assert (st, total) == (0, 0) and text == b"\xEE" * 16
        assert h.gatherLinesFromDevice(kept[0].data_ptr(), len(data), kept[2].data_ptr(), kept[3].data_ptr(), 0, None, 0) == (0, 0)
    finally:
        h.destroy()


def test_gather_clamps_bad_line_arrays(workdir):
    """the arrays are the caller's contract: wrong text is allowed, an access outside the buffers is not"""
    h = gpu_handle(pattern_file(workdir, "clamp", ref.PATS))
    try:
        data = np.frombuffer(b"0123456789", dtype=np.uint8)
        d_in = torch.from_numpy(data.copy()).to("cuda:0")
        d_start = torch.tensor([-4, 8, 1 << 30, 3, 10], dtype=torch.int32, device="cuda:0")
        d_len = torch.tensor([3, 100, 5, -2, 1], dtype=torch.int32, device="cuda:0")
        st, total, text = device_gather(h, (d_in, 0, d_start, d_len), 10, 5, out_capacity=64)
        assert (st, total) == (0, 3 + 1 + 2 + 1 + 0 + 1 + 0 + 1 + 0 + 1) and text[:total] == b"012\n89\n\n\n\n"
    finally:
        h.destroy()


def test_gather_every_misalignment_of_the_output_and_sizes_around_the_tile(workdir):
    """every (address of d_out) & 15 against texts of 1 byte, around the 16 bytes of a thread and around the 4096 of a tile, outCapacity == the
    text: the first and the last thread of a text store bytes, not 16 at once, and nothing lands in front of d_out or behind the text"""
    front, tile = 64, 4096
    rng = np.random.default_rng(20261018)
    data = rng.integers(32, 127, size=2 * tile + 64, dtype=np.uint8)
    d_in = torch.from_numpy(data.copy()).to("cuda:0")
    h = gpu_handle(pattern_file(workdir, "gather-misaligned", ref.PATS))
    try:
        for total in (1, 15, 16, 17, tile - 1, tile, tile + 1, 2 * tile + 5):
            # a few short lines (one of them empty) around one line sized to hit the total; a line of len bytes is len + 1 bytes of text
            short = [(40, 3), (9, 0), (21, 7)][:max(0, min(3, (total - 1) // 8))]
            used = sum(ln + 1 for _, ln in short)
            lines = short[:1] + [(5, total - used - 1)] + short[1:]
            start = np.array([s for s, _ in lines], dtype=np.int32)
            length = np.array([ln for _, ln in lines], dtype=np.int32)
            expect = ref.gather_py(data.tobytes(), start, length)
            assert len(expect) == total
            d_start, d_len = torch.from_numpy(start).to("cuda:0"), torch.from_numpy(length).to("cuda:0")
            for off in range(16):
                d_out = torch.full((front + off + total + GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
                assert d_out.data_ptr() % 16 == 0
                st, got = h.gatherLinesFromDevice(d_in.data_ptr(), data.size, d_start.data_ptr(), d_len.data_ptr(), len(lines),
                                                  d_out.data_ptr() + front + off, total, check=False)
                torch.cuda.synchronize()
                out = d_out.cpu().numpy()
                what = f"{total} bytes at offset {off}"
                assert (st, got) == (0, total), f"{what}: status {st}, {got} bytes"
                assert np.all(out[:front + off] == 0xEE), f"{what}: wrote in front of d_out"
                assert np.all(out[front + off + total:] == 0xEE), f"{what}: wrote behind the text"
                assert out[front + off:front + off + total].tobytes() == expect, f"{what}: gathered text differs"
    finally:
        h.destroy()


def test_example_program_equals_grep(workdir):
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "lines_example"], check=True, stdout=subprocess.PIPE)
    name, pats, data = ref.NOCASE_CASES[0]
    pf = pattern_file(workdir, "example", pats)
    text = os.path.join(workdir, "lines_example.txt")
    with open(text, "wb") as f:
        f.write(data + b"last line without a newline: needle")
    data = open(text, "rb").read()
    for flags, invert, nocase in (([], False, False), (["-v"], True, False), (["-i"], False, True), (["-v", "-i"], True, True)):
        p = subprocess.run([os.path.join(ROOT, "examples", "lines_example"), *flags, pf, text], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, p.stderr.decode()
        want = ref.lines_py(pats, data, invert, nocase)
        assert p.stdout == ref.gather_py(data, want[1], want[2]), f"lines_example {' '.join(flags)}"
