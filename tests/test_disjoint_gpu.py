"""PFACX_matchDisjointFromDevice / PFACX_replaceFromDevice / PFACX_matchDisjointFromHost (GPU platform) against the references of
tests/disjoint_ref.py.  The selection: every edge case of the host file, the seeded random cases, every kernel variant and mode, both sides of the
32 MiB switch, pair counts around the block of pairs and over several doubling rounds, the two chains of ab / ba that never merge, hops that skip
whole blocks, misaligned pointers, a caseless set, the scratch accounting.  The replacement: tables that delete, shrink, keep, grow and hold a
replacement longer than two tiles, every misalignment of the three byte pointers, sizes around the 16-byte step and the tile, replacements on tile
boundaries, more tokens in a tile than its staging holds, truncation, the 2^32 size query, hostile arrays, overlap, the round trip.  All arrays are
poisoned and carry GUARD words behind capacity."""

import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import disjoint_ref as ref  # noqa: E402
from tests.disjoint_ref import GUARD, KINDS, RANDOM_SEEDS, host_disjoint, repl_table, replacements_for  # noqa: E402
from tests.gpu_helpers import MODES, VARIANTS, make_handle, oracle_match  # noqa: E402
from tests.spans_helpers import pattern_file, random_case  # noqa: E402
from tests.spans_ref import pattern_lengths, pattern_lengths_of_file  # noqa: E402

BLOCK = api.PFACX_DISJOINT_BLOCK
TILE = api.PFACX_REPLACE_TILE
INVALID, TRUNCATED = api.STATUS.INVALID_PARAMETER, api.STATUS.OUTPUT_TRUNCATED


def as_array(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0")


def device_disjoint(h, data, in_offset=0):
    """matchDisjointFromDevice over poisoned arrays of capacity == size (+ GUARD) -> ((ids, pos), covered bytes); the guard words behind capacity and
    the input must stay untouched"""
    data = as_array(data)
    n = int(data.size)
    d_in = torch.zeros(n + in_offset + 64, dtype=torch.uint8, device="cuda:0")
    d_in[in_offset:in_offset + n] = dev(data)
    d_ids, d_pos = (torch.full((n + GUARD,), -5, dtype=torch.int32, device="cuda:0") for _ in range(2))
    st, nt, cb = h.matchDisjointFromDevice(d_in.data_ptr() + in_offset, n, d_ids.data_ptr(), d_pos.data_ptr(), n)
    torch.cuda.synchronize()
    assert st == 0 and nt <= n
    assert bool((d_ids[n:] == -5).all()) and bool((d_pos[n:] == -5).all()), "wrote behind capacity"
    assert torch.equal(d_in[in_offset:in_offset + n].cpu(), torch.from_numpy(data.copy())), "the caller's input was modified"
    return (d_ids[:nt].cpu().numpy().copy(), d_pos[:nt].cpu().numpy().copy()), cb


def device_replace(h, data, ids, pos, repls=None, table=None, capacity=None, in_offset=0, out_offset=0, repl_offset=0, num_tokens=None):
    """replaceFromDevice with guard bytes on both sides of d_out -> (status, outBytes, the first min(outBytes, capacity) bytes); capacity None: the
    size the size query reports"""
    data = as_array(data)
    n = int(data.size)
    off, blob = table if table is not None else repl_table(repls)
    ids, pos = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(pos, dtype=np.int32)
    count = int(ids.size) if num_tokens is None else num_tokens
    d_ids, d_pos, d_off = dev(np.append(ids, [-5] * 4).astype(np.int32)), dev(np.append(pos, [-5] * 4).astype(np.int32)), dev(off)
    d_in = torch.zeros(n + in_offset + 64, dtype=torch.uint8, device="cuda:0")
    d_in[in_offset:in_offset + n] = dev(data)
    d_repl = torch.zeros(blob.size + repl_offset + 16, dtype=torch.uint8, device="cuda:0")
    if blob.size:
        d_repl[repl_offset:repl_offset + blob.size] = dev(blob)
    args = (d_in.data_ptr() + in_offset, n, d_ids.data_ptr(), d_pos.data_ptr(), count, d_off.data_ptr(), int(off.size), d_repl.data_ptr() + repl_offset,
            int(blob.size))
    if capacity is None:
        st, capacity = h.replaceFromDevice(*args, None, 0, check=False)
        assert st == (TRUNCATED if capacity else 0), "the size query"
    d_out = torch.full((GUARD + out_offset + capacity + GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
    at = GUARD + out_offset
    st, total = h.replaceFromDevice(*args, d_out.data_ptr() + at, capacity, check=False)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(out[:at] == 0xEE) and np.all(out[at + capacity:] == 0xEE), "wrote outside d_out[0, outCapacity)"
    assert torch.equal(d_in[in_offset:in_offset + n].cpu(), torch.from_numpy(data.copy())), "the input was modified"
    return st, total, out[at:at + min(total, capacity)].tobytes()


def check_replace(h, data, tokens, lengths, repls, what, **kw):
    want = ref.replace_py(as_array(data).tobytes(), tokens[0], tokens[1], lengths, repls)
    st, total, got = device_replace(h, data, tokens[0], tokens[1], repls, **kw)
    assert st == 0 and total == len(want), f"{what}: status {st}, {total} bytes, want {len(want)}"
    if got != want:
        g, w = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
        bad = np.flatnonzero(g != w)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}")


def gpu_handle(pf, flags=0, variant=api.PFACX_KERNEL_AUTO, perf=api.PFAC_TIME_DRIVEN, tex=api.PFAC_TEXTURE_OFF):
    h = api.PFAC.create()
    h.setPerfMode(perf)
    h.setTextureMode(tex)
    h.setKernelVariant(variant)
    h.readPatternFromFileEx(pf, flags)
    return h


def check_select(h, pats, data, what, want=None, nocase=False, **kw):
    """the device form against Python's re (or `want`), numTokens and coveredBytes included -> the tokens"""
    want = ref.disjoint_py(pats, as_array(data).tobytes(), nocase) if want is None else want
    got, covered = device_disjoint(h, data, **kw)
    ref.same(got, want, what)
    assert covered == ref.covered_of(want, pattern_lengths(pats)), f"{what}: coveredBytes"
    return got


# ---------------------------------------------------------------- the cases of the host file


@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_on_the_device_form_and_the_host_form(workdir, case):
    name, pats, data = case
    nocase = name.startswith("nocase")
    h = gpu_handle(pattern_file(workdir, "dj_" + name, pats), api.PFACX_READ_NOCASE if nocase else 0)
    try:
        want = ref.disjoint_py(pats, data, nocase)
        if not data:
            d = torch.full((GUARD,), -5, dtype=torch.int32, device="cuda:0")
            assert h.matchDisjointFromDevice(d.data_ptr(), 0, d.data_ptr(), d.data_ptr(), 0) == (0, 0, 0)
            assert h.replaceFromDevice(d.data_ptr(), 0, None, None, 0, None, 0, None, 0, None, 0) == (0, 0)
            torch.cuda.synchronize()
            assert bool((d == -5).all()), "size == 0 touches nothing"
        else:
            got = check_select(h, pats, data, f"{name}/device", want, nocase)
            for kind in KINDS:
                check_replace(h, data, got, pattern_lengths(pats), replacements_for(pats, kind), f"{name}/{kind}")
        got, covered, after = host_disjoint(h, data)              # the GPU platform: the pipelined host path, the loop on the host
        ref.same(got, want, f"{name}/host form")
        assert covered == ref.covered_of(want, pattern_lengths(pats)) and after == data
    finally:
        h.destroy()


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_cases_on_the_device_form_and_the_host_form(workdir, seed):
    pats, data = random_case(seed)
    pf = pattern_file(workdir, f"dj_random{seed}", pats)
    lengths = pattern_lengths(pats)
    want = ref.disjoint_from_result(oracle_match(pf, data), lengths)
    h = gpu_handle(pf)
    try:
        got = check_select(h, pats, data, f"seed {seed}", want)
        check_replace(h, data, got, lengths, replacements_for(pats, "mixed"), f"seed {seed}/mixed")
        got, covered, _ = host_disjoint(h, data.tobytes())
        ref.same(got, want, f"seed {seed}/host form")
        assert covered == ref.covered_of(want, lengths)
    finally:
        h.destroy()


# ---------------------------------------------------------------- workloads: every variant and mode, both sides of the 32 MiB switch


@pytest.fixture(scope="module")
def text_200k(workloads):
    w = workloads["c3"]
    data = w.data[:200000].copy()
    lengths = pattern_lengths_of_file(w.pattern_file)
    want = ref.disjoint_from_result(oracle_match(w.pattern_file, data), lengths)
    assert want[0].size > 100
    return w.pattern_file, data, want, ref.covered_of(want, lengths)


@pytest.mark.parametrize("perf,tex,mode_name", MODES)
@pytest.mark.parametrize("variant,vname", VARIANTS)
def test_200_kb_every_variant_and_mode(text_200k, variant, vname, perf, tex, mode_name):
    pf, data, want, want_covered = text_200k
    h = make_handle(pf, perf, tex, variant)
    try:
        got, covered = device_disjoint(h, data)
        ref.same(got, want, f"{vname}/{mode_name}")
        assert covered == want_covered
    finally:
        h.destroy()


SPARSE = [b"needle", b"needles", b"lesson", b"on"]


@pytest.mark.parametrize("mib", [31, 33])
def test_each_side_of_the_32_mib_switch(workdir, mib):
    """sparse: a match every 64 KiB or so, so that the reference stays cheap"""
    n = mib << 20
    rng = np.random.Generator(np.random.PCG64(mib))
    data = np.full(n, ord("."), dtype=np.uint8)
    piece = np.frombuffer(b"a needlesson, one needle; lessons", dtype=np.uint8)
    for at in np.sort(rng.integers(0, n - piece.size, size=n >> 16)):
        data[at:at + piece.size] = piece
    data[n - 6:] = np.frombuffer(b"needle", dtype=np.uint8)
    h = gpu_handle(pattern_file(workdir, "dj_sparse", SPARSE))
    try:
        got = check_select(h, SPARSE, data, f"{mib} MiB")
        assert got[0].size > 1000 and got[1][-1] == n - 6
        hot, covered, _ = host_disjoint(h, data)                  # pieces of 32 MiB on the GPU platform
        ref.same(hot, got, f"{mib} MiB/host form")
    finally:
        h.destroy()


# ---------------------------------------------------------------- the pair-space passes


@pytest.mark.parametrize("pairs", [1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1, 3 * 8192 + 5])
def test_pair_counts_around_the_block_and_over_several_rounds(workdir, pairs):
    """block edges, several doubling rounds, a number of blocks that is no power of two; every pair a token (a over a...), and every pair a token
    with a gap in front (ab over ab...: the hop of two positions is one pair)"""
    h = gpu_handle(pattern_file(workdir, "dj_a_ab", [b"a", b"ab"]))
    try:
        got, covered = device_disjoint(h, np.full(pairs, ord("a"), dtype=np.uint8))
        assert covered == pairs and np.array_equal(got[1], np.arange(pairs, dtype=np.int32)) and np.all(got[0] == 1)
        got, covered = device_disjoint(h, np.tile(np.frombuffer(b"ab", dtype=np.uint8), pairs))
        assert covered == 2 * pairs and np.array_equal(got[1], np.arange(0, 2 * pairs, 2, dtype=np.int32)) and np.all(got[0] == 2)
    finally:
        h.destroy()


@pytest.mark.parametrize("lead", [b"", b"x"])
@pytest.mark.parametrize("k", [300, 5000])
def test_two_chains_that_never_merge(workdir, k, lead):
    """ab / ba over (ab)^k: every position starts a match, the chain from pair 0 and the chain from pair 1 never meet.  An abc every 700 bytes
    flips the parity of the taken chain, inside blocks and across them"""
    pats = [b"ab", b"ba", b"abc"]
    body = bytearray(b"ab" * k)
    for at in range(100, len(body) - 3, 700):
        body[at:at + 3] = b"abc"
    data = lead + bytes(body)
    h = gpu_handle(pattern_file(workdir, "dj_abba", pats))
    try:
        got = check_select(h, pats, data, f"k {k}/lead {lead!r}")
        assert {1, 2, 3} <= set(got[0].tolist()), "both parities and the flip take part"
        check_replace(h, data, got, pattern_lengths(pats), [b"", b"AB", b"", b"<abc>"], f"k {k}/lead {lead!r}/replace")
    finally:
        h.destroy()


def test_hops_that_skip_whole_blocks(workdir):
    """a^2000 over a run of 5000 a: two hops of 2000 pairs each skip three blocks, then come 1000 one-byte tokens"""
    pats = [b"a", b"a" * 2000]
    data = b"some text" + b"a" * 5000 + b"and more a text"
    h = gpu_handle(pattern_file(workdir, "dj_hops", pats))
    try:
        got = check_select(h, pats, data, "hops")
        assert got[0].tolist()[:4] == [2, 2, 1, 1] and got[0].size == 2 + 1000 + 2
        check_replace(h, data, got, pattern_lengths(pats), [b"", b"", b"<2000>"], "hops/replace")
    finally:
        h.destroy()


def test_last_match_ends_exactly_at_size(workdir):
    pats = [b"needle", b"dle", b"e"]
    h = gpu_handle(pattern_file(workdir, "dj_last", pats))
    try:
        for data in (b"..ab" * 300 + b"needle", b"needle", b"e", b"x" * 1000 + b"nee"):
            got = check_select(h, pats, data, f"{len(data)} bytes")
            assert got[1][-1] + pattern_lengths(pats)[got[0][-1]] == len(data)
    finally:
        h.destroy()


@pytest.mark.parametrize("offset", [1, 3, 15])
def test_input_pointers_off_alignment(workdir, offset):
    pats = [b"NEEDLE", b"QQ", b"Z", b"EDLEQ", b"LEQQ"]
    rng = np.random.Generator(np.random.PCG64(offset))
    h = gpu_handle(pattern_file(workdir, "dj_align", pats))
    try:
        for n in (5000, 70000):
            data = rng.integers(97, 123, size=n, dtype=np.uint8)
            for _ in range(n // 50):
                p = pats[int(rng.integers(0, len(pats)))]
                at = int(rng.integers(0, n - len(p) + 1))
                data[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
            check_select(h, pats, data, f"offset {offset}/{n} bytes", in_offset=offset)
    finally:
        h.destroy()


def test_caseless_handle_replaces_in_the_callers_bytes(workdir):
    name, pats, data = next(c for c in ref.CASES if c[0] == "nocase-mixed")
    for d, variant in ((data, api.PFACX_KERNEL_AUTO), (data * 4000, api.PFACX_KERNEL_FILTER)):
        h = gpu_handle(pattern_file(workdir, "dj_" + name, pats), api.PFACX_READ_NOCASE, variant)
        try:
            want = ref.disjoint_py(pats, d, nocase=True)
            assert want[0].size != ref.disjoint_py(pats, d)[0].size, "the case is meant to matter here"
            for off in (0, 5):
                got = check_select(h, pats, d, f"{name}/{len(d)} bytes/offset {off}", want, in_offset=off)
            check_replace(h, d, got, pattern_lengths(pats), [b"", b"<n>", b"", b"GET /", b"le"], f"{name}/{len(d)} bytes")   # replace_py: the original bytes
            _, _, text = device_replace(h, d, got[0], got[1], [b"", b"<n>", b"", b"GET /", b"le"])
            assert b"HTTP" in text and b"a <n> in GET / HTTP" in text and b"NEEDLE" not in text
        finally:
            h.destroy()


def scratch_formula(pairs):
    """include/pfac_ext.h: the scratch of a select call with P pairs"""
    r = lambda b: (b + 255) & ~255  # noqa: E731
    blocks = (pairs + BLOCK - 1) // BLOCK
    return 2 * r(4 * pairs) + r(pairs) + r(4 * blocks) + r(4 * (blocks + 1)) + 256


def test_scratch_formula_and_trim(workdir):
    pats = [b"NEEDLE", b"Z", b"ZZ"]
    rng = np.random.Generator(np.random.PCG64(4))
    data = rng.integers(97, 123, size=300000, dtype=np.uint8)
    data[rng.random(data.size) < 0.01] = ord("Z")
    want = ref.disjoint_py(pats, data.tobytes())
    h = gpu_handle(pattern_file(workdir, "dj_scratch", pats))
    try:
        d_in = dev(data)
        d_a, d_b = (torch.full((data.size,), -5, dtype=torch.int32, device="cuda:0") for _ in range(2))
        h.matchSpansFromDevice(d_in.data_ptr(), data.size, d_a.data_ptr(), d_b.data_ptr(), data.size)      # the scan's scratch and the pattern lengths are there
        _, pairs = h.matchFromDeviceReduce(d_in.data_ptr(), data.size, d_a.data_ptr(), d_b.data_ptr())
        torch.cuda.synchronize()
        before = h.info().deviceScratchBytes
        ref.same(device_disjoint(h, data)[0], want, "first call")
        grown = h.info().deviceScratchBytes
        assert pairs > 2 * BLOCK and grown - before == scratch_formula(pairs), "the disjoint scratch follows the formula and is counted"
        ref.same(device_disjoint(h, data)[0], want, "second call")
        check_replace(h, data, want, pattern_lengths(pats), [b"", b"n", b"zz", b""], "replace")          # 8 bytes per token: fits the same allocation
        assert h.info().deviceScratchBytes == grown, "calls of the same shape allocate nothing"
        h.trim()
        assert h.info().deviceScratchBytes < before, "trim gives the scratch back"
        trimmed = h.info().deviceScratchBytes
        ref.same(device_disjoint(h, data)[0], want, "after trim")
        assert h.info().deviceScratchBytes > trimmed, "the call works again after the trim, on scratch of its own"
        none = np.full(5000, ord("q"), dtype=np.uint8)             # no pairs: no launch and no scratch
        h.trim()
        d_q = dev(none)
        h.matchSpansFromDevice(d_q.data_ptr(), none.size, d_a.data_ptr(), d_b.data_ptr(), none.size)      # (the scan's own scratch)
        trimmed = h.info().deviceScratchBytes
        assert device_disjoint(h, none)[0][0].size == 0 and h.info().deviceScratchBytes == trimmed
    finally:
        h.destroy()


def test_error_rows_on_a_device_handle(workdir):
    h = gpu_handle(pattern_file(workdir, "dj_errors", [b"ab"]))
    try:
        d_in = dev(np.frombuffer(b"ab.ab.", dtype=np.uint8))
        d = [torch.full((6 + GUARD,), -5, dtype=torch.int32, device="cuda:0") for _ in range(2)]
        I, (S, L) = d_in.data_ptr(), (t.data_ptr() for t in d)
        call = lambda *a: h.matchDisjointFromDevice(*a, check=False)[0]  # noqa: E731
        assert call(I, 6, S, L, 5) == INVALID and call(I, 1 << 31, S, L, 1 << 31) == INVALID
        assert call(None, 6, S, L, 6) == INVALID and call(I, 6, None, L, 6) == INVALID and call(I, 6, S, None, 6) == INVALID
        torch.cuda.synchronize()
        assert all(bool((t == -5).all()) for t in d), "a refused call wrote"
        assert h.matchDisjointFromDevice(I, 6, S, L, 6) == (0, 2, 4), "the handle is usable after refused calls"
        off, blob = repl_table([b"", b"xyz"])
        d_off, d_blob = dev(off), dev(blob)
        d_out = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda:0")
        rep = lambda *a: h.replaceFromDevice(*a, check=False)[0]  # noqa: E731
        assert rep(I, 6, S, L, 2, d_off.data_ptr(), 2, d_blob.data_ptr(), 3, d_out.data_ptr(), 64) == INVALID, "numOff < F + 2"
        assert rep(I, 6, S, L, 1 << 31, d_off.data_ptr(), 3, d_blob.data_ptr(), 3, d_out.data_ptr(), 64) == INVALID, "numTokens >= 2^31"
        assert rep(I, 6, S, L, 2, d_off.data_ptr(), 3, d_blob.data_ptr(), 1 << 31, d_out.data_ptr(), 64) == INVALID, "replBytes >= 2^31"
        assert rep(I, 6, None, L, 2, d_off.data_ptr(), 3, d_blob.data_ptr(), 3, d_out.data_ptr(), 64) == INVALID
        assert rep(I, 6, S, L, 2, d_off.data_ptr(), 3, d_blob.data_ptr(), 3, None, 64) == INVALID
        torch.cuda.synchronize()
        assert bool((d_out == 0xEE).all()), "a refused call wrote"
        assert h.replaceFromDevice(I, 6, S, L, 2, d_off.data_ptr(), 3, d_blob.data_ptr(), 3, d_out.data_ptr(), 64) == (0, 8)
        torch.cuda.synchronize()
        assert d_out[:8].cpu().numpy().tobytes() == b"xyz.xyz." and bool((d_out[8:] == 0xEE).all())
    finally:
        h.destroy()
    bare = api.PFAC.create()
    try:
        assert bare.matchDisjointFromDevice(I, 6, S, L, 6, check=False)[0] == api.STATUS.PATTERNS_NOT_READY
        assert bare.replaceFromDevice(I, 6, S, L, 2, None, 0, None, 0, None, 0, check=False)[0] == api.STATUS.PATTERNS_NOT_READY
    finally:
        bare.destroy()


# ---------------------------------------------------------------- the replacement alone


WORDS = [b"needle", b"ab", b"x", b"QQQQ"]
LONG = bytes(range(33, 123)) * 100                              # 9000 bytes: longer than two tiles


@pytest.fixture(scope="module")
def words(workdir):
    h = gpu_handle(pattern_file(workdir, "dj_words", WORDS))
    yield h
    h.destroy()


def text_of(rng, n, density=0.03):
    """n bytes of lower-case letters other than a, b, x with WORDS dropped in"""
    data = rng.choice(np.frombuffer(b"cdefghijklmnopqrstuvwyz ", dtype=np.uint8), size=n)
    at = int(rng.integers(0, 4))
    while at < n:
        p = WORDS[int(rng.integers(0, len(WORDS)))]
        if at + len(p) <= n:
            data[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
        at += len(p) + int(rng.geometric(density)) - 1
    return data


TABLES = {"delete": [b"", b"", b"", b"", b""], "shrink": [b"", b"ndl", b"a", b"", b"Q"], "same": [b"", b"NEEDLE", b"AB", b"X", b"qqqq"],
          "grow": [b"", b"<a needle was here>", b"abab", b"xx", b"Q" * 40], "long": [b"", b"[n]", b"", LONG, b"qq"]}


@pytest.mark.parametrize("kind", list(TABLES))
def test_replace_tables_that_delete_shrink_keep_grow_and_hold_a_long_one(words, kind):
    rng = np.random.Generator(np.random.PCG64(len(kind)))
    for n in (5000, 40000):
        data = text_of(rng, n)
        tokens = ref.disjoint_py(WORDS, data.tobytes())
        assert tokens[0].size > 50 and {1, 2, 3, 4} == set(tokens[0].tolist())
        check_replace(words, data, tokens, pattern_lengths(WORDS), TABLES[kind], f"{kind}/{n} bytes", in_offset=n % 7, out_offset=n % 5, repl_offset=3)


def test_replace_every_misalignment_of_the_three_pointers(words):
    rng = np.random.Generator(np.random.PCG64(16))
    data = text_of(rng, 5120)
    tokens = ref.disjoint_py(WORDS, data.tobytes())
    lengths = pattern_lengths(WORDS)
    for out_off in range(16):
        for in_off in range(16):
            check_replace(words, data, tokens, lengths, TABLES["grow"], f"input + {in_off}, output + {out_off}", in_offset=in_off, out_offset=out_off,
                          repl_offset=(in_off + 5 * out_off) % 16)
    for repl_off in range(16):
        check_replace(words, data, tokens, lengths, TABLES["shrink"], f"replacements + {repl_off}", repl_offset=repl_off, in_offset=3, out_offset=9)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 33, TILE - 1, TILE, TILE + 1, 3 * TILE + 7])
def test_replace_sizes_around_the_steps(words, n):
    rng = np.random.Generator(np.random.PCG64(n))
    data = text_of(rng, n, 0.2)
    lengths = pattern_lengths(WORDS)
    lists = [ref.disjoint_py(WORDS, data.tobytes()), (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))]
    data2 = data.copy()
    data2[0] = data2[-1] = ord("x")                               # a token at byte 0 and one that ends at the last byte
    for k, (d, tokens) in enumerate(((data, lists[0]), (data, lists[1]), (data2, ref.disjoint_py(WORDS, data2.tobytes())))):
        for kind in ("same", "delete", "grow"):
            for off in (0, 3):
                check_replace(words, d, tokens, lengths, TABLES[kind], f"{n} bytes/list {k}/{kind}/offset {off}", in_offset=off, out_offset=(off * 5) % 16)


def test_replace_on_tile_boundaries(words):
    """replacements that begin or end exactly where a tile of the output ends; tiles are cut on the output ADDRESS: with and without an offset"""
    lengths = pattern_lengths(WORDS)
    table = [b"", b"0123456789", b"", b"X", LONG]
    for off in (0, 9):
        for lead in (TILE - off - 10, TILE - off, TILE - off - 1, TILE - off - 5, 2 * TILE - off - 9000 % TILE):
            data = b"." * lead + b"needle" + b"," * 50 + b"x" + b"ab" + b";" * (TILE - 60) + b"QQQQ" + b"tail" * 700 + b"needle"
            tokens = ref.disjoint_py(WORDS, data)
            check_replace(words, data, tokens, lengths, table, f"lead {lead}/offset {off}", out_offset=off, in_offset=(off + 3) % 16)


def test_replace_more_tokens_in_a_tile_than_one_staging_trip_holds(workdir):
    h = gpu_handle(pattern_file(workdir, "dj_justa", [b"a"]))
    try:
        n = 2 * TILE
        for data in (b"a" * n, b"head " + b"a" * n + b" tail"):
            tokens = ref.disjoint_py([b"a"], data)
            for repl in (b"b", b"", b"bb"):
                for off in (0, 6):
                    check_replace(h, data, tokens, [0, 1], [b"", repl], f"a -> {repl!r}/{len(data)} bytes/offset {off}", out_offset=off, in_offset=off // 2)
    finally:
        h.destroy()


def test_replace_truncation(words):
    rng = np.random.Generator(np.random.PCG64(3))
    data = text_of(rng, 3 * TILE)
    tokens = ref.disjoint_py(WORDS, data.tobytes())
    want = ref.replace_py(data.tobytes(), tokens[0], tokens[1], pattern_lengths(WORDS), TABLES["grow"])
    assert len(want) > 3 * TILE
    for cap in (0, 1, TILE - 1, TILE, len(want) - 1):
        for off in (0, 5):
            st, total, got = device_replace(words, data, tokens[0], tokens[1], TABLES["grow"], capacity=cap, out_offset=off)     # (checks the guards)
            assert (st, total) == (TRUNCATED, len(want)), f"capacity {cap}"
    st, total, got = device_replace(words, data, tokens[0], tokens[1], TABLES["grow"], capacity=len(want) + 100)
    assert (st, total, got) == (0, len(want), want)


def test_replace_size_is_computed_in_64_bits(workdir):
    h = gpu_handle(pattern_file(workdir, "dj_justa", [b"a"]))
    try:
        n = 64 << 10
        tokens, covered = device_disjoint(h, np.full(n, ord("a"), dtype=np.uint8))
        assert tokens[0].size == n == covered
        st, total, _ = device_replace(h, b"a" * n, tokens[0], tokens[1], [b"", b"r" * n], capacity=0)
        assert (st, total) == (TRUNCATED, 1 << 32)
    finally:
        h.destroy()


def test_replace_without_tokens_is_a_copy(words):
    rng = np.random.Generator(np.random.PCG64(8))
    data = rng.integers(0, 256, size=3 * TILE + 5, dtype=np.uint8)
    empty = np.zeros(0, dtype=np.int32)
    for off in (0, 7):
        st, total, got = device_replace(words, data, empty, empty, TABLES["grow"], in_offset=off, out_offset=(off * 3) % 16)
        assert (st, total, got) == (0, data.size, data.tobytes())
    st, total, got = device_replace(words, data, empty, empty, TABLES["grow"], capacity=100)
    assert (st, total, got) == (TRUNCATED, data.size, data.tobytes()[:100])
    d, d_out = dev(data), torch.full((data.size,), 0xEE, dtype=torch.uint8, device="cuda:0")
    assert words.replaceFromDevice(d.data_ptr(), data.size, None, None, 0, None, 0, None, 0, d_out.data_ptr(), data.size) == (0, data.size)
    torch.cuda.synchronize()
    assert torch.equal(d_out, d), "no tokens: the arrays may be null"
    assert words.replaceFromDevice(d.data_ptr(), data.size, None, None, 1, None, 0, None, 0, d_out.data_ptr(), data.size, check=False)[0] == INVALID


def test_replace_hostile_arrays_stay_inside_the_buffers(words):
    """the arrays are the caller's contract: unspecified text is allowed, an access outside the buffers is not"""
    rng = np.random.Generator(np.random.PCG64(9))
    n = 2 * TILE + 50
    data = text_of(rng, n)
    big, F = (1 << 31) - 1, len(WORDS)
    good = repl_table(TABLES["grow"])
    lists = {
        "negative starts": ([1, 2, 3], [-7, -1, -big]),
        "starts beyond size": ([1, 2, 3, 1], [n, n + 1, big, n - 2]),
        "descending": ([1 + k % 4 for k in range(0, n - 10, 37)], list(range(n - 10, 0, -37))),
        "ids 0, F + 1, negative": ([0, F + 1, -1, big, -big, 1], [2, 10, 12, 19, 22, 28]),
        "all the same": ([4] * 3000, [5] * 3000),
    }
    for what, (ids, pos) in lists.items():
        for cap in (0, 100, 3 * n):
            for off in (0, 11):
                st, total, got = device_replace(words, data, ids, pos, table=good, capacity=cap, out_offset=off, in_offset=off // 2)
                assert st in (0, TRUNCATED), what                # (device_replace has checked the guard bytes on both sides)
    tokens = ref.disjoint_py(WORDS, data.tobytes())
    blob = np.frombuffer(b"0123456789", dtype=np.uint8).copy()
    for what, off in {"negative": [0, -5, -1, 3, 9, -big], "beyond replBytes": [0, 5, big, 11, 10, 12], "descending": [0, 9, 6, 3, 0, 0]}.items():
        for cap in (0, 3 * n):
            st, total, got = device_replace(words, data, tokens[0], tokens[1], table=(np.array(off, dtype=np.int32), blob), capacity=cap)
            assert st in (0, TRUNCATED), what
    # by the rules: ids outside [1, F] do nothing; a decreasing pair of offsets is an empty replacement; offsets are clamped to [0, replBytes]
    st, total, got = device_replace(words, b"a needle x", [0, 1, F + 1, 3], [0, 2, 8, 9], table=(np.array([0, 8, 4, 4, 99, 99], dtype=np.int32), blob))
    assert (st, got) == (0, b"a  456789")


def test_replace_refuses_overlap(words):
    n = 1000
    buf = torch.full((3 * n,), 0x61, dtype=torch.uint8, device="cuda:0")
    ids, pos = dev(np.array([3], dtype=np.int32)), dev(np.array([0], dtype=np.int32))
    off, blob = repl_table(TABLES["same"])
    d_off, d_blob = dev(off), dev(blob)
    base = buf.data_ptr() + n
    args = (ids.data_ptr(), pos.data_ptr(), 1, d_off.data_ptr(), int(off.size), d_blob.data_ptr(), int(blob.size))
    for delta in (0, 1, -1, n - 1, 1 - n, 16, -16):
        assert words.replaceFromDevice(base, n, *args, base + delta, n, check=False)[0] == INVALID, f"d_out = d_input + {delta}"
    torch.cuda.synchronize()
    assert bool((buf == 0x61).all()), "a refused call wrote"
    for delta in (n, -n):                                       # ranges that touch do not overlap
        assert words.replaceFromDevice(base, n, *args, base + delta, n) == (0, n)
    torch.cuda.synchronize()
    assert bool((buf[n:2 * n] == 0x61).all()) and bool((buf[1:n] == 0x61).all()) and bool((buf[2 * n + 1:] == 0x61).all())


def test_round_trip_equals_re_sub(workdir):
    rng = np.random.Generator(np.random.PCG64(11))
    vocab = sorted({rng.choice(np.frombuffer(b"abcdefgh", dtype=np.uint8), size=int(rng.integers(2, 9))).tobytes() for _ in range(60)})
    repls = [b""] + [(b"<%d>" % k if k % 3 else b"") + (w.upper() if k % 2 else b"") for k, w in enumerate(vocab)]
    data = rng.choice(np.frombuffer(b"abcdefgh  \n", dtype=np.uint8), size=1 << 20)
    lookup = {w: repls[k + 1] for k, w in enumerate(vocab)}
    want = re.sub(b"|".join(re.escape(w) for w in sorted(vocab, key=len, reverse=True)), lambda m: lookup[m.group()], data.tobytes())
    off, blob = repl_table(repls)
    h = gpu_handle(pattern_file(workdir, "dj_vocab", vocab))
    try:
        n = data.size
        d_in, d_off, d_blob = dev(data), dev(off), dev(blob)
        d_ids, d_pos = (torch.full((n + GUARD,), -5, dtype=torch.int32, device="cuda:0") for _ in range(2))
        _, nt, covered = h.matchDisjointFromDevice(d_in.data_ptr(), n, d_ids.data_ptr(), d_pos.data_ptr(), n)
        assert nt > 10000
        d_out = torch.full((len(want) + GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
        st, total = h.replaceFromDevice(d_in.data_ptr(), n, d_ids.data_ptr(), d_pos.data_ptr(), nt, d_off.data_ptr(), int(off.size), d_blob.data_ptr(),
                                        int(blob.size), d_out.data_ptr(), len(want))
        torch.cuda.synchronize()
        assert (st, total) == (0, len(want))
        assert d_out[:total].cpu().numpy().tobytes() == want and bool((d_out[total:] == 0xEE).all())
    finally:
        h.destroy()
