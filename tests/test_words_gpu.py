"""PFACX_matchWordsFromDevice / PFACX_wordsPairsFromDevice / PFACX_matchWordsFromHost (GPU platform) against the references of tests/words_ref.py:
every case of the table at two input alignments, random cases in every kernel variant and mode, pair counts around the block size, more pairs than one
grid pass takes, ALL with truncation, one input above the 32 MiB switch, a 100 000-pattern set, the pairs form over the lists of the reduce and the
batch reduce call and over lists with ids and positions that must be ignored, the term frequencies of PFACX_countPairsFromDevice over the ALL list,
the scratch accounting, the caller's bytes.  All arrays are poisoned and carry guard words on both sides."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import allmatch_ref as am  # noqa: E402
from tests import scale_sets as ss  # noqa: E402
from tests import words_ref as ref  # noqa: E402
from tests.gpu_helpers import MODES, VARIANTS, make_handle  # noqa: E402
from tests.spans_helpers import pattern_file, random_case  # noqa: E402
from tests.spans_ref import brute_result  # noqa: E402
from tests.test_count_gpu import prefix_of, scale_text  # noqa: E402  (cached for the session: the prefix table of 100 000 patterns is built once)

ALL = api.PFACX_WORDS_ALL
BLOCK = api.PFACX_WORDS_BLOCK               # scan_words.hip: kWordsBlock
GUARD = 64
POISON = -5
INVALID, TRUNCATED = api.STATUS.INVALID_PARAMETER, api.STATUS.OUTPUT_TRUNCATED


def as_array(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)


def cls_arg(cls):
    return None if cls is None else api.word_class(cls)


def gpu_handle(pf, flags=0, variant=api.PFACX_KERNEL_AUTO, perf=api.PFAC_TIME_DRIVEN, tex=api.PFAC_TEXTURE_OFF):
    h = api.PFAC.create()
    h.setPerfMode(perf)
    h.setTextureMode(tex)
    h.setKernelVariant(variant)
    h.readPatternFromFileEx(pf, flags)
    return h


def out_arrays(cap):
    return tuple(torch.full((GUARD + cap + GUARD,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))


def check_guards(arrays, cap, clean_from):
    """nothing in front of the arrays, at or behind capacity, or in [clean_from, capacity)"""
    for a in arrays:
        assert bool((a[:GUARD] == POISON).all()) and bool((a[GUARD + cap:] == POISON).all()), "wrote outside the arrays"
        assert bool((a[GUARD + clean_from:GUARD + cap] == POISON).all()), "wrote behind the list"


def device_words(h, data, cls, flags, in_offset=0, capacity=None, keep_on_device=False):
    """matchWordsFromDevice -> (status, (pos, ids) of the pairs written, the full length).  The arrays take the scan's unordered list below `size`;
    behind max(size, the list) and outside the arrays nothing may be written, and the input must stay untouched"""
    data = as_array(data)
    n = int(data.size)
    cap = n * max(1, int(h.info().maxMatchesPerPosition)) if capacity is None else capacity
    d_in = torch.zeros(n + in_offset + 64, dtype=torch.uint8, device="cuda:0")
    src = torch.from_numpy(data.copy()).to("cuda:0")
    d_in[in_offset:in_offset + n] = src
    d_ids, d_pos = out_arrays(cap)
    st, total = h.matchWordsFromDevice(d_in.data_ptr() + in_offset, n, cls_arg(cls), flags, d_ids.data_ptr() + 4 * GUARD, d_pos.data_ptr() + 4 * GUARD, cap,
                                       check=False)
    torch.cuda.synchronize()
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > cap), (st, total, cap)
    k = min(total, cap)
    check_guards((d_ids, d_pos), cap, min(cap, max(k, n)))
    assert torch.equal(d_in[in_offset:in_offset + n], src), "the caller's input was modified"
    assert bool((d_in[:in_offset] == 0).all()) and bool((d_in[in_offset + n:] == 0).all())
    pos, ids = d_pos[GUARD:GUARD + k], d_ids[GUARD:GUARD + k]
    return st, ((pos, ids) if keep_on_device else (pos.cpu().numpy(), ids.cpu().numpy())), total


def device_pairs(h, d_in, n, cls, flags, pair_ids, pair_pos, capacity):
    """wordsPairsFromDevice over a pair list on the host -> (status, (pos, ids), the full length); strictly nothing behind the list"""
    d_pi = torch.from_numpy(np.ascontiguousarray(pair_ids, dtype=np.int32)).to("cuda:0")
    d_pp = torch.from_numpy(np.ascontiguousarray(pair_pos, dtype=np.int32)).to("cuda:0")
    d_ids, d_pos = out_arrays(capacity)
    st, total = h.wordsPairsFromDevice(d_in.data_ptr(), n, cls_arg(cls), flags, d_pi.data_ptr(), d_pp.data_ptr(), len(pair_ids),
                                       d_ids.data_ptr() + 4 * GUARD if capacity else None, d_pos.data_ptr() + 4 * GUARD if capacity else None, capacity,
                                       check=False)
    torch.cuda.synchronize()
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > capacity)
    k = min(total, capacity)
    check_guards((d_ids, d_pos), capacity, k)
    assert np.array_equal(d_pi.cpu().numpy(), pair_ids) and np.array_equal(d_pp.cpu().numpy(), pair_pos), "the caller's pair list was modified"
    return st, (d_pos[GUARD:GUARD + k].cpu().numpy(), d_ids[GUARD:GUARD + k].cpu().numpy()), total


def pairs_by_definition(pair_ids, pair_pos, pats, data, cls, all_matches):
    """the contract of the pairs form, pair by pair: an id outside [1, F] or a position outside [0, n) gives nothing; the chain from the pair's id down,
    each member kept if it fits the buffer and its neighbours are outside the class (whether the pattern occurs there is the caller's business)"""
    prefix, chain, _ = am.prefix_table(pats)
    inw, n = ref.in_class(cls), len(data)
    pos, ids = [], []
    for q, p in zip(pair_ids.tolist(), pair_pos.tolist()):
        if not (1 <= q <= len(pats) and 0 <= p < n) or (p > 0 and inw[data[p - 1]]):
            continue
        steps = max(1, int(chain[q]))
        for _ in range(steps):
            if q < 1:
                break
            e = p + len(pats[q - 1])
            if e == n or (e < n and not inw[data[e]]):
                pos.append(p)
                ids.append(q)
                if not all_matches:
                    break
            q = int(prefix[q])
    return np.array(pos, dtype=np.int32), np.array(ids, dtype=np.int32)


# ---------------------------------------------------------------- the cases of the host file


@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_on_the_device_form_and_the_host_form(workdir, case):
    name, pats, data, cls, nocase = case
    h = gpu_handle(pattern_file(workdir, "words_" + name, pats), api.PFACX_READ_NOCASE if nocase else 0)
    try:
        for flags in (0, ALL):
            want = ref.words_brute(pats, data, cls, bool(flags), nocase)
            for off in (0, 5):
                st, got, total = device_words(h, data, cls, flags, in_offset=off)
                assert st == 0 and total == want[0].size
                ref.same(got, want, f"{name}/device/flags {flags}/offset {off}")
            if name in ref.WANT:
                ids, pos = ref.WANT[name][flags]
                ref.same(got, (pos, ids), f"{name}/device/flags {flags}: against the list worked out by hand")
            if cls is None:
                ref.same(got, ref.words_re(pats, data, bool(flags), nocase), f"{name}/device/flags {flags}: against re")
            got = h.match_words_host_array(as_array(data), cls_arg(cls), bool(flags))     # the GPU platform: the pipelined pairs path, walked on the host
            ref.same(got, want, f"{name}/host form/flags {flags}")
    finally:
        h.destroy()


@pytest.mark.parametrize("perf,tex,mode_name", MODES)
@pytest.mark.parametrize("variant,vname", VARIANTS)
def test_random_cases_every_variant_and_mode(workdir, variant, vname, perf, tex, mode_name):
    from tests.gpu_helpers import oracle_match
    for seed in (4, 7, 11):
        pats, data = random_case(seed)
        pf = pattern_file(workdir, f"words_random{seed}", pats)
        result = oracle_match(pf, data)
        prefix, chain, _ = am.prefix_table(pats)
        lengths = [0] + [len(p) for p in pats]
        h = make_handle(pf, perf, tex, variant)
        try:
            for cls in (b"a", b"ab"):
                for flags in (0, ALL):
                    want = ref.words_from_result(result, (prefix, chain), lengths, data, cls, bool(flags))
                    st, got, total = device_words(h, data, cls, flags)
                    assert st == 0 and total == want[0].size
                    ref.same(got, want, f"seed {seed}/{vname}/{mode_name}/class {cls}/flags {flags}")
        finally:
            h.destroy()


# ---------------------------------------------------------------- pair counts around the block, more than one grid pass


@pytest.mark.parametrize("pairs", [1, BLOCK - 1, BLOCK, BLOCK + 1])
def test_pair_counts_around_the_block(workdir, pairs):
    pats = [b"a", b"ab"]
    data = b"a " * pairs
    h = gpu_handle(pattern_file(workdir, "words_block", pats))
    try:
        for flags in (0, ALL):
            st, got, total = device_words(h, data, None, flags)
            assert (st, total) == (0, pairs)
            assert got[0].tolist() == list(range(0, 2 * pairs, 2)) and got[1].tolist() == [1] * pairs
            st, got, total = device_words(h, data, ref.FULL, flags)          # nothing bounded: every pair counts 0
            assert (st, total) == (0, 0)
    finally:
        h.destroy()


def test_more_pairs_than_one_grid_pass_takes(workdir):
    """600 000 pairs: above 8 blocks x 256 threads x 256 CUs, so blocks take more than 256 pairs each"""
    n = 600_000
    data = np.full(n, ord("a"), dtype=np.uint8)
    h = gpu_handle(pattern_file(workdir, "words_grid", [b"a"]))
    try:
        assert n > 8 * BLOCK * int(h.info().multiProcessorCount)
        d_in = torch.from_numpy(data.copy()).to("cuda:0")
        a_ids, a_pos = (torch.full((n,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
        _, listed = h.matchAllFromDevice(d_in.data_ptr(), n, a_ids.data_ptr(), a_pos.data_ptr(), n)
        assert listed == n
        for flags in (0, ALL):
            st, (pos, ids), total = device_words(h, data, ref.EMPTY, flags, keep_on_device=True)
            assert (st, total) == (0, n)
            assert torch.equal(pos, a_pos) and torch.equal(ids, a_ids), f"flags {flags}: the all-match list"
            assert torch.equal(pos, torch.arange(n, dtype=torch.int32, device="cuda:0")) and bool((ids == 1).all())
    finally:
        h.destroy()


# ---------------------------------------------------------------- truncation


def test_all_with_truncation_writes_exactly_the_first_capacity_pairs(workdir):
    h = gpu_handle(pattern_file(workdir, "words_trunc", ref.SPACED))
    try:
        data = b"a a a a a"
        want = ref.words_brute(ref.SPACED, data, None, True)
        for cap in (14, 9):
            st, got, total = device_words(h, data, None, ALL, capacity=cap)
            assert (st, total) == (TRUNCATED, 15)
            ref.same(got, (want[0][:cap], want[1][:cap]), f"capacity {cap}")
        assert device_words(h, data, None, ALL, capacity=15)[::2] == (0, 15)
    finally:
        h.destroy()
    # chains of depth 8 over several blocks, capacity == size: the cut falls inside a chain and inside a block
    rng = np.random.Generator(np.random.PCG64(8))
    data = as_array(b"".join(b"a" * int(k) + b"b" for k in rng.integers(0, 30, 400)))
    h = gpu_handle(pattern_file(workdir, "words_trunc_nested", ref.NESTED))
    try:
        want = ref.words_brute(ref.NESTED, data.tobytes(), ref.EMPTY, True)
        assert want[0].size > 3 * data.size
        for cap in (data.size, data.size + 1001, want[0].size - 1):
            st, got, total = device_words(h, data, ref.EMPTY, ALL, capacity=cap)
            assert (st, total) == (TRUNCATED, want[0].size)
            ref.same(got, (want[0][:cap], want[1][:cap]), f"nested/capacity {cap}")
    finally:
        h.destroy()


# ---------------------------------------------------------------- a big input, a big set


def check_against_result(h, data, result, table, lengths, cls, what):
    for flags in (0, ALL):
        want = ref.words_from_result(result, table, lengths, data, cls, bool(flags))
        cap = max(int(data.size), int(want[0].size))
        st, (pos, ids), total = device_words(h, data, cls, flags, capacity=cap, keep_on_device=True)
        assert (st, total) == (0, want[0].size), f"{what}/flags {flags}"
        assert torch.equal(pos.cpu(), torch.from_numpy(want[0])) and torch.equal(ids.cpu(), torch.from_numpy(want[1])), f"{what}/flags {flags}"
    return want


def test_big_input_through_the_filter_kernel():
    data, result, density = ss.density_stream(0.10)
    assert data.size == ss.BIG
    pats = ss.patterns(ss.C3)
    h = make_handle(ss.pattern_file(ss.C3), api.PFAC_SPACE_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        want = check_against_result(h, data, result, prefix_of(tuple(pats)), [0] + [len(p) for p in pats], None, f"{ss.BIG} bytes")
        assert want[0].size > 100, "some occurrences are whole words"
    finally:
        h.destroy()


def test_a_100_000_pattern_set():
    pats = tuple(ss.patterns(ss.S100))
    data = scale_text(pats)
    pf = ss.pattern_file(ss.S100)
    result = ss.want(pf, data)
    h = make_handle(pf, api.PFAC_SPACE_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        lengths = [0] + [len(p) for p in pats]
        want = check_against_result(h, data, result, prefix_of(pats), lengths, None, "S100/default class")
        assert want[0].size > 100
        check_against_result(h, data, result, prefix_of(pats), lengths, b"0123456789", "S100/digits")
    finally:
        h.destroy()


# ---------------------------------------------------------------- the pairs form


def test_pairs_form_over_the_reduce_and_the_batch_reduce_list(workdir):
    pats = [b"foo", b"foobar", b"bar", b"o", b"foob"]
    data = as_array(b"foo bar foobar,foobarx foo o oo foob|bar foo" * 30)
    n = int(data.size)
    h = gpu_handle(pattern_file(workdir, "words_pairs", pats))
    try:
        d_in = torch.from_numpy(data.copy()).to("cuda:0")
        d_ids, d_pos = (torch.full((n,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
        _, count = h.matchFromDeviceReduce(d_in.data_ptr(), n, d_ids.data_ptr(), d_pos.data_ptr())
        torch.cuda.synchronize()
        pair_ids, pair_pos = d_ids[:count].cpu().numpy(), d_pos[:count].cpu().numpy()
        for cls in (None, b"fobar"):
            for flags in (0, ALL):
                want = ref.words_brute(pats, data.tobytes(), cls, bool(flags))
                st, got, total = device_pairs(h, d_in, n, cls, flags, pair_ids, pair_pos, want[0].size + 3)
                assert (st, total) == (0, want[0].size)
                ref.same(got, want, f"reduce list/class {cls}/flags {flags}")
                assert device_words(h, data, cls, flags)[2] == total, "the match call over the same bytes"
                # the count query, and a capacity the list does not fit
                assert device_pairs(h, d_in, n, cls, flags, pair_ids, pair_pos, 0)[::2] == (TRUNCATED if total else 0, total)
                st, got, t2 = device_pairs(h, d_in, n, cls, flags, pair_ids, pair_pos, total - 1)
                assert (st, t2) == (TRUNCATED, total)
                ref.same(got, (want[0][:total - 1], want[1][:total - 1]), "capacity = the length minus 1")
        # the batch reduce call: positions relative to the buffer, no match across a segment border
        offsets = np.array([0, 5, 13, 14, 14, 100, n], dtype=np.uint64)
        d_off = torch.from_numpy(offsets.view(np.int64)).to("cuda:0")
        d_seg = torch.full((offsets.size,), POISON, dtype=torch.int32, device="cuda:0")
        _, count = h.matchBatchFromDeviceReduce(d_in.data_ptr(), n, d_off.data_ptr(), offsets.size - 1, d_ids.data_ptr(), d_pos.data_ptr(), d_seg.data_ptr())
        torch.cuda.synchronize()
        pair_ids, pair_pos = d_ids[:count].cpu().numpy(), d_pos[:count].cpu().numpy()
        result = np.concatenate([brute_result(pats, data[int(a):int(b)].tobytes()) for a, b in zip(offsets[:-1], offsets[1:])])
        assert np.array_equal(pair_pos, np.flatnonzero(result)) and np.array_equal(pair_ids, result[result > 0])
        prefix, chain, _ = am.prefix_table(pats)
        for flags in (0, ALL):
            want = ref.words_from_result(result, (prefix, chain), [0] + [len(p) for p in pats], data, None, bool(flags))
            st, got, total = device_pairs(h, d_in, n, None, flags, pair_ids, pair_pos, n)
            assert (st, total) == (0, want[0].size)
            ref.same(got, want, f"batch list/flags {flags}")
    finally:
        h.destroy()


def test_pairs_form_ignores_what_lies_outside_the_set_and_the_buffer(workdir):
    pats = [b"foo", b"foobar", b"bar", b"o", b"foob", b"o"]                # (id 4 is a duplicate line: the trie holds id 6)
    f = len(pats)
    data = as_array(b"foo bar foobar foo")
    n = int(data.size)
    h = gpu_handle(pattern_file(workdir, "words_junk", pats))
    try:
        d_in = torch.zeros(n + 64, dtype=torch.uint8, device="cuda:0")
        d_in[:n] = torch.from_numpy(data.copy()).to("cuda:0")
        d_in[n:] = ord("o")                                                 # what a read behind the buffer would find
        junk_ids = [0, -1, f + 1, 2**31 - 1, -2**31]
        junk_pos = [-1, -2**31, n, n + 1, 2**31 - 1]
        pair_ids = np.array([1, 2, 3, 2, 2, 1, 5, 4, 6] + junk_ids + [1] * len(junk_pos) + [2, 2, 1, 6], dtype=np.int32)
        pair_pos = np.array([0, 0, 4, 8, 15, 15, 15, 1, 1] + [8] * len(junk_ids) + junk_pos + [n - 5, n - 3, n - 2, n - 1], dtype=np.int32)
        for cls in (None, ref.EMPTY, ref.FULL):
            for flags in (0, ALL):
                want = pairs_by_definition(pair_ids, pair_pos, pats, data.tobytes(), cls, bool(flags))
                st, got, total = device_pairs(h, d_in, n, cls, flags, pair_ids, pair_pos, 64)
                assert (st, total) == (0, want[0].size)
                ref.same(got, want, f"class {cls}/flags {flags}")
        # worked out by hand, ALL under the empty class: a member that does not fit the buffer is not kept, its prefixes are
        got = device_pairs(h, d_in, n, ref.EMPTY, ALL, np.array([2, 2, 1, 6], dtype=np.int32), np.array([n - 5, n - 3, n - 2, n - 1], dtype=np.int32), 16)[1]
        assert got[0].tolist() == [n - 5, n - 5, n - 3, n - 1] and got[1].tolist() == [5, 1, 1, 6], "foobar never fits; foob fits 5 bytes, foo 3, not 2"
    finally:
        h.destroy()


def test_pairs_form_refuses_overlapping_arrays_and_takes_any_capacity(workdir):
    h = gpu_handle(pattern_file(workdir, "words_overlap", [b"ab", b"cd"]))
    try:
        d_in = torch.from_numpy(as_array(b"ab cd ab").copy()).to("cuda:0")
        buf = torch.full((64,), POISON, dtype=torch.int32, device="cuda:0")
        buf[0:3] = torch.tensor([1, 2, 1], dtype=torch.int32)
        buf[8:11] = torch.tensor([0, 3, 6], dtype=torch.int32)
        before = buf.clone()
        B = buf.data_ptr()
        call = lambda ids, pos, cap: h.wordsPairsFromDevice(d_in.data_ptr(), 8, None, 0, B, B + 32, 3, ids, pos, cap, check=False)  # noqa: E731
        for ids, pos in ((B, B + 128), (B + 128, B + 32), (B + 8, B + 128), (B + 128, B + 40), (B + 36, B + 128)):
            assert call(ids, pos, 3)[0] == INVALID
        assert call(B + 4, B + 128, 2)[0] == INVALID and call(B + 12, B + 128, 2) == (TRUNCATED, 3), "arrays that touch but do not overlap"
        assert call(None, None, 0) == (TRUNCATED, 3), "the count query"
        torch.cuda.synchronize()
        assert torch.equal(buf[:3], before[:3]) and torch.equal(buf[8:11], before[8:11]) and torch.equal(buf[40:], before[40:])
        assert call(B + 128, B + 192, 16) == (0, 3)
        torch.cuda.synchronize()
        assert buf[32:35].tolist() == [1, 2, 1] and buf[48:51].tolist() == [0, 3, 6] and bool((buf[35:48] == POISON).all()) and bool((buf[51:] == POISON).all())
    finally:
        h.destroy()


# ---------------------------------------------------------------- term frequencies, scratch


def test_count_pairs_over_the_all_list_gives_whole_word_term_frequencies(workdir):
    pats = [b"the", b"then", b"other", b"he", b"a", b"the end"]
    text = b"the other then bathe the, then the end he a the end. other the-a a" * 50
    data = as_array(text)
    n, f = int(data.size), len(pats)
    want = ref.per_pattern_counts(pats, ref.words_re(pats, text, True))
    # per copy: `the` in front of `,`, twice in `the end`, in `the-a` (the copies join as `a athe`: only the first copy starts with a word), ...
    assert want.tolist() == [0, 201, 100, 100, 50, 101, 100], "the whole words, not `the` inside `other`, `then` and `bathe`"
    h = gpu_handle(pattern_file(workdir, "words_tf", pats))
    try:
        st, (pos, ids), total = device_words(h, data, None, ALL, keep_on_device=True)
        ids = ids.contiguous()
        counts = torch.full((f + 1,), 0x5A5A, dtype=torch.int64, device="cuda:0")
        h.countPairsFromDevice(ids.data_ptr(), total, api.PFACX_COUNT_LONGEST, counts.data_ptr(), f + 1)
        torch.cuda.synchronize()
        assert counts.cpu().numpy().astype(np.uint64).tolist() == want.tolist() and total == int(want.sum())
    finally:
        h.destroy()


def test_scratch_accounting_and_trim(workdir):
    pats = [b"NEEDLE", b"NEE", b"Z"]
    rng = np.random.Generator(np.random.PCG64(4))
    data = rng.integers(97, 123, size=300000, dtype=np.uint8)
    data[rng.random(data.size) < 0.01] = ord("Z")
    data[1000:1008] = np.frombuffer(b" NEEDLE ", dtype=np.uint8)
    n, f = int(data.size), len(pats)
    pairs = int(np.count_nonzero(data == ord("Z"))) + 1
    h = gpu_handle(pattern_file(workdir, "words_scratch", pats))
    try:
        assert pairs <= 8 * BLOCK * int(h.info().multiProcessorCount), "a block per 256 pairs"
        d_in = torch.from_numpy(data.copy()).to("cuda:0")
        d_ids, d_pos = (torch.full((n,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
        # the scan's own scratch, the ordered pair list and the prefix table are there already: the all-match call shares them
        h.matchAllFromDevice(d_in.data_ptr(), n, d_ids.data_ptr(), d_pos.data_ptr(), n)
        torch.cuda.synchronize()
        before = h.info().deviceScratchBytes
        assert device_words(h, data, None, 0)[2] == 1, "NEEDLE between two spaces; every Z has a letter next to it"
        grown = h.info().deviceScratchBytes
        r256 = lambda b: (b + 255) // 256 * 256  # noqa: E731
        blocks = (pairs + BLOCK - 1) // BLOCK
        assert grown - before == r256(8 * (blocks + 1)) + 4 * (f + 1), "the block offsets and the pattern lengths (pfac_ext.h)"
        assert device_words(h, data, ref.EMPTY, ALL)[2] == pairs + 1
        assert h.info().deviceScratchBytes == grown, "a second call of the same shape allocates nothing"
        h.trim()
        assert h.info().deviceScratchBytes < before, "trim gives the scratch back"
        trimmed = h.info().deviceScratchBytes
        assert device_words(h, data, None, ALL)[2] == 1
        assert h.info().deviceScratchBytes > trimmed, "the call works again after the trim, on scratch of its own"
    finally:
        h.destroy()
