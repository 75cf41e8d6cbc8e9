"""PFACX_coverSpansFromDevice against the two models of tests/cover_ref.py and the host form: intervals at the edges of every level of the
bitmap hierarchy (32, 1024, 32 768, 1 048 576) singly and in one list, the word and thread edges written out by hand, the last word of the
bitmap, the edges of an extract block, a list past one grid pass of the mark launch, 100 000 intervals of 2^31 - 3 bytes each, the seeded
random lists, lengths, hostile entries, every refusal with each overlap, truncation, the count query and the empty list; then the chain a
scanner runs -- class signatures, cover, redaction in place -- for the plain and the batch list, and the cross-check against
PFACX_matchSpansFromDevice.  All arrays are poisoned and carry guard words on both sides; the interval arrays must stay untouched.  Every
comparison is exact."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import cover_ref as ref  # noqa: E402

T = api.PFACX_COVER_BLOCK_BYTES                 # scan_cover.hip: kCoverBlockBits, the positions of one extract block
MARK = api.PFACX_COVER_MARK_BLOCK               # scan_cover.hip: kCoverThreads
PER_CU = api.PFACX_GRID_BLOCKS_PER_CU           # scan_passes.h: gridFor takes eight blocks per compute unit at most
LENGTHS = api.PFACX_COVER_LENGTHS
GUARD = 64
POISON = -5
INVALID, TRUNCATED, ALLOC = api.STATUS.INVALID_PARAMETER, api.STATUS.OUTPUT_TRUNCATED, api.STATUS.CUDA_ALLOC_FAILED


@pytest.fixture(scope="module")
def handle():
    h = api.PFAC.create()
    yield h
    h.destroy()


def guarded(values, dtype=torch.int32):
    """`values` on the device between GUARD poisoned entries -> (tensor, the address of the first value)"""
    t = torch.full((GUARD + len(values) + GUARD,), POISON, dtype=dtype, device="cuda:0")
    if len(values):
        t[GUARD:GUARD + len(values)] = torch.from_numpy(np.ascontiguousarray(values))
    return t, t.data_ptr() + t.element_size() * GUARD


def run_cover(h, starts, second, size, lengths=False, capacity=None, expect_status=None):
    """the device form into poisoned arrays of `capacity` entries (default: the full length, asked for first) -> (status, (starts, lengths,
    covered) written, the number of spans)"""
    a = np.ascontiguousarray(starts, dtype=np.int32)
    b = np.ascontiguousarray(second, dtype=np.int32)
    n, flags = int(a.size), (LENGTHS if lengths else 0)
    (d_a, pa), (d_b, pb) = guarded(a), guarded(b)
    before = d_a.clone(), d_b.clone()
    if n == 0:
        pa = pb = None
    if capacity is None:
        st, capacity, _ = h.coverSpansFromDevice(pa, pb, n, size, flags, None, None, 0, check=False)
        assert st in (0, TRUNCATED) and (st == TRUNCATED) == (capacity > 0)
    out = [torch.full((GUARD + capacity + GUARD,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    ptr = [o.data_ptr() + 4 * GUARD if capacity else None for o in out]
    st, spans, covered = h.coverSpansFromDevice(pa, pb, n, size, flags, ptr[0], ptr[1], capacity, check=False)
    torch.cuda.synchronize()
    if expect_status is not None:
        assert st == expect_status
        return st, None, spans
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (spans > capacity), (st, spans, capacity)
    k = min(spans, capacity)
    for o in out:
        assert bool((o[:GUARD] == POISON).all()) and bool((o[GUARD + capacity:] == POISON).all()), "wrote outside the arrays"
        assert bool((o[GUARD + k:GUARD + capacity] == POISON).all()), "wrote behind the list"
    assert torch.equal(d_a, before[0]) and torch.equal(d_b, before[1]), "the interval arrays, or what lies around them, were modified"
    return st, (out[0][GUARD:GUARD + k].cpu().numpy(), out[1][GUARD:GUARD + k].cpu().numpy(), covered), spans


def check(h, starts, second, size, lengths=False, what="", want=None):
    want = ref.model(starts, second, size, lengths) if want is None else want
    st, got, spans = run_cover(h, starts, second, size, lengths)
    assert st == 0 and spans == len(want[0]), what
    ref.same(got, want, what)
    return want


def mark_grid_pass(h):
    """the intervals one grid pass of pfac_cover_mark takes: gridFor's cap times the block"""
    return PER_CU * int(h.info().multiProcessorCount) * MARK


# ---------------------------------------------------------------- 1. the edges of every level

LEVEL_SIZE = 4 * 1024 * 1024 + 1024 + 37


def level_points(B):
    """k B - 1, k B, k B + 1 for k = 1, 2, 3, 33 (the second word of the level above) and the largest k that fits"""
    last = (LEVEL_SIZE - 1) // B
    return sorted({k * B + d for k in (1, 2, 3, 33, last) if k <= last for d in (-1, 0, 1)})


@pytest.mark.parametrize("B", [32, 1024, 32768, 1048576])
def test_level_edges_singly_and_in_one_list(handle, B):
    points = level_points(B)
    pairs = [(s, e) for s in points for e in points if s < e]
    d_a, d_b = (torch.zeros(1, dtype=torch.int32, device="cuda:0") for _ in range(2))
    out = [torch.full((GUARD + 2 + GUARD,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    clean = out[0].clone()
    for s, e in pairs:                                          # singly: one span, the interval itself
        d_a[0], d_b[0] = s, e
        out[0].copy_(clean)
        out[1].copy_(clean)
        st, spans, covered = handle.coverSpansFromDevice(d_a.data_ptr(), d_b.data_ptr(), 1, LEVEL_SIZE, 0, out[0].data_ptr() + 4 * GUARD,
                                                         out[1].data_ptr() + 4 * GUARD, 2, check=False)
        assert (st, spans, covered) == (0, 1, e - s), (s, e)
        got = torch.stack(out).cpu().numpy()
        assert got[:, GUARD].tolist() == [s, e - s] and np.count_nonzero(got != POISON) == 2, (s, e)
    # all in one list: everything from the first point to the last is covered; then every second of them, which leaves gaps
    check(handle, [s for s, _ in pairs], [e for _, e in pairs], LEVEL_SIZE, what=f"B {B}/all")
    some = [p for p in pairs if p[1] - p[0] <= 2][::2]            # within one k only
    want = check(handle, [s for s, _ in some], [e for _, e in some], LEVEL_SIZE, what=f"B {B}/gaps")
    assert len(want[0]) > 1


def test_level_edges_of_every_level_in_one_list(handle):
    pairs = [(s, e) for B in (32, 1024, 32768, 1048576) for s in level_points(B)[::2] for e in level_points(B)[1::3] if s < e and e - s <= B + 2]
    want = check(handle, [s for s, _ in pairs], [e for _, e in pairs], LEVEL_SIZE, what="all levels")
    assert len(want[0]) > 4


# ---------------------------------------------------------------- 2. word, thread and last-word edges


def test_word_and_thread_edges_by_hand(handle):
    assert len(ref.EDGE_TABLE) >= 40
    for intervals, want in ref.EDGE_TABLE:
        st, got, spans = run_cover(handle, [s for s, _ in intervals], [e for _, e in intervals], ref.EDGE_SIZE)
        assert st == 0 and list(zip(got[0].tolist(), got[1].tolist())) == want and got[2] == sum(n for _, n in want), intervals


@pytest.mark.parametrize("size", [64, 65, 95, T, T + 1, T + 31, 33 * T + 32 * 33 + 31])
def test_last_word_never_yields_positions_at_or_above_size(handle, size):
    assert size % 32 in (0, 1, 31)
    for starts, ends in (([size - 1], [size]), ([size - 40], [size]), ([0], [size]), ([size - 3], [size + 100]), ([0], [size + 100]),
                         ([size - 33, size - 1], [size - 2, ref.INT_MAX]), ([size], [size + 100])):
        want = check(handle, starts, ends, size, what=(size, starts, ends))
        assert all(s + n <= size for s, n in zip(want[0].tolist(), want[1].tolist()))


# ---------------------------------------------------------------- 3. the edges of an extract block


def test_extract_block_edges(handle):
    size = 3 * T + 9
    for starts, ends, spans in (([T - 1], [T + 1], 1), ([1], [3 * T + 5], 1), ([7, T], [T, T + 9], 1), ([T, 7], [T + 9, T], 1),
                                ([7, T + 1], [T, T + 9], 2), ([T - 1, 2 * T], [T, 2 * T + 1], 2), ([0], [T], 1), ([T], [2 * T], 1),
                                ([T - 1, T + 1, 2 * T - 1, 2 * T + 1], [T, T + 2, 2 * T, 2 * T + 2], 4), ([0, 2 * T], [T + 1, 3 * T + 9], 2)):
        want = check(handle, starts, ends, size, what=(starts, ends))
        assert len(want[0]) == spans


def test_most_spans_across_extract_blocks_and_truncation_inside_a_block(handle):
    size = 2 * T + 3
    starts, ends = ref.alternating(size)
    want = check(handle, starts, ends, size, what="alternating")
    total = (size + 1) // 2
    assert len(want[0]) == total and total > T
    order = np.random.RandomState(3).permutation(total)
    ref.same(run_cover(handle, np.array(starts)[order], np.array(ends)[order], size)[1], want, "alternating/shuffled")
    for capacity in (T // 4 + 5, T // 2, T // 2 + 1, total - 1):      # inside the first block, at its last span, at the second block's first
        st, got, spans = run_cover(handle, starts, ends, size, capacity=capacity)
        assert st == TRUNCATED and spans == total and got[2] == total
        assert got[0].tolist() == want[0][:capacity].tolist() and got[1].tolist() == want[1][:capacity].tolist()


# ---------------------------------------------------------------- 4. many intervals, long intervals


def test_intervals_past_one_grid_pass_of_the_mark_launch(handle):
    size, count = 64 * 1024, mark_grid_pass(handle) + 3
    rng = np.random.RandomState(17)
    few_s = rng.randint(0, size - 3000, size=64)
    few_e = few_s + rng.randint(1, 40, size=64)
    pick = rng.randint(0, 64, size=count)
    starts, ends = few_s[pick].astype(np.int32), few_e[pick].astype(np.int32)
    starts[-3:], ends[-3:] = [size - 2000, size - 1000, size - 10], [size - 1990, size - 900, size]      # only the second trip sees these
    want = ref.model(few_s.tolist() + starts[-3:].tolist(), few_e.tolist() + ends[-3:].tolist(), size)
    check(handle, starts, ends, size, what="second trip", want=want)


def test_long_intervals_cost_what_short_ones_cost():
    """100 000 copies of [1, size - 1) at size = 2^31 - 1, with the first and the last byte: levels 5 and 6, no input buffer"""
    size = 2 ** 31 - 1
    starts = np.full(100002, 1, dtype=np.int32)
    ends = np.full(100002, size - 1, dtype=np.int32)
    starts[50000], ends[50000] = 0, 1
    starts[-1], ends[-1] = size - 1, size
    h = api.PFAC.create()
    try:
        (d_a, pa), (d_b, pb) = guarded(starts), guarded(ends)
        out = [torch.full((GUARD + 4 + GUARD,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2)]
        st, spans, covered = h.coverSpansFromDevice(pa, pb, starts.size, size, 0, out[0].data_ptr() + 4 * GUARD, out[1].data_ptr() + 4 * GUARD, 4,
                                                    check=False)
        torch.cuda.synchronize()
        if st == ALLOC:
            words, scratch = size, 0
            while words > 1:
                words = (words + 31) // 32
                scratch += (4 * words + 255) // 256 * 256
            pytest.skip(f"the handle's scratch of about {scratch} bytes could not be allocated")
        assert (st, spans, covered) == (0, 1, size)
        got = torch.stack(out).cpu().numpy()
        assert got[:, GUARD].tolist() == [0, size] and np.count_nonzero(got != POISON) == 2
        st, spans, covered = h.coverSpansFromDevice(pa + 4, pb + 4, 49999, size, 0, None, None, 0, check=False)       # without the two ends
        assert (st, spans, covered) == (TRUNCATED, 1, size - 2)
    finally:
        h.destroy()


# ---------------------------------------------------------------- 5. the models and the host form


@pytest.mark.parametrize("block", range(4))
def test_seeded_lists_against_the_models_and_the_host_form(handle, block):
    for seed in ref.RANDOM_SEEDS[50 * block:50 * block + 50]:
        starts, ends, size = ref.random_list(seed)
        want = check(handle, starts, ends, size, what=f"seed {seed}")
        host = handle.cover_spans_host_array(starts, ends, size)
        ref.same(host, want, f"seed {seed}/host")
        if seed % 5 == 0:
            check(handle, starts, ref.as_lengths(starts, ends), size, lengths=True, what=f"seed {seed}/lengths")
            order = np.random.RandomState(seed + 1000).permutation(len(starts))
            check(handle, [starts[i] for i in order], [ends[i] for i in order], size, what=f"seed {seed}/shuffled")


def test_hostile_entries_and_shapes(handle):
    for name, starts, second, lengths in ref.HOSTILE:
        check(handle, starts, second, ref.HOSTILE_SIZE, lengths, name)
    for name, starts, ends in ref.SHAPES:
        check(handle, starts, ends, ref.SHAPES_SIZE, False, name)
        check(handle, starts, ref.as_lengths(starts, ends), ref.SHAPES_SIZE, True, name + "/lengths")


def test_truncation_count_query_and_no_intervals(handle):
    starts, ends = [40, 3, 90, 20, 3, 60, 21], [45, 8, 99, 22, 5, 61, 30]
    want = ref.model(starts, ends, 100)
    spans = len(want[0])
    for capacity in (0, 1, spans - 1, spans, spans + 1, 1000):   # 1000: more entries than (size + 1) / 2 spans can ever fill
        st, got, total = run_cover(handle, starts, ends, 100, capacity=capacity)
        assert total == spans and got[2] == want[2] and st == (TRUNCATED if capacity < spans else 0)
        k = min(capacity, spans)
        assert got[0].tolist() == want[0][:k].tolist() and got[1].tolist() == want[1][:k].tolist()
    st, got, total = run_cover(handle, [], [], 100, capacity=4)
    assert (st, total, got[2]) == (0, 0, 0)
    st, got, total = run_cover(handle, [5], [9], 0, capacity=4)
    assert (st, total, got[2]) == (0, 0, 0)
    st, got, total = run_cover(handle, [500, -9, 7], [600, 0, 7], 100, capacity=4)      # intervals, and none of them covers anything
    assert (st, total, got[2]) == (0, 0, 0)


def test_every_refusal_and_every_overlap(handle):
    lib = api.load_library()
    (d_a, pa), (d_b, pb) = guarded(np.array([1, 5, 7, 9], dtype=np.int32)), guarded(np.array([3, 9, 8, 12], dtype=np.int32))
    out = [torch.full((8,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    po, pl = out[0].data_ptr(), out[1].data_ptr()
    ns, cb = C.c_size_t(77), C.c_size_t(77)
    H, NS, CB = handle._h, C.byref(ns), C.byref(cb)

    def call(h, start, end, n, size, flags, span_start, span_len, capacity, p_ns, p_cb):
        return lib.PFACX_coverSpansFromDevice(h, start, end, n, size, flags, span_start, span_len, capacity, p_ns, p_cb)

    assert call(None, pa, pb, 4, 20, 0, po, pl, 8, NS, CB) == api.STATUS.INVALID_HANDLE
    assert call(H, pa, pb, 4, 20, 0, po, pl, 8, None, CB) == INVALID and call(H, pa, pb, 4, 20, 0, po, pl, 8, NS, None) == INVALID
    assert call(H, None, pb, 4, 20, 0, po, pl, 8, NS, CB) == INVALID and call(H, pa, None, 4, 20, 0, po, pl, 8, NS, CB) == INVALID
    assert call(H, pa, pb, 4, 20, 0, None, pl, 8, NS, CB) == INVALID and call(H, pa, pb, 4, 20, 0, po, None, 8, NS, CB) == INVALID
    assert call(H, pa, pb, 4, 2 ** 31, 0, po, pl, 8, NS, CB) == INVALID and call(H, pa, pb, 2 ** 31, 20, 0, po, pl, 8, NS, CB) == INVALID
    for flags in (2, 3, 0x80000000):
        assert call(H, pa, pb, 4, 20, flags, po, pl, 8, NS, CB) == INVALID, flags
    # a span array that shares a byte with an interval array: each of the four pairings, at either end of the interval array
    for span_start, span_len in ((pa, pl), (pb, pl), (po, pa), (po, pb), (pa + 12, pl), (po, pb - 4 * 7), (pa - 4 * 7, pl), (po, pb + 12)):
        assert call(H, pa, pb, 4, 20, 0, span_start, span_len, 8, NS, CB) == INVALID, (span_start - pa, span_len - pb)
    torch.cuda.synchronize()
    assert (ns.value, cb.value) == (77, 77) and all(bool((o == POISON).all()) for o in out), "a refused call wrote something"
    assert call(H, pa, pb, 4, 20, 0, pa + 16, pb + 16, 8, NS, CB) == 0 and (ns.value, cb.value) == (2, 9), "arrays that only touch are apart"


# ---------------------------------------------------------------- 6. the chain of a scanner


def redact_by_map(text, starts, ends):
    """model (a) applied to a list: the text with every byte some interval holds overwritten"""
    want = np.frombuffer(text, dtype=np.uint8).copy()
    s, n, _ = ref.spans_by_map(starts, ends, len(text))
    for a, k in zip(s.tolist(), n.tolist()):
        want[a:a + k] = ord("#")
    return want


@pytest.mark.parametrize("batch", [False, True], ids=["plain", "batch"])
def test_class_signatures_cover_and_redaction_in_place(batch):
    text = ref.token_text(7, 64 * 1024)
    n = len(text)
    data = np.frombuffer(text, dtype=np.uint8)
    offsets = np.array([0] + (np.nonzero(data == 10)[0] + 1).tolist() + [n], dtype=np.uint64)
    h = api.PFAC.create()
    try:
        with h.clsigOpenText(b"".join(r + b"\n" for r in ref.CLSIG_RULES)) as sg:
            d_text = torch.from_numpy(data.copy()).to("cuda:0")
            d_ids, d_pos, d_end = (torch.full((n,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(3))
            if batch:
                d_off = torch.from_numpy(offsets.view(np.int64)).to("cuda:0")
                _, count = sg.match_batch_device(d_text.data_ptr(), n, d_off.data_ptr(), offsets.size - 1, d_ids.data_ptr(), d_pos.data_ptr(),
                                                 d_end.data_ptr(), n)
                host_list = sg.match_batch_host_array(data, offsets)
            else:
                _, count = sg.match_device(d_text.data_ptr(), n, d_ids.data_ptr(), d_pos.data_ptr(), d_end.data_ptr(), n)
                host_list = sg.match_host_array(data)
            torch.cuda.synchronize()
            assert count >= 300
            list_before = d_pos.clone(), d_end.clone()
            d_start, d_len = (torch.full((GUARD + count + GUARD,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
            st, spans, covered = h.coverSpansFromDevice(d_pos.data_ptr(), d_end.data_ptr(), count, n, 0, d_start.data_ptr() + 4 * GUARD,
                                                        d_len.data_ptr() + 4 * GUARD, count)
            h.redactSpansFromDevice(d_text.data_ptr(), n, d_start.data_ptr() + 4 * GUARD, d_len.data_ptr() + 4 * GUARD, spans, ord("#"),
                                    d_text.data_ptr())
            torch.cuda.synchronize()
            assert torch.equal(d_pos, list_before[0]) and torch.equal(d_end, list_before[1]), "the list was modified"
            pos, end = d_pos[:count].cpu().numpy(), d_end[:count].cpu().numpy()
            want = redact_by_map(text, pos.tolist(), end.tolist())
            assert 0 < spans <= count and covered == int(np.count_nonzero(want == ord("#")))
            assert np.array_equal(d_text.cpu().numpy(), want), "model (a) over the list the call returned"
            for t in (d_start, d_len):
                assert bool((t[:GUARD] == POISON).all()) and bool((t[GUARD + spans:] == POISON).all())
            # the host chain: the host list through the host form, redacted in numpy
            h_start, h_len, h_covered = h.cover_spans_host_array(host_list[0], host_list[2], n)
            host_text = data.copy()
            for a, k in zip(h_start.tolist(), h_len.tolist()):
                host_text[a:a + k] = ord("#")
            assert h_covered == covered and np.array_equal(host_text, want)
            assert d_start[GUARD:GUARD + spans].cpu().numpy().tolist() == h_start.tolist()
    finally:
        h.destroy()


def test_same_spans_as_match_spans_from_the_all_match_list():
    data = ref.prefix_text(11, 40000)
    n = int(data.size)
    h = api.PFAC.create()
    try:
        h.readPatternFromMemory(b"".join(p + b"\n" for p in ref.PREFIX_PATTERNS))
        d_in = torch.from_numpy(data).to("cuda:0")
        cap = n * int(h.info().maxMatchesPerPosition)
        d_ids, d_pos = (torch.full((cap,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
        _, count = h.matchAllFromDevice(d_in.data_ptr(), n, d_ids.data_ptr(), d_pos.data_ptr(), cap)
        torch.cuda.synchronize()
        assert count > 8000
        lens = torch.tensor([0] + [len(p) for p in ref.PREFIX_PATTERNS], dtype=torch.int32, device="cuda:0")
        d_len = lens[d_ids[:count].long()].contiguous()
        d_start = d_pos[:count].contiguous()
        a, b = (torch.full((n,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
        _, want_spans, want_covered = h.matchSpansFromDevice(d_in.data_ptr(), n, a.data_ptr(), b.data_ptr(), n)
        torch.cuda.synchronize()
        want = a[:want_spans].cpu().numpy(), b[:want_spans].cpu().numpy(), want_covered
        x, y = (torch.full((want_spans + 2,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
        st, spans, covered = h.coverSpansFromDevice(d_start.data_ptr(), d_len.data_ptr(), count, n, LENGTHS, x.data_ptr(), y.data_ptr(),
                                                    want_spans + 2)
        torch.cuda.synchronize()
        assert (st, spans) == (0, want_spans)
        ref.same((x[:spans].cpu().numpy(), y[:spans].cpu().numpy(), covered), want, "matchSpans")
    finally:
        h.destroy()
