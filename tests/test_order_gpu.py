"""PFACX_orderHitsFromDevice against the models of tests/order_ref.py and the host form: list lengths around a wave, a tile and one full grid of
the count and scatter launches, the selection of digits (one digit of eight, the sign bit, no digit, maximal skew), stability inside and across
tiles, the wave, lane and round edges of the multisplit, the chains a scanner runs (class signatures -> order -> locate; cover over the ordered
and the unordered list; a batch list under its unchanged segFirst; an edit list with four columns; a signature list with two; a reduce list,
which is ordered already), every refusal, and the scratch.  All arrays are poisoned and carry guard words on both sides.  Every comparison is
exact."""

import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import cover_ref  # noqa: E402
from tests import order_ref as ref  # noqa: E402

T = api.PFACX_ORDER_TILE                        # scan_order_hits.hip: kOrderTile
THREADS = api.PFACX_ORDER_THREADS               # scan_order_hits.hip: kOrderThreads
WAVE_SPAN = T // (THREADS // 64)                # the contiguous part of a tile one wave owns
PER_CU = api.PFACX_GRID_BLOCKS_PER_CU
TIES = api.PFACX_ORDER_TIES_BY_ID
GUARD = 64
POISON = -5
INVALID = api.STATUS.INVALID_PARAMETER


@pytest.fixture(scope="module")
def handle():
    h = api.PFAC.create()
    yield h
    h.destroy()


def guarded(values):
    """`values` on the device between GUARD poisoned entries -> (tensor, the address of the first value)"""
    t = torch.full((GUARD + len(values) + GUARD,), POISON, dtype=torch.int32, device="cuda:0")
    if len(values):
        t[GUARD:GUARD + len(values)] = torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32))
    return t, t.data_ptr() + 4 * GUARD


def run_order(h, starts, ids=None, ends=None, aux=None, ties=False, with_perm=True):
    """the device form over guarded copies -> (columns given ..., perm, was_ordered)"""
    n = len(starts)
    cols = [guarded(np.asarray(c, dtype=np.int32)) if c is not None else None for c in (starts, ids, ends, aux)]
    perm = guarded(np.full(n, POISON, dtype=np.int32)) if with_perm else None
    ptr = [c[1] if c is not None else None for c in cols]
    st, was = h.orderHitsFromDevice(ptr[0], ptr[1], ptr[2], ptr[3], n, TIES if ties else 0, perm[1] if perm else None)
    torch.cuda.synchronize()
    assert st == 0
    for c in cols + [perm]:
        if c is not None:
            assert bool((c[0][:GUARD] == POISON).all()) and bool((c[0][GUARD + n:] == POISON).all()), "wrote outside the arrays"
    out = [c[0][GUARD:GUARD + n].cpu().numpy() for c in cols if c is not None]
    return (*out, perm[0][GUARD:GUARD + n].cpu().numpy() if perm else None, was)


def check(h, starts, ids=None, ends=None, aux=None, ties=False, what="", python_too=True, host_too=True):
    want = ref.model(starts, ids, ends, aux, ties, python_too=python_too)
    got = run_order(h, starts, ids, ends, aux, ties)
    ref.same(got, want, what)
    if host_too:
        ref.same(h.order_hits_host_array(starts, ids, ends, aux, ties_by_id=ties), got, (what, "host form"))
    return want


def arange(n):
    return np.arange(n, dtype=np.int32)


# ---------------------------------------------------------------- 1. list lengths

@pytest.mark.parametrize("n", [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1])
def test_list_lengths(handle, n):
    rng = np.random.RandomState(n)
    starts = rng.randint(-3 * n, 3 * n + 1, size=n).astype(np.int32)
    ids = rng.randint(1, 5, size=n).astype(np.int32)
    ends = (starts + rng.randint(1, 9, size=n)).astype(np.int32)
    for ties in (False, True):
        check(handle, starts, ids, ends, arange(n), ties, (n, ties))
    check(handle, starts, what=(n, "bare"))


def test_one_entry_more_than_a_full_grid(handle):
    """more than one tile per block: the contiguous-range split of the count and scatter launches"""
    n = PER_CU * int(handle.info().multiProcessorCount) * T + 1
    rng = np.random.RandomState(1)
    starts = rng.randint(0, 1 << 20, size=n).astype(np.int32)            # many equal starts: three digits
    aux = arange(n)
    want = check(handle, starts, None, None, aux, False, "full grid + 1", python_too=False)
    assert want[-1] == 0 and np.array_equal(want[1], want[2])


# ---------------------------------------------------------------- 2. digit selection

@pytest.mark.parametrize("digit", range(8))
def test_keys_that_differ_in_one_digit(handle, digit):
    n = 2 * T + 77
    r = np.random.RandomState(digit).randint(0, 256, size=n).astype(np.int64)
    base = 0x12345678
    varied = ((base & ~(0xFF << (8 * (digit & 3)))) | (r << (8 * (digit & 3)))).astype(np.uint32).view(np.int32)
    fixed = np.full(n, base, dtype=np.int32)
    if digit < 4:                                                        # a digit of the id word: only the ties flag sees it
        check(handle, fixed, varied, None, arange(n), True, digit)
        want = check(handle, fixed, varied, None, arange(n), False, (digit, "no flag"))
        assert want[-1] == 1
    else:
        check(handle, varied, fixed, None, arange(n), False, digit)
        check(handle, varied, fixed, None, arange(n), True, (digit, "ties"))


def test_keys_that_differ_only_in_the_sign_bit(handle):
    n = T + 5
    neg = np.random.RandomState(3).randint(0, 2, size=n).astype(bool)
    starts = np.where(neg, 5 + ref.INT_MIN, 5).astype(np.int32)
    want = check(handle, starts, None, None, arange(n), False, "sign of start")
    assert want[0][0] < 0 < want[0][-1]
    check(handle, np.full(n, 7, dtype=np.int32), starts, None, arange(n), True, "sign of id")


def test_keys_that_agree_everywhere(handle):
    n = T + 1
    for ties in (False, True):
        want = check(handle, np.full(n, -9, dtype=np.int32), np.full(n, 4, dtype=np.int32), None, arange(n)[::-1].copy(), ties, "all equal")
        assert want[-1] == 1


@pytest.mark.parametrize("at", [0, 1, 64, T - 1, T, 2 * T])
def test_one_entry_differs_from_all_the_others(handle, at):
    n = 2 * T + 1
    for odd in (ref.INT_MIN, 0x00010000, ref.INT_MAX):
        starts = np.full(n, 0x00020000, dtype=np.int32)
        starts[at] = odd
        check(handle, starts, None, None, arange(n), False, (at, odd))


# ---------------------------------------------------------------- 3. stability

def test_stability_inside_and_across_tiles(handle):
    n = T + 1
    want = check(handle, np.full(n, 3, dtype=np.int32), None, None, arange(n), False, "one start")
    assert want[-1] == 1
    n = 2 * T + 1
    starts = (np.array([30, 10, 20], dtype=np.int32))[arange(n) % 3]
    want = check(handle, starts, None, None, arange(n), False, "three starts interleaved")
    third = (n + 2) // 3
    assert want[1][:4].tolist() == [1, 4, 7, 10] and (np.diff(want[1][:len(range(1, n, 3))]) == 3).all() and third > T // 2


def test_stability_with_the_ties_flag(handle):
    n = 2 * T + 1
    k = arange(n)
    starts = (k % 3).astype(np.int32)
    ids = (1000 - (k // 3) // 5).astype(np.int32)                         # descending inside each start, in runs of five equal (start, id)
    want = check(handle, starts, ids, None, k, True, "ids descending, runs of five")
    same = (np.diff(want[0]) == 0) & (np.diff(want[1]) == 0)
    assert same.sum() > n // 2 and (np.diff(want[2])[same] > 0).all(), "equal (start, id) keep their incoming order"


# ---------------------------------------------------------------- 4. wave, lane and round edges

def test_wave_lane_and_round_edges(handle):
    k = arange(2 * T)
    cases = {
        "a wave of one digit": (255 - (k // 64) % 256),                   # all 64 lanes of every round hold one digit; descending by round
        "every lane another digit": 255 - (k % 256),                      # 64 distinct digits a round, descending
        "the digit changes at the wave boundary": 3 - (k // WAVE_SPAN) % 4,
        "the digit changes at the round boundary": 1 - (k // 64) % 2,
        "the digit changes one lane off the boundaries": 7 - ((k + 1) // 64) % 8,
        "two digits alternate lane by lane": k % 2 * 200,
    }
    for name, starts in cases.items():
        for n in (T, 2 * T, T + WAVE_SPAN + 64 + 1):
            check(handle, starts[:n].astype(np.int32), None, None, arange(n), False, (name, n))


def test_seeded_lists_and_column_combinations(handle):
    for seed, combo in zip(ref.RANDOM_SEEDS[:16], itertools.cycle(ref.COLUMN_COMBINATIONS)):
        starts, ids, ends, aux = ref.random_list(seed, n=3 * T // 2 + seed)
        cols = ref.pick_columns(starts, ids, ends, aux, combo)
        check(handle, *cols, ties=False, what=(seed, combo))
        if combo[0]:
            check(handle, *cols, ties=True, what=(seed, combo, "ties"))
    got = run_order(handle, [3, 1, 2], with_perm=False)
    assert got[0].tolist() == [1, 2, 3] and got[1] is None and got[2] == 0


# ---------------------------------------------------------------- 5. the chains

def clsig_list(h, text, batch_offsets=None):
    """the device list of the three token rules over `text` -> (ids, pos, end tensors of n entries, count, seg_first or None, the host list)"""
    data = np.frombuffer(text, dtype=np.uint8)
    n = data.size
    with h.clsigOpenText(b"".join(r + b"\n" for r in ref.CLSIG_RULES)) as sg:
        d_text = torch.from_numpy(data.copy()).to("cuda:0")
        d_ids, d_pos, d_end = (torch.full((n,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(3))
        if batch_offsets is not None:
            d_off = torch.from_numpy(batch_offsets.view(np.int64)).to("cuda:0")
            d_first = torch.zeros(batch_offsets.size, dtype=torch.int64, device="cuda:0")
            _, count = sg.match_batch_device(d_text.data_ptr(), n, d_off.data_ptr(), batch_offsets.size - 1, d_ids.data_ptr(), d_pos.data_ptr(),
                                             d_end.data_ptr(), n, d_first.data_ptr())
            first = d_first.cpu().numpy()
        else:
            _, count = sg.match_device(d_text.data_ptr(), n, d_ids.data_ptr(), d_pos.data_ptr(), d_end.data_ptr(), n)
            first = None
        torch.cuda.synchronize()
    return d_text, d_ids, d_pos, d_end, count, first


def test_class_signatures_order_locate_and_cover():
    text = cover_ref.token_text(7, 64 * 1024)
    n = len(text)
    data = np.frombuffer(text, dtype=np.uint8)
    h = api.PFAC.create()
    try:
        d_text, d_ids, d_pos, d_end, count, _ = clsig_list(h, text)
        assert count >= 300
        ids, pos, end = (t[:count].cpu().numpy() for t in (d_ids, d_pos, d_end))
        want = ref.model(pos, ids, end, None, True)
        assert (np.diff(pos) < 0).any(), "the list is not in start order"
        spans = [torch.full((count,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(4)]
        _, ns0, cb0 = h.coverSpansFromDevice(d_pos.data_ptr(), d_end.data_ptr(), count, n, 0, spans[0].data_ptr(), spans[1].data_ptr(), count)
        behind = [t[count:].clone() for t in (d_pos, d_ids, d_end)]          # (the scan's scratch, not poison)
        _, was = h.orderHitsFromDevice(d_pos.data_ptr(), d_ids.data_ptr(), d_end.data_ptr(), None, count, TIES)
        torch.cuda.synchronize()
        assert all(torch.equal(t[count:], b) for t, b in zip((d_pos, d_ids, d_end), behind)), "wrote behind the list"
        got = (d_pos[:count].cpu().numpy(), d_ids[:count].cpu().numpy(), d_end[:count].cpu().numpy())
        for g, w in zip(got, want[:3]):
            assert np.array_equal(g, w)
        assert was == want[-1]
        # locate: record = the newlines in front of the start, column = the distance to the byte behind the last of them
        d_rec, d_col = (torch.full((count,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
        h.locatePairsFromDevice(d_text.data_ptr(), n, None, 0, d_pos.data_ptr(), count, d_rec.data_ptr(), d_col.data_ptr())
        torch.cuda.synchronize()
        newlines = np.nonzero(data == 10)[0]
        rec = np.searchsorted(newlines, got[0], side="left")
        line_start = np.where(rec > 0, newlines[np.maximum(rec, 1) - 1] + 1, 0)
        assert np.array_equal(d_rec.cpu().numpy(), rec) and np.array_equal(d_col.cpu().numpy(), got[0] - line_start)
        # cover: the same spans from the ordered list as from the unordered one
        _, ns1, cb1 = h.coverSpansFromDevice(d_pos.data_ptr(), d_end.data_ptr(), count, n, 0, spans[2].data_ptr(), spans[3].data_ptr(), count)
        torch.cuda.synchronize()
        assert (ns0, cb0) == (ns1, cb1) and ns0 > 0 and torch.equal(spans[0], spans[2]) and torch.equal(spans[1], spans[3])
    finally:
        h.destroy()


def test_batch_list_keeps_its_seg_first():
    text = cover_ref.token_text(9, 32 * 1024)
    data = np.frombuffer(text, dtype=np.uint8)
    offsets = np.array([0] + (np.nonzero(data == 10)[0] + 1).tolist() + [len(text)], dtype=np.uint64)
    h = api.PFAC.create()
    try:
        _, d_ids, d_pos, d_end, count, first = clsig_list(h, text, offsets)
        assert count >= 100 and int(first[-1]) == count
        ids, pos, end = (t[:count].cpu().numpy() for t in (d_ids, d_pos, d_end))
        h.orderHitsFromDevice(d_pos.data_ptr(), d_ids.data_ptr(), d_end.data_ptr(), None, count, 0)
        torch.cuda.synchronize()
        got = (d_pos[:count].cpu().numpy(), d_ids[:count].cpu().numpy(), d_end[:count].cpu().numpy())
        busy = 0
        for s in range(offsets.size - 1):
            a, b = int(first[s]), int(first[s + 1])
            if a == b:
                continue
            want = ref.model(pos[a:b], ids[a:b], end[a:b], python_too=False)
            busy += b - a > 1
            for g, w in zip(got, want[:3]):
                assert np.array_equal(g[a:b], w), s
            assert (got[0][a:b] >= int(offsets[s])).all() and (got[0][a:b] < int(offsets[s + 1])).all()
        assert busy > 10
    finally:
        h.destroy()


def test_edit_list_with_four_columns_and_signature_list_with_two():
    data = np.frombuffer(ref.edit_text(5, 20000), dtype=np.uint8).copy()
    n = data.size
    h = api.PFAC.create()
    try:
        d_in = torch.from_numpy(data).to("cuda:0")
        with h.editOpen(ref.EDIT_PATTERNS, ref.EDIT_BUDGETS) as es:
            cols = [torch.full((n,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(4)]       # ids, pos, end, dist
            st, count = es.match_device(d_in.data_ptr(), n, cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), cols[3].data_ptr(), n)
            torch.cuda.synchronize()
        assert st == 0 and count >= 50
        ids, pos, end, dist = (c[:count].cpu().numpy() for c in cols)
        assert (np.diff(pos) < 0).any(), "the list is not in start order"
        for ties in (False, True):
            got = run_order(h, pos, ids, end, dist, ties)
            ref.same(got, ref.model(pos, ids, end, dist, ties), ("edit", ties))
        with h.sigOpenText(ref.SIG_TEXT) as ss:
            d_ids, d_pos = (torch.full((n,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
            st, count = ss.match_device(d_in.data_ptr(), n, d_ids.data_ptr(), d_pos.data_ptr(), n)
            torch.cuda.synchronize()
        assert st == 0 and count >= 50
        ids, pos = d_ids[:count].cpu().numpy(), d_pos[:count].cpu().numpy()
        want = ref.model(pos, ids, None, None, True)
        assert want[-1] == 0
        _, was = h.orderHitsFromDevice(d_pos.data_ptr(), d_ids.data_ptr(), None, None, count, TIES)
        torch.cuda.synchronize()
        assert was == want[-1] and np.array_equal(d_pos[:count].cpu().numpy(), want[0]) and np.array_equal(d_ids[:count].cpu().numpy(), want[1])
    finally:
        h.destroy()


def test_a_reduce_list_is_ordered_already():
    data = cover_ref.prefix_text(11, 40000)
    n = int(data.size)
    h = api.PFAC.create()
    try:
        h.readPatternFromMemory(b"".join(p + b"\n" for p in cover_ref.PREFIX_PATTERNS))
        d_in = torch.from_numpy(data).to("cuda:0")
        d_ids, d_pos = (torch.full((n,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
        _, count = h.matchFromDeviceReduce(d_in.data_ptr(), n, d_ids.data_ptr(), d_pos.data_ptr())
        torch.cuda.synchronize()
        assert count > 8000
        # copies whose every other byte is poison: a call that writes a column back, even with the same values, is not told apart from one that
        # does not by the values -- so the list is checked through arrays the call must not touch at all, guards included
        ids, pos = d_ids[:count].cpu().numpy(), d_pos[:count].cpu().numpy()
        (t_pos, p_pos), (t_ids, p_ids), (t_perm, p_perm) = guarded(pos), guarded(ids), guarded(np.full(count, POISON, dtype=np.int32))
        before = t_pos.clone(), t_ids.clone()
        _, was = h.orderHitsFromDevice(p_pos, p_ids, None, None, count, 0, p_perm)
        torch.cuda.synchronize()
        assert was == 1 and torch.equal(t_pos, before[0]) and torch.equal(t_ids, before[1])
        assert np.array_equal(t_perm[GUARD:GUARD + count].cpu().numpy(), np.arange(count)) and bool((t_perm[:GUARD] == POISON).all())
        assert bool((t_perm[GUARD + count:] == POISON).all())
    finally:
        h.destroy()


# ---------------------------------------------------------------- 6. refusals and scratch

def test_every_refusal_and_every_overlap(handle):
    lib = api.load_library()
    arrays = [guarded(np.array(v, dtype=np.int32)) for v in ([5, 3, 9, 1], [1, 2, 3, 4], [6, 4, 10, 2], [0, 1, 2, 3], [POISON] * 4)]
    before = [a[0].clone() for a in arrays]
    ps, pi, pe, pa, pp = (a[1] for a in arrays)
    was = C.c_int(77)
    H, W = handle._h, C.byref(was)
    form = lib.PFACX_orderHitsFromDevice
    assert form(None, ps, pi, pe, pa, 4, 0, pp, W) == INVALID
    assert form(H, None, pi, pe, pa, 4, 0, pp, W) == INVALID
    assert form(H, ps, pi, pe, pa, 2 ** 31, 0, pp, W) == INVALID
    for flags in (2, 3, 0x80000000):
        assert form(H, ps, pi, pe, pa, 4, flags, pp, W) == INVALID, flags
    assert form(H, ps, None, pe, pa, 4, TIES, pp, W) == INVALID
    for i, j in itertools.combinations(range(5), 2):
        for shift in (0, 12, -12):
            args = [ps, pi, pe, pa, pp]
            args[j] = args[i] + shift
            assert form(H, args[0], args[1], args[2], args[3], 4, 0, args[4], W) == INVALID, (i, j, shift)
    torch.cuda.synchronize()
    assert was.value == 77 and all(torch.equal(a[0], b) for a, b in zip(arrays, before)), "a refused call wrote something"
    assert form(H, None, None, None, None, 0, 0, None, W) == 0 and was.value == 1
    was.value = 77
    assert form(H, ps, ps + 8, None, None, 2, 0, None, None) == 0, "arrays that only touch are apart; no h_wasOrdered"
    torch.cuda.synchronize()
    assert arrays[0][0][GUARD:GUARD + 4].tolist() == [3, 5, 1, 9]
    hostonly = api.PFAC.createHostOnly()
    try:
        assert form(hostonly._h, ps, pi, pe, pa, 4, 0, pp, W) == api.STATUS.LIB_NOT_EXIST and was.value == 77
    finally:
        hostonly.destroy()


def test_scratch_grows_on_the_first_call_and_trim_gives_it_back():
    h = api.PFAC.create()
    try:
        base = int(h.info().deviceScratchBytes)
        n = 3 * T
        got = run_order(h, arange(n))                                    # ordered: the probe words alone
        probe = int(h.info().deviceScratchBytes) - base
        assert got[-1] == 1 and 0 < probe <= 256
        got = run_order(h, arange(n)[::-1].copy())
        grown = int(h.info().deviceScratchBytes) - base
        assert got[-1] == 0 and got[0].tolist() == list(range(n))
        blocks = 3
        parts = (40, 8 * n, 8 * n, 4 * n, 1024 * blocks, 1024 * blocks + 4)
        assert grown == sum((p + 255) // 256 * 256 for p in parts), "the formula of the header"
        h.trim()
        assert int(h.info().deviceScratchBytes) == base
        assert run_order(h, [2, 1, 2, 1], None, None, [0, 1, 2, 3])[1].tolist() == [1, 3, 0, 2], "and the next call allocates again"
    finally:
        h.destroy()
