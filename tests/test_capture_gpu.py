"""PFACX_capturePairsFromDevice and PFACX_matchCapturedFromDevice (include/pfac_ext.h; scan_capture.hip) on the GPU.  Every result is compared with
tests/capture_ref.py and, where the skip class is empty, the window 0 and the flags 0, with the record ends that PFACX_splitFromDevice's own offsets
give for the same buffer and class, so the two calls cannot drift apart.  Every call: guard words on both sides of both output arrays, the input and
the list unmodified, stop bytes around the input.  T: a tile, R: the bytes behind it that its bitmaps cover; behind T + R a pair is on the slow path."""

import numpy as np
import pytest
import torch                              # before the library loads its HIP runtime, as in every GPU test module

from pfac_amd import api  # noqa: E402
from tests import capture_ref as ref  # noqa: E402
from tests import split_ref  # noqa: E402

pytestmark = pytest.mark.gpu

T = api.PFACX_SPLIT_TILE
R = api.PFACX_CAPTURE_REACH
AT_POS = api.PFACX_CAPTURE_AT_POS
GUARD = -0x5A5A5A5B                       # no start, no length, not -1
PAD = 4                                   # guard words on each side of an output array
EDGE = 32                                 # bytes in front of and behind the input
INT_MAX = (1 << 31) - 1

KEYS = [b"k=", b"key:", b"longerkey=", b"q" * (R + 76)]                    # ids 1 .. 4; the last is longer than the reach
PATTERNS, LENS = ref.pattern_file(KEYS)
BLANK, STOP = b" ", b";"


@pytest.fixture(scope="module")
def handle():
    assert torch.cuda.is_available(), "GPU tests need a device; there is no CPU fallback to test"
    torch.cuda.set_device(0)
    h = api.PFAC.create()
    h.readPatternFromMemory(PATTERNS)
    yield h
    h.destroy()


def stop_byte(stop):
    return 0x0A if stop is None else (stop[0] if len(stop) else 0x0A)


def on_device(data, mis=0, fill=0x0A):
    """the bytes at an address that is `mis` mod 16, `fill` (a stop byte of the call's class) around them -> (the whole buffer, the input's view)"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    whole = torch.full((EDGE + 16 + data.size + EDGE,), fill, dtype=torch.uint8, device="cuda:0")
    view = whole[EDGE + mis:EDGE + mis + data.size]
    view.copy_(torch.from_numpy(data.copy()))
    assert view.data_ptr() % 16 == mis
    return whole, view


def guarded(n):
    return torch.full((n + 2 * PAD,), GUARD, dtype=torch.int32, device="cuda:0")


def inner(buf, n):
    got = buf.cpu().numpy()
    assert np.all(got[:PAD] == GUARD) and np.all(got[PAD + n:] == GUARD), "written outside an array"
    return got[PAD:PAD + n].copy()


def capture_device(h, view, size, ids, positions, skip, stop, window, flags):
    """-> (status, valStart, valLen); the guards and the list checked"""
    pos = np.ascontiguousarray(positions, dtype=np.int32)
    d_pos = torch.from_numpy(pos.copy()).to("cuda:0")
    idv = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
    d_ids = None if idv is None else torch.from_numpy(idv.copy()).to("cuda:0")
    start, length = guarded(pos.size), guarded(pos.size)
    st = h.capturePairsFromDevice(view.data_ptr(), size, skip, stop, window, flags, None if d_ids is None else d_ids.data_ptr(), d_pos.data_ptr(),
                                  pos.size, start.data_ptr() + 4 * PAD, length.data_ptr() + 4 * PAD, check=False)
    torch.cuda.synchronize()
    assert np.array_equal(d_pos.cpu().numpy(), pos) and (idv is None or np.array_equal(d_ids.cpu().numpy(), idv)), "the list is never written"
    return st, inner(start, pos.size), inner(length, pos.size)


def record_ends(h, view, size, begins, stop, data):
    """what a caller does without the call: PFACX_splitFromDevice's own offsets of the same buffer and class; the end of the record of each b is
    offsets[record + 1] - 1 where that byte is a stop byte, else n"""
    _, segments, _ = h.splitFromDevice(view.data_ptr(), size, stop, 0, None, 0, check=False)
    off = torch.zeros(segments + 1, dtype=torch.int64, device="cuda:0")
    st, n, _ = h.splitFromDevice(view.data_ptr(), size, stop, 0, off.data_ptr(), segments + 1)
    assert (st, n) == (0, segments)
    off = off.cpu().numpy()
    table = split_ref.class_lookup(stop)
    ends = np.full(begins.size, size, dtype=np.int64)
    inside = begins < size
    last = off[np.searchsorted(off, begins[inside], side="right")] - 1
    ends[inside] = np.where(table[data[last]], last, size)
    return ends


def check(h, data, ids, positions, skip=None, stop=None, window=0, flags=0, mis=0, device=None, want=None):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    fill = stop_byte(stop)
    whole, view = device if device is not None else on_device(data, mis, fill)
    if want is None:
        want = ref.capture(data, ids, positions, LENS, skip, stop, window, flags)
    st, start, length = capture_device(h, view, data.size, None if flags & AT_POS else ids, positions, skip, stop, window, flags)
    assert st == api.STATUS.SUCCESS
    assert np.array_equal(start, want[0]), (np.nonzero(start != want[0])[0][:8], start[start != want[0]][:8], want[0][start != want[0]][:8])
    assert np.array_equal(length, want[1]), (np.nonzero(length != want[1])[0][:8], length[length != want[1]][:8], want[1][length != want[1]][:8])
    if not skip and window == 0 and flags == 0:
        found = start >= 0
        ends = record_ends(h, view, data.size, start[found].astype(np.int64), stop, data)
        assert np.array_equal(start[found].astype(np.int64) + length[found], ends), "the value ends where the split's record ends"
    back = whole.cpu().numpy()
    lo = EDGE + mis
    assert np.array_equal(back[lo:lo + data.size], data) and np.all(back[:lo] == fill) and np.all(back[lo + data.size:] == fill), "the input is never written"
    return start, length


def text_with(n, stops=(), blanks=(), stop=ord(";"), blank=ord(" ")):
    """n bytes of 'x' with `stop` at the positions of `stops` and `blank` at those of `blanks` (positions outside the text are dropped)"""
    data = np.full(n, ord("x"), dtype=np.uint8)
    for at, byte in ((blanks, blank), (stops, stop)):
        at = np.asarray([p for p in at if 0 <= p < n], dtype=np.int64)
        data[at] = byte
    return data


def test_hand_table():
    for data, file, lens, skip, stop, window, flags, ids, pos, start, length in ref.table_cases():
        h = api.PFAC.create()
        if file is not None:
            h.readPatternFromMemory(file)
        check(h, data, ids, pos, skip, stop, window, flags, 3, want=(start, length))
        h.destroy()


@pytest.mark.parametrize("mis", [0, 1, 7, 15])
def test_b_s_and_e_at_the_edges_of_a_bitmap_word(handle, mis):
    """b at bits 0 and 63 of a word; a skip run that ends inside the word, at its last bit, at the first of the next and behind it; the value's end in
    the same word, the next word and three words on.  One case per 512-byte slot"""
    n = 60 * 512 + 100
    stops, blanks, begins = [], [], []
    slot = 0
    for bit in (0, 63):
        for run in (0, 1, 63 - bit, 64 - bit, 65 - bit, 130):
            for value in (0, 1, 62, 64, 200):
                b = slot * 512 + 64 + bit
                blanks += range(b, b + run)
                stops.append(b + run + value)
                begins.append(b)
                slot += 1
    assert slot * 512 < n and slot == 60
    data = text_with(n, stops, blanks)
    device = on_device(data, mis, ord(";"))
    start, length = check(handle, data, None, begins, BLANK, STOP, 0, AT_POS, mis, device)
    assert 0 in length and 200 in length
    check(handle, data, None, begins, None, STOP, 0, AT_POS, mis, device)
    check(handle, data, None, begins, BLANK, STOP, 100, AT_POS, mis, device)


@pytest.mark.parametrize("end", [T - 1, T, T + R - 1, T + R, T + R + 1, None])
def test_a_value_that_ends_around_the_tile_and_the_reach(handle, end):
    """pairs of tile 0 whose value ends at the tile's last byte, behind it, at the last bit of the bitmaps, and behind them: the slow path; None: no
    stop byte before n"""
    n = 2 * T + 300
    data = text_with(n, [] if end is None else [end], [T - 9, T - 8])
    begins = [5, T - 9, T - 1]
    for mis in (0, 7):
        device = on_device(data, mis, ord(";"))
        start, length = check(handle, data, None, begins, BLANK, STOP, 0, AT_POS, mis, device)
        assert (start + length).tolist() == [n if end is None else end] * 3
        check(handle, data, None, begins, None, STOP, 0, AT_POS, mis, device)
        check(handle, data, [1, 2, 1], [3, T - 13, T - 3], BLANK, STOP, 0, 0, mis, device)    # the same b by a pattern's length: 5, T - 9, T - 1
        check(handle, data, [1, 2, 1], [3, T - 13, T - 3], None, STOP, 0, 0, mis, device)     # ... and against the split's record ends


def test_a_skip_run_across_a_word_the_tile_end_and_the_reach(handle):
    n = 2 * T + 300
    runs = [(60, 70), (T - 10, T + 5), (T + R - 5, T + R + 5)]
    for lo, hi in runs + [(T - 1, T + R + 40)]:
        data = text_with(n, [hi + 20], range(lo, hi))
        start, length = check(handle, data, None, [lo - 1, lo], BLANK, STOP, 0, AT_POS, 15)       # the last run: a pair of tile 0 whose s lies behind T + R
        assert start.tolist() == [lo - 1, hi] and length.tolist() == [hi + 21 - lo, 20]
    data = text_with(n, [], range(T - 3, n))                               # nothing but blanks to the end: s = e = n, behind the bitmaps
    start, length = check(handle, data, None, [T - 3], BLANK, STOP, 0, AT_POS, 1)
    assert (start.tolist(), length.tolist()) == ([n], [0])


def test_the_window_at_every_edge(handle):
    """b = 100, blanks up to s = 110, the value up to e = 150: w exactly on s, s + 1, e - 1, e, e + 1; then a value without an end from T - 10 on
    and w on T + R and one past it; a window larger than the input"""
    n = 2 * T + 300
    data = text_with(n, [150], range(100, 110))
    device = on_device(data, 7, ord(";"))
    for window, want in ((10, (110, 0)), (11, (110, 1)), (49, (110, 39)), (50, (110, 40)), (51, (110, 40)), (n + 5, (110, 40)), (INT_MAX * 4, (110, 40)),
                         (1, (101, 0))):
        start, length = check(handle, data, None, [100], BLANK, STOP, window, AT_POS, 7, device)
        assert (start[0], length[0]) == want
    for window, want in ((R + 10, R + 10), (R + 11, R + 11), (R + 9, R + 9), (4 * T, n - (T - 10))):
        start, length = check(handle, data, [1, 1], [T - 12, T - 12], BLANK, STOP, window, 0, 7, device)     # b = T - 10
        assert start.tolist() == [T - 10] * 2 and length.tolist() == [want] * 2
        check(handle, data, None, [T - 10], None, STOP, window, AT_POS, 7, device)


def test_a_match_that_ends_with_the_input_or_with_a_tile(handle):
    n = T + 50
    data = text_with(n, [40, T + 20])
    data[n - 2:] = np.frombuffer(b"k=", dtype=np.uint8)
    data[T - 2:T] = np.frombuffer(b"k=", dtype=np.uint8)
    start, length = check(handle, data, [1, 2, 1, 1, 3, 4], [10, T - 4, T - 2, n - 2, n - 5, n - 1], BLANK, STOP, 0, 0, 1)
    assert start.tolist() == [12, T, T, n, n, n] and length.tolist() == [28, 20, 20, 0, 0, 0]
    check(handle, data, [1, 2, 1, 1, 3, 4], [10, T - 4, T - 2, n - 2, n - 5, n - 1], None, STOP, 0, 0, 0)


def test_equal_positions_and_a_long_pattern_in_front_of_a_short_one(handle):
    """two pairs at one position with different ids, as PFACX_matchAll* lists them; a long pattern at a lower position that ends behind a short one at
    a higher position: b is not monotonic, the tiles follow pos; the longest pattern ends behind the bitmaps of its pair's tile"""
    n = 2 * T + 300
    data = text_with(n, [90, 300, T + 7, T + R + 200, 2 * T + 100], [12, 13, T + 3])
    ids = [1, 2, 3, 3, 1, 4, 1, 4, 2, 1]
    pos = [10, 10, 10, 50, 55, T - 80, T - 3, T - 3, T - 1, T + R + 150]
    start, length = check(handle, data, ids, pos, BLANK, STOP, 0, 0, 7)
    assert start.tolist()[:5] == [14, 14, 20, 60, 57] and (start + length).tolist()[5:8] == [T + R + 200, T + 7, T + R + 200]
    check(handle, data, ids, pos, None, STOP, 0, 0, 7)
    check(handle, data, ids, pos, BLANK, STOP, 64, 0, 7)


@pytest.mark.parametrize("n", [2 * T + 1, 3 * T, 5 * T + 9])
def test_tiles_with_and_without_pairs(handle, n):
    """a pair in each of three tiles with an empty tile between; a tile's first pair at its first and at its last byte; a last tile of one byte and
    of exactly T bytes"""
    rng = np.random.Generator(np.random.PCG64(n))
    data = text_with(n, rng.integers(0, n, size=n // 300).tolist(), rng.integers(0, n, size=n // 40).tolist())
    tiles = (n + T - 1) // T
    begins = sorted({0, 17, n - 1, (tiles - 1) * T} | ({2 * T, 2 * T + 5, 3 * T - 1, 4 * T + T // 2, 5 * T} if tiles > 4 else {T - 1, T - 1 + T}))
    begins = [b for b in begins if b < n]
    for mis in (0, 15):
        device = on_device(data, mis, ord(";"))
        check(handle, data, None, begins, BLANK, STOP, 0, AT_POS, mis, device)
        check(handle, data, None, begins, None, STOP, 0, AT_POS, mis, device)
        check(handle, data, [1] * len(begins), begins, None, STOP, 0, 0, mis, device)


@pytest.mark.parametrize("skip,stop", [(b" ", b";"), (b" \t", b"\r\n"), (b" ", bytes(range(56, 256))), (b" ;,", b";,"), (split_ref.FULL_CLASS, b""),
                                       (None, None), (b"x", bytes(range(0, 100)))])
def test_classes(handle, skip, stop):
    """one, two and 200 members in D: both template paths; S overlapping D; S full with D empty"""
    rng = np.random.Generator(np.random.PCG64(len(skip or b"") + 300 * len(stop or b"a")))
    n = T + R + 2500
    pool = list(b"abcxyz=:0123") + list((skip or b"")[:4]) * 3 + list((stop if stop is not None else b"\n")[:4])
    data = np.asarray(rng.choice(pool, size=n), dtype=np.uint8)
    data[T - 400:T + R + 400] = ord("x") if skip != b"x" else ord("y")     # a stretch without a stop byte across the reach
    pos = np.sort(rng.integers(0, n, size=700)).astype(np.int32)
    ids = rng.integers(1, 4, size=pos.size).astype(np.int32)
    device = on_device(data, 7, stop_byte(stop))
    for window in (0, 40):
        check(handle, data, ids, pos, skip, stop, window, 0, 7, device)
    check(handle, data, None, pos, skip, stop, 0, AT_POS, 7, device)
    check(handle, data, ids, pos, None, stop, 0, 0, 7, device)


def test_untrusted_lists(handle):
    """a descending list, ids 0, F + 1 and negative, positions -1, n and INT_MAX: success, the guards and the input intact (inner() and the frame
    check them), (-1, 0) wherever the position lies outside; a sorted list with such ids and positions equals the reference entry for entry"""
    n = 3 * T + 5
    rng = np.random.Generator(np.random.PCG64(11))
    data = text_with(n, rng.integers(0, n, size=200).tolist(), rng.integers(0, n, size=2000).tolist())
    whole, view = on_device(data, 0, ord(";"))
    F = len(KEYS)
    for pos in (np.arange(n + 3, -4, -97), rng.integers(-10, n + 10, size=5000), [2 * T + 1, 5, -3, T, n + 7, 0, T, INT_MAX, -1, n, -INT_MAX - 1]):
        pos = np.asarray(pos, dtype=np.int64).astype(np.int32)
        ids = rng.choice([0, 1, 2, 3, F, F + 1, -1, -INT_MAX, INT_MAX], size=pos.size).astype(np.int32)
        for flags in (0, AT_POS):
            st, start, length = capture_device(handle, view, n, ids, pos, BLANK, STOP, 0, flags)
            outside = (pos < 0) | (pos >= n)
            assert st == api.STATUS.SUCCESS and np.all(start[outside] == -1) and np.all(length[outside] == 0)
    assert np.array_equal(view.cpu().numpy(), data)
    pos = np.sort(np.concatenate([rng.integers(0, n, size=600), [-INT_MAX - 1, -1, -1, n, n + 1, INT_MAX]])).astype(np.int32)
    ids = rng.choice([0, 1, 2, 3, F + 1, -1, -INT_MAX, INT_MAX], size=pos.size).astype(np.int32)
    start, length = check(handle, data, ids, pos, BLANK, STOP, 0, 0, 0, (whole, view))
    assert np.all(start[(ids < 1) | (ids > F)] == -1)


@pytest.mark.parametrize("pairs", [1, 255, 256, 257, 1025])
def test_the_pair_stride_of_a_block(handle, pairs):
    """more and fewer pairs in one tile than the block has threads"""
    n = 2 * T
    rng = np.random.Generator(np.random.PCG64(pairs))
    data = text_with(n, rng.integers(0, n, size=400).tolist(), rng.integers(0, n, size=3000).tolist())
    pos = np.sort(rng.integers(T, 2 * T, size=pairs)).astype(np.int32)
    ids = rng.integers(1, 4, size=pairs).astype(np.int32)
    check(handle, data, ids, pos, BLANK, STOP, 0, 0, 1)
    check(handle, data, ids, np.repeat(pos, 2)[:pairs], None, STOP, 0, 0, 1)


HEADERS = b"GET /index.html HTTP/1.1\r\nHost:   example.org\r\nuser= bob \nContent-Length:\t42\r\nk=\r\nx=last\r\n\r\n"
HEADER_KEYS = [b"host:", b"user=", b"content-length:", b"k=", b"x="]


@pytest.mark.parametrize("nocase", [False, True])
def test_scan_forms_and_the_gather(nocase):
    """reduce, then capture: every capacity around the count, the truncated status, the full count, a caseless handle that folds for the match and
    never for the classes; then the values as text through PFACX_gatherLinesFromDevice, equal to the reference's"""
    text = HEADERS.upper().replace(b"EXAMPLE.ORG", b"example.org").replace(b"BOB", b"bob").replace(b"LAST", b"last") if nocase else HEADERS
    file, lens = ref.pattern_file(HEADER_KEYS if nocase else [b"Host:", b"user=", b"Content-Length:", b"k=", b"x="])
    data = np.frombuffer(text * 400, dtype=np.uint8).copy()                # more than two tiles
    h = api.PFAC.create()
    h.readPatternFromMemoryEx(file, api.PFACX_READ_NOCASE if nocase else 0)
    whole, view = on_device(data, 3)
    n = data.size
    ids_w = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    pos_w = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    _, count_w = h.matchFromDeviceReduce(view.data_ptr(), n, ids_w.data_ptr(), pos_w.data_ptr())
    torch.cuda.synchronize()
    ids_w, pos_w = ids_w.cpu().numpy()[:count_w], pos_w.cpu().numpy()[:count_w]
    assert count_w == 5 * 400
    for skip, stop, window, flags in ((b" \t", b"\r\n", 0, 0), (b" ", b"e", 0, 0), (b" ", b"E", 9, 0), (b" \t", b"\r\n", 0, AT_POS)):
        want = ref.capture(data, ids_w, pos_w, lens, skip, stop, window, flags)
        for capacity in (0, count_w - 1, count_w, count_w + 1):
            ids = torch.full((n,), GUARD, dtype=torch.int32, device="cuda:0")
            pos = torch.full((n,), GUARD, dtype=torch.int32, device="cuda:0")
            start, length = guarded(capacity), guarded(capacity)
            st, count = h.matchCapturedFromDevice(view.data_ptr(), n, skip, stop, window, flags, ids.data_ptr(), pos.data_ptr(),
                                                  start.data_ptr() + 4 * PAD, length.data_ptr() + 4 * PAD, capacity, check=False)
            torch.cuda.synchronize()
            assert count == count_w and st == (api.STATUS.SUCCESS if capacity >= count_w else api.STATUS.OUTPUT_TRUNCATED)
            assert np.array_equal(ids.cpu().numpy()[:count], ids_w) and np.array_equal(pos.cpu().numpy()[:count], pos_w)
            kept = min(capacity, count_w)
            got_start, got_length = inner(start, capacity), inner(length, capacity)
            assert np.array_equal(got_start[:kept], want[0][:kept]) and np.array_equal(got_length[:kept], want[1][:kept])
            assert np.all(got_start[kept:] == GUARD) and np.all(got_length[kept:] == GUARD), "exactly the first capCapacity entries"
    assert not np.array_equal(ref.capture(data, ids_w, pos_w, lens, b" ", b"e", 0, 0)[1], ref.capture(data, ids_w, pos_w, lens, b" ", b"E", 0, 0)[1])
    # the host form on the GPU platform: the staged-piece path, then the host loop
    host = data.copy()
    ids = np.zeros(n, dtype=np.int32)
    pos = np.zeros(n, dtype=np.int32)
    start = np.full(count_w, GUARD, dtype=np.int32)
    length = np.full(count_w, GUARD, dtype=np.int32)
    st, count = h.matchCapturedFromHost(host.ctypes.data, n, b" \t", b"\r\n", 0, 0, ids.ctypes.data, pos.ctypes.data, start.ctypes.data,
                                        length.ctypes.data, count_w)
    want = ref.capture(data, ids_w, pos_w, lens, b" \t", b"\r\n", 0, 0)
    assert (st, count) == (0, count_w) and np.array_equal(pos[:count], pos_w) and np.array_equal(start, want[0]) and np.array_equal(length, want[1])
    # the composition: keys in, values out as text, an entry with valStart == -1 (a position outside the input) an empty line
    d_ids = torch.from_numpy(np.concatenate([ids_w[:7], [1]]).astype(np.int32)).to("cuda:0")
    d_pos = torch.from_numpy(np.concatenate([pos_w[:7], [n]]).astype(np.int32)).to("cuda:0")
    d_start, d_len = guarded(8), guarded(8)
    st = h.capturePairsFromDevice(view.data_ptr(), n, b" \t", b"\r\n", 0, 0, d_ids.data_ptr(), d_pos.data_ptr(), 8, d_start.data_ptr() + 4 * PAD,
                                  d_len.data_ptr() + 4 * PAD)
    want = ref.capture(data, d_ids.cpu().numpy(), d_pos.cpu().numpy(), lens, b" \t", b"\r\n", 0, 0)
    assert want[0][7] == -1 and np.array_equal(inner(d_start, 8), want[0]) and np.array_equal(inner(d_len, 8), want[1])
    text_want = ref.values_text(data, want[0], want[1])
    assert text_want == b"example.org\nbob \n42\n\nlast\nexample.org\nbob \n\n"
    out = torch.full((len(text_want) + 8,), 0x23, dtype=torch.uint8, device="cuda:0")
    st, out_bytes = h.gatherLinesFromDevice(view.data_ptr(), n, d_start.data_ptr() + 4 * PAD, d_len.data_ptr() + 4 * PAD, 8, out.data_ptr(), len(text_want))
    torch.cuda.synchronize()
    got = out.cpu().numpy().tobytes()
    assert (st, out_bytes) == (0, len(text_want)) and got[:len(text_want)] == text_want and got[len(text_want):] == b"#" * 8
    assert np.array_equal(view.cpu().numpy(), data) and np.array_equal(host, data)
    h.destroy()


def r256(b):
    return (b + 255) & ~255


def scratch_formula(size):
    """the formula of include/pfac_ext.h"""
    return r256(4 * ((size + T - 1) // T)) + r256(8)


def test_scratch_accounting():
    h = api.PFAC.create()                  # no pattern set, PFACX_CAPTURE_AT_POS: the capture scratch alone
    before = int(h.info().deviceScratchBytes)
    for size in (70 * T + 1, 70 * T + 1, 64):
        data = text_with(size, [40])
        whole, view = on_device(data, 0, ord(";"))
        st, start, length = capture_device(h, view, size, None, [0, size - 1], BLANK, STOP, 0, AT_POS)
        assert st == 0 and start.tolist() == [0, size - 1] and length.tolist() == [40, 1 if size > 64 else 1]
        assert int(h.info().deviceScratchBytes) - before == scratch_formula(70 * T + 1), "grown once, by the header's formula; never again"
    h.trim()
    assert int(h.info().deviceScratchBytes) == before
    h.destroy()


def test_empty_calls_and_statuses(handle):
    data = np.frombuffer(b"k= v;key:w;", dtype=np.uint8)
    whole, view = on_device(data, 1, ord(";"))
    x = guarded(4)
    good = (view.data_ptr(), data.size, BLANK, STOP, 0, 0, x.data_ptr(), x.data_ptr(), 1, x.data_ptr(), x.data_ptr())
    assert handle.capturePairsFromDevice(*good[:8], 0, None, None, check=False) == 0, "numPairs == 0"
    assert handle.capturePairsFromDevice(good[0], 0, *good[2:], check=False) == 0, "size == 0"
    assert np.all(x.cpu().numpy() == GUARD), "no array is touched"
    assert handle.capturePairsFromDevice(*good[:5], 2, *good[6:], check=False) == api.STATUS.INVALID_PARAMETER
    assert handle.capturePairsFromDevice(*good[:6], None, *good[7:], check=False) == api.STATUS.INVALID_PARAMETER, "null ids without AT_POS"
    bare = api.PFAC.create()
    assert bare.capturePairsFromDevice(*good, check=False) == api.STATUS.PATTERNS_NOT_READY
    bare.destroy()
    host_only = api.PFAC.createHostOnly()
    assert host_only.capturePairsFromDevice(*good[:5], AT_POS, *good[6:], check=False) == api.STATUS.LIB_NOT_EXIST
    host_only.destroy()
    start, length = check(handle, data, [1, 2], [0, 5], BLANK, STOP, 0, 0, 1, (whole, view))
    assert (start.tolist(), length.tolist()) == ([3, 9], [1, 1])
