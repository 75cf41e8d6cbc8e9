"""The model of the stream calls (PFACX_stream*) for tests/test_stream_host.py and test_stream_gpu.py.

Nothing here uses the library's stream code.  The expected answer starts from the FULL list of the concatenated stream S -- the
oracle's result over S as one buffer -- and is split by the finality rule of include/pfac_ext.h into what every single call and the
flush must return: with M = maxPatternLen, T = bytes seen with the piece and R = where the previous call stopped, a piece call
reports exactly the pairs at stream positions [R, max(R, T - (M - 1))), the flush those at [R, T); positions are made relative to the
first byte of the piece of that call (the flush: to T).  The tests compare call by call, not only the concatenated total.

The cuts come from a seeded generator that mixes the sizes that matter (0, 1, M - 2, M - 1, M, M + 1, a few KiB, runs of pieces
shorter than M) and PLACES cuts strictly inside occurrences taken from the model's list: random cuts alone rarely hit one.
"""
import numpy as np


def pattern_lengths(pattern_file):
    """pattern length by id (ids are line numbers from 1; entry 0 is 0)"""
    with open(pattern_file, "rb") as f:
        raw = f.read()
    lines = raw.split(b"\n")[:-1]                 # bytes behind the last newline are no pattern
    return np.array([0] + [len(l) for l in lines], dtype=np.int64)


def full_list(pattern_file, data):
    """(positions, ids) of the whole stream as one buffer, ascending position: the oracle's result"""
    from oracle import binding as ob
    o = ob.Oracle(pattern_file, hashed=False)
    try:
        full = o.match(np.ascontiguousarray(data, dtype=np.uint8))
    finally:
        o.close()
    pos = np.flatnonzero(full > 0).astype(np.int64)
    return pos, full[pos].astype(np.int32)


def split(pos, ids, sizes, max_len):
    """[(ids, piece-relative positions, piece offset)] for every piece call, then (ids, positions relative to T) of the flush"""
    calls = []
    T = R = 0
    for size in sizes:
        off = T
        T += int(size)
        if size == 0:
            calls.append((np.zeros(0, np.int32), np.zeros(0, np.int32), off))
            continue
        R2 = max(R, T - (max_len - 1))
        a, b = np.searchsorted(pos, R), np.searchsorted(pos, R2)
        calls.append((ids[a:b].astype(np.int32), (pos[a:b] - off).astype(np.int32), off))
        R = R2
    a = np.searchsorted(pos, R)
    flush = (ids[a:].astype(np.int32), (pos[a:] - T).astype(np.int32))
    return calls, flush


def straddling(pos, ids, lengths, sizes):
    """how many occurrences of the model's list have a cut strictly inside them"""
    cuts = np.unique(np.cumsum(np.asarray(sizes, dtype=np.int64))[:-1]) if len(sizes) > 1 else np.zeros(0, np.int64)
    if pos.size == 0 or cuts.size == 0:
        return 0
    ends = pos + lengths[ids]                      # one behind the last byte
    first_cut_behind_start = np.searchsorted(cuts, pos, side="right")      # first cut > pos
    ok = first_cut_behind_start < cuts.size
    inside = np.zeros(pos.size, dtype=bool)
    inside[ok] = cuts[first_cut_behind_start[ok]] < ends[ok]
    return int(np.count_nonzero(inside))


def per_piece_differs(pattern_file, data, pos, ids, lengths, sizes):
    """how many positions of the model's list get ANOTHER id (or none) from per-piece matching -- the oracle over the bytes from the
    position to the end of its piece, which is what one plain call per piece sees there"""
    from oracle import binding as ob
    data = np.ascontiguousarray(data, dtype=np.uint8)
    cuts = np.unique(np.cumsum(np.asarray(sizes, dtype=np.int64)))
    ends = pos + lengths[ids]
    nxt = np.searchsorted(cuts, pos, side="right")
    o = ob.Oracle(pattern_file, hashed=False)
    differ = 0
    try:
        for k in np.flatnonzero(cuts[np.minimum(nxt, cuts.size - 1)] < ends):
            piece_end = int(cuts[nxt[k]])
            alone = o.match(np.ascontiguousarray(data[int(pos[k]):piece_end]))
            differ += int(alone[0] != ids[k])
    finally:
        o.close()
    return differ


def make_sizes(n, max_len, pos, ids, lengths, seed, placed=20, twice=5, coarse=24):
    """piece sizes (sum n) for a stream of n bytes: the mixed sizes, runs of short pieces, placed cuts, coarse pieces for the rest"""
    rng = np.random.Generator(np.random.PCG64(seed))
    M = max(1, int(max_len))
    cuts = []
    # cuts placed strictly inside occurrences (all of them where there are fewer than `placed`), two cuts inside `twice` of them
    long_enough = np.flatnonzero(lengths[ids] >= 2) if pos.size else np.zeros(0, np.int64)
    chosen = long_enough if long_enough.size <= placed else rng.choice(long_enough, size=placed, replace=False)
    second = 0
    for k in chosen:
        p, ln = int(pos[k]), int(lengths[ids[k]])
        c1 = p + int(rng.integers(1, ln))
        cuts.append(c1)
        if second < twice and ln >= 3:
            c2 = p + int(rng.integers(1, ln))
            if c2 != c1:
                cuts.append(c2)
                second += 1
    # the sizes that matter, from the start of the stream, each followed by a run of pieces shorter than M
    x = 0
    for size in (0, 1, M - 2, M - 1, M, M + 1, 0, 3000, 2 * M + 5, 4097):
        if size < 0:
            continue
        x += size
        if x >= n:
            break
        cuts.append(x)                              # (size 0: the same cut twice = an empty piece)
        for _ in range(6):
            x += int(rng.integers(1, M)) if M > 1 else 1
            if x >= n:
                break
            cuts.append(x)
    # a long run of short pieces somewhere in the middle
    x = n // 2
    for _ in range(40):
        x += int(rng.integers(1, M)) if M > 1 else 1
        if x < n:
            cuts.append(x)
    # coarse pieces over the rest
    for c in rng.integers(1, max(2, n), size=coarse):
        cuts.append(int(c))
    cuts = sorted(c for c in cuts if 0 < c < n or c == 0)
    edges = [0] + cuts + [n]
    sizes = [edges[i + 1] - edges[i] for i in range(len(edges) - 1)]
    assert sum(sizes) == n and min(sizes) >= 0
    return sizes


def run(stream_piece, stream_flush, data, sizes, calls, flush, what):
    """feed `data` cut by `sizes` through stream_piece(offset, size) -> (ids, pos, piece offset) and stream_flush() -> (ids, pos);
    compare every call with the model's split"""
    off = 0
    for k, size in enumerate(sizes):
        got_ids, got_pos, got_off = stream_piece(off, size)
        want_ids, want_pos, want_off = calls[k]
        where = f"{what}: call {k} (offset {off}, size {size})"
        assert got_off == want_off, f"{where}: piece offset {got_off}, want {want_off}"
        assert got_ids.size == want_ids.size, f"{where}: {got_ids.size} pairs, want {want_ids.size}"
        assert np.array_equal(got_pos, want_pos), f"{where}: positions differ"
        assert np.array_equal(got_ids, want_ids), f"{where}: ids differ"
        off += size
    got_ids, got_pos = stream_flush()
    assert got_ids.size == flush[0].size, f"{what}: flush: {got_ids.size} pairs, want {flush[0].size}"
    assert np.array_equal(got_pos, flush[1]) and np.array_equal(got_ids, flush[0]), f"{what}: flush differs"
