"""The cases of tests/test_gather_edges_host.py and tests/test_gather_edges_gpu.py: PFACX_gatherLinesFromDevice where its four launches
(scan_lines.hip: pfac_lines_gather_count, pfac_array_scan<u64>, pfac_lines_gather_offsets, pfac_lines_gather_copy) take another path -- at the
edges of an output tile, of the tile's staging, of a thread's 16 bytes, of the cut of the offset passes and of one pass of the grid.  No test
functions and nothing of the library: a vectorised reference (gather_text, gather_total), a plain Python transcription of the kernels
(tile_model) whose `mutate` switches on one named off-by-one at a time, and builders of cases

    (name, data, start, length, in_offset, out_offset, capacity or None)            capacity None: the size of the whole text

each with `.claims`, the edges it says it reaches, which check_claims() evaluates from the definition of the text alone (offsets by cumsum,
tile bounds from out_offset), never through the model.

    A  a line start on oLo - 1, oLo, oLo + 1, oHi - 1, oHi of tile 1 and of the last tile, and on the first two bytes of tile 1's last
       thread, d_out at 0, 1 and 15 mod 16: the two binary searches
    B  a tile that stages 4096 starts (all empty lines; 4095 empty lines and a line that is not), 4095 starts behind a line that began in front
       of the tile, and one line over three tiles (cnt == 1: every thread takes the lo == 0 branch)
    C  runs of 15, 16, 17 and 33 empty lines between lines of 1 .. 40 bytes at every out_offset; texts that end inside a thread's 16 bytes
    D  255 .. 513 lines, and 8 C 256 - 1, 8 C 256, 8 C 256 + 1 lines on C compute units: the cut of the count and offsets passes
    E  more tiles than one pass of the copy's grid; 65536 lines of 65536 bytes of text: 2^32
    F  descending, overlapping, repeated and hostile lists against the clamped reference
    G  the last line ends with the input, a line starts at n, the input at every offset from a 16-byte boundary

Test infrastructure only."""
import numpy as np

TILE = 4096                             # scan_passes.h: kOutTile = 4096 -- the output bytes of a tile of pfac_lines_gather_copy
STEP = 16                               # scan_passes.h: tileFrame, v0 = vLo + threadIdx.x * 16 -- a thread's bytes of a tile
THREADS = 256                           # scan_lines.hip: kLinesThreads = 256 -- the threads of a block of all three gather kernels
BLOCKS_PER_CU = 8                       # scan_passes.h: offsetBlocks, gridCap(c, 8) -- the most blocks of the count and offsets passes
TILE_BLOCKS_PER_CU = 32                 # scan_lines.hip: PFACX_linesGather, gridCap(c, 8) * 4ull -- the most blocks of the copy
SCAN_STEP = 1024                        # scan_lines.hip: PFACX_linesGather, pfac_array_scan<...>, dim3(1), dim3(1024) -- block totals per step

NL = 10
FILL = 0xEE                             # what tile_model leaves where it writes nothing: the guard byte of the device tests
INT_MAX, INT_MIN = (1 << 31) - 1, -(1 << 31)
U64 = (1 << 64) - 1

# name -> what it changes.  first_lt, last_le, cap_minus_1 and per_unrounded are EQUIVALENT mutants: see equivalent_mutants()
MUTANTS = {
    "first_lt": "the tile's first search: off[mid] < oLo for <= oLo",
    "first_le_plus_1": "the tile's first search: off[mid] <= oLo + 1 for <= oLo",
    "last_le": "the tile's second search: off[mid] <= oHi for < oHi",
    "last_lt_minus_16": "the tile's second search: off[mid] < oHi - 16 for < oHi",
    "cap_minus_1": "the staging holds 4095 starts",
    "rel_lt": "the thread's search: rel[mid] < r for <= r",
    "k_from_tile": "the lo == 0 branch: k = r for cLo - off[first]",
    "per_unrounded": "offsetBlocks: per is not rounded up to the block size (and the blocks follow from it)",
    "per_unrounded_grid_kept": "offsetBlocks: per is not rounded, the blocks are those of the rounded per",
    "no_second_trip": "the tile loop of a block runs once",
}


def equivalent_mutants():
    """name -> why no input can tell it from the kernel.  rel[] serves one purpose, the line a thread STARTS in: a thread looks up r, its
    first byte's distance from oLo, a multiple of 16 that is at most 4080 (less d_out & 15 in tile 0), and walks on from there through the
    list itself, next().  So an offset staged at rel > 4080 is never the answer of a search, and the second search and the cap have 15 bytes
    of slack (last_lt_minus_16 is the first that has none).
    last_le: one more offset is staged, the start at oHi, rel = oHi - oLo; where it makes 4097 of 4096 the cap drops exactly it.
    cap_minus_1: 4096 offsets are staged only when every byte behind oLo is a start; the one dropped is the start at oLo + 4095.
    first_lt: the line in front of a start on oLo becomes the tile's first and the start on oLo rel[1] = 0, which every search prefers to
    rel[0]; the lo == 0 branch is then taken by no thread.  4097 of 4096: see cap_minus_1.
    per_unrounded: both passes bound their items by `end` = min(count, first + per) and step through them a block at a time from `first`; no
    line of them needs first to be a multiple of the block size.  The rounding is for whole waves, not for the result.  What does go wrong is
    a `per` that does not belong to the launched blocks: per_unrounded_grid_kept"""
    return {"last_le": "the start at oHi is staged behind every r and is what the cap drops",
            "cap_minus_1": "the 4096th staged offset is a start on the tile's last byte: no thread starts there",
            "first_lt": "the start on oLo is found as rel[1] = 0; the offset the cap then drops is the tile's last byte",
            "per_unrounded": "the passes bound every item by `end`; per may be any size as long as blocks * per >= count"}


def as_array(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------- the reference

def clamped(n, start, length):
    """include/pfac_ext.h and scan_passes.h: clampSpan -- every (start, len) as [s, e) inside [0, n]"""
    start, length = np.asarray(start, dtype=np.int64), np.asarray(length, dtype=np.int64)
    s = np.minimum(np.maximum(start, 0), n)
    e = np.where(length <= 0, s, np.minimum(n, s + length))
    return s, e


def offsets(n, start, length):
    """(the offset of every line in the text, the size of the text): a line is its bytes and a '\\n'"""
    s, e = clamped(n, start, length)
    v = e - s + 1
    return np.cumsum(v) - v, int(v.sum())


def gather_total(n, start, length):
    return offsets(n, start, length)[1]


def gather_text(data, start, length):
    """the text as a uint8 array: byte j belongs to line `line[j]`, is its byte k[j] or, behind its last byte, the '\\n'"""
    data = as_array(data)
    n = int(data.size)
    s, e = clamped(n, start, length)
    ln = e - s
    off, total = offsets(n, start, length)
    line = np.repeat(np.arange(s.size, dtype=np.int64), ln + 1)
    k = np.arange(total, dtype=np.int64) - off[line]
    newline = k == ln[line]
    out = data[np.where(newline, 0, s[line] + k)] if n else np.zeros(total, dtype=np.uint8)
    out[newline] = NL
    return out


# ---------------------------------------------------------------------------------------------------------------- the model

def offset_blocks(count, compute_units, mutate=None):
    """scan_passes.h: offsetBlocks(c, count, kLinesThreads, per) -> (blocks, per), count >= 1"""
    blocks = (count + THREADS - 1) // THREADS
    if blocks > BLOCKS_PER_CU * compute_units:
        blocks = BLOCKS_PER_CU * compute_units
    plain = (count + blocks - 1) // blocks
    per = (plain + THREADS - 1) // THREADS * THREADS
    if mutate == "per_unrounded":
        return (count + plain - 1) // plain, plain
    if mutate == "per_unrounded_grid_kept":
        return (count + per - 1) // per, plain
    return (count + per - 1) // per, per


def copy_grid(n, count, capacity, mis_out, compute_units):
    """scan_lines.hip: PFACX_linesGather -- the blocks of pfac_lines_gather_copy (capacity > 0)"""
    most = min(count * (n + 1), capacity) + mis_out
    return min((most + TILE - 1) // TILE, TILE_BLOCKS_PER_CU * compute_units)


def model_offsets(n, start, length, compute_units, mutate=None):
    """pfac_lines_gather_count, pfac_array_scan<u64> and pfac_lines_gather_offsets -> (off[count] as a list, the total).  The value of a
    line comes from numpy, the cut into blocks, the scan's steps and each block's running base are the kernels'.  An entry no block writes
    stays 0; an item behind the list reads (0, 0)"""
    count = int(len(start))
    s, e = clamped(n, start, length)
    value = (e - s + 1).tolist()
    at = lambda k: value[k] if 0 <= k < count else 1  # noqa: E731
    blocks, per = offset_blocks(count, compute_units, mutate)
    span = lambda b: (b * per, count if ((count - b * per) & U64) < per else b * per + per)  # noqa: E731
    base = [0] * (blocks + 1)
    for b in range(blocks):                                   # offsetsBlockTotal
        first, end = span(b)
        base[b] = sum(at(k) for k in range(first, end))
    carry = 0
    for lo in range(0, blocks, SCAN_STEP):                    # pfac_array_scan: `carry` in front of each step of 1024
        step = base[lo:min(lo + SCAN_STEP, blocks)]
        run = carry
        for i, x in enumerate(step):
            base[lo + i] = run
            run += x
        carry = run
    base[blocks] = carry
    off = [0] * count
    for b in range(blocks):                                   # offsetsOfBlock
        first, end = span(b)
        run = base[b]
        for k in range(first, end):
            if 0 <= k < count:
                off[k] = run
            run += at(k)
    return off, base[blocks]


def tile_model(data, start, length, mis_out, capacity, compute_units, mutate=None):
    """pfac_lines_gather_copy behind the three offset launches, line by line of the kernel -> the `capacity` bytes of d_out as bytes, FILL
    where nothing is written.  mutate: a key of MUTANTS.  Every read of data, start, length, off and rel is checked: outside, it reads 0"""
    assert mutate is None or mutate in MUTANTS
    data = as_array(data)
    n, count = int(data.size), int(len(start))
    if capacity is None:
        capacity = gather_total(n, start, length)
    off, total = model_offsets(n, start, length, compute_units, mutate)
    s_all, e_all = clamped(n, start, length)
    s_all, l_all = s_all.tolist(), (e_all - s_all).tolist()
    byte_at = data.tolist()
    out = bytearray([FILL]) * capacity
    if capacity == 0:
        return bytes(out)
    limit = min(total, capacity)
    grid = copy_grid(n, count, capacity, mis_out, compute_units)
    off_at = lambda i: off[i] if 0 <= i < count else 0  # noqa: E731
    line_of = lambda i: (s_all[i], l_all[i]) if 0 <= i < count else (0, 0)  # noqa: E731
    cap = TILE - 1 if mutate == "cap_minus_1" else TILE
    for block in range(grid):
        v_lo = block * TILE
        while v_lo < limit + mis_out:
            o_lo = v_lo - mis_out if v_lo > mis_out else 0                       # tileFrame
            o_hi = min(v_lo + TILE - mis_out, limit)
            lo, hi = 0, count                                                    # t == 0
            while hi - lo > 1:
                mid = lo + (hi - lo) // 2
                if (off_at(mid) < o_lo) if mutate == "first_lt" else (off_at(mid) <= o_lo + (mutate == "first_le_plus_1")):
                    lo = mid
                else:
                    hi = mid
            lo2, hi2 = lo, count
            while hi2 - lo2 > 1:
                mid = lo2 + (hi2 - lo2) // 2
                if (off_at(mid) <= o_hi) if mutate == "last_le" else (off_at(mid) < o_hi - (STEP if mutate == "last_lt_minus_16" else 0)):
                    lo2 = mid
                else:
                    hi2 = mid
            first = lo
            cnt = min(lo2 - lo + 1, cap)
            rel = [0] + [(off_at(first + j) - o_lo) & 0xFFFFFFFF for j in range(1, cnt)]
            for t in range(THREADS):
                v0 = v_lo + STEP * t
                c_lo = v0 - mis_out if v0 > mis_out else 0
                c_hi = min(v0 + STEP - mis_out, o_hi) if v0 + STEP > mis_out else 0
                nb = c_hi - c_lo if c_lo < c_hi else 0
                if nb == 0:
                    continue
                r = c_lo - o_lo
                lo, hi = 0, cnt
                while hi - lo > 1:
                    mid = (lo + hi) // 2
                    if (rel[mid] < r) if mutate == "rel_lt" else (rel[mid] <= r):
                        lo = mid
                    else:
                        hi = mid
                i = first + lo
                if lo == 0:
                    k = r if mutate == "k_from_tile" else (c_lo - off_at(first)) & U64
                else:
                    k = (r - rel[lo]) & 0xFFFFFFFF
                s, ln = line_of(i)
                for b in range(nb):                                               # next()
                    if k < ln:
                        byte = byte_at[s + k] if 0 <= s + k < n else 0
                        k += 1
                    else:
                        byte = NL
                        k = 0
                        i += 1
                        ln = line_of(i)[1] if i < count else 0
                        s = line_of(i)[0] if i < count else s
                    if 0 <= c_lo + b < capacity:
                        out[c_lo + b] = byte
            v_lo += grid * TILE
            if mutate == "no_second_trip":
                break
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------------- cases and claims

class Case(tuple):
    """(name, data, start, length, in_offset, out_offset, capacity or None) and, beside the tuple, .claims"""

    def __new__(cls, name, data, start, length, in_offset=0, out_offset=0, capacity=None, claims=()):
        self = super().__new__(cls, (name, as_array(data), np.ascontiguousarray(start, dtype=np.int32), np.ascontiguousarray(length, dtype=np.int32),
                                     int(in_offset), int(out_offset), capacity))
        self.claims = tuple(claims)
        return self

    name = property(lambda self: self[0])

    def total(self):
        return gather_total(int(self[1].size), self[2], self[3])

    def limit(self):
        return self.total() if self[6] is None else min(self.total(), self[6])


def tile_bounds(tile, mis, limit):
    """output bytes [oLo, oHi) of tile `tile`: tiles are cut on the output ADDRESS, v = o + mis"""
    return (tile * TILE - mis if tile else 0), min(tile * TILE + TILE - mis, limit)


def last_tile(mis, limit):
    return (limit + mis - 1) // TILE


def check_claims(case, compute_units):
    """every claim of the case from the definition of the text: offsets by cumsum of the clamped lengths, tiles from out_offset"""
    name, data, start, length, _, mis, capacity = case
    n, count = int(data.size), int(start.size)
    off, total = offsets(n, start, length)
    s, e = clamped(n, start, length)
    limit = case.limit()
    assert case.claims, name
    for claim in case.claims:
        kind, args = claim[0], claim[1:]
        if kind in ("start", "nonempty_start"):                # a line starts `delta` bytes from the tile's oLo / oHi; tile -1: the last
            tile, where, delta = args
            tile = last_tile(mis, limit) if tile < 0 else tile
            assert 0 < tile <= last_tile(mis, limit), claim
            at = tile_bounds(tile, mis, limit)[where == "oHi"] + delta
            hit = np.flatnonzero(off == at)
            assert hit.size == 1, (name, claim)
            assert kind == "start" or e[hit[0]] > s[hit[0]], (name, claim)
        elif kind == "newline":                               # the tile's first / last byte is a line's '\n'
            tile, where = args
            o_lo, o_hi = tile_bounds(tile, mis, limit)
            at = o_lo if where == "first" else o_hi - 1
            assert np.any(off + (e - s) == at), (name, claim)
        elif kind == "stages":                                # sCount before the cap: the line at or in front of oLo and the starts inside (oLo, oHi)
            tile, want = args
            o_lo, o_hi = tile_bounds(tile, mis, limit)
            assert 1 + int(np.count_nonzero((off > o_lo) & (off < o_hi))) == want, (name, claim)
        elif kind == "starts_in":
            tile, want = args
            o_lo, o_hi = tile_bounds(tile, mis, limit)
            assert int(np.count_nonzero((off >= o_lo) & (off < o_hi))) == want, (name, claim)
        elif kind == "line_newline_at_byte":                  # the '\n' of a line that is not empty is byte b of some thread's 16
            at = (off + (e - s))[e > s]
            assert np.any((at + mis) % STEP == args[0]), (name, claim)
        elif kind == "sixteen_newlines":                      # some thread's 16 bytes are 16 lines
            text = gather_text(data, start, length)
            own = np.flatnonzero(text == NL)
            run = np.zeros(total + 1, dtype=np.int64)
            run[own + 1] = 1
            run = np.cumsum(run)
            v0 = np.arange(-mis % STEP, total - STEP + 1, STEP)
            assert v0.size and np.any(run[v0 + STEP] - run[v0] == STEP), (name, claim)
        elif kind == "ends_mid_thread":
            assert capacity == total and (total + mis) % STEP != 0, (name, claim)
        elif kind == "capacity_is_total":
            assert capacity == total == args[0], (name, claim)
        elif kind == "lines":
            assert count == args[0], (name, claim)
        elif kind == "cut":                                   # offsetBlocks: (blocks, per), stated by hand
            assert offset_blocks(count, compute_units) == args, (name, claim, offset_blocks(count, compute_units))
        elif kind == "per_one_line_fewer":
            assert offset_blocks(count - 1, compute_units)[1] == args[0] != offset_blocks(count, compute_units)[1], (name, claim)
        elif kind == "scan_steps":                            # pfac_array_scan walks the block totals in this many steps of 1024
            assert (offset_blocks(count, compute_units)[0] + SCAN_STEP - 1) // SCAN_STEP == args[0], (name, claim)
        elif kind == "tiles_past_one_pass":
            tiles = (limit + mis + TILE - 1) // TILE
            assert tiles > TILE_BLOCKS_PER_CU * compute_units == copy_grid(n, count, limit, mis, compute_units), (name, claim)
        elif kind == "total":
            assert total == args[0], (name, claim)
        elif kind == "truncated":
            assert capacity is not None and capacity < total, (name, claim)
        elif kind == "descending":
            assert np.all(np.diff(start.astype(np.int64)) < 0) and np.all(e > s), (name, claim)
        elif kind == "overlapping":
            assert np.all(s[1:] < e[:-1]) and np.all(s[1:] > s[:-1]), (name, claim)
        elif kind == "repeated":
            assert count == args[0] and np.all(start == start[0]) and np.all(length == length[0]) and e[0] > s[0], (name, claim)
        elif kind == "hostile":
            assert np.any(start < 0) and np.any(start > n) and np.any(length < 0) and np.any(length.astype(np.int64) + start > n), (name, claim)
            assert {INT_MAX, INT_MIN} <= set(start.tolist()) and {INT_MAX, INT_MIN} <= set(length.tolist()), (name, claim)
        elif kind == "last_ends_at_n":
            assert e[-1] == n and s[-1] < n, (name, claim)
        elif kind == "start_is_n":
            assert np.any(start == n), (name, claim)
        else:
            raise AssertionError("unknown claim %r" % (claim,))


def payload(n, seed):
    """n printable bytes, no '\\n' among them"""
    return np.random.Generator(np.random.PCG64(seed)).integers(33, 127, size=n, dtype=np.uint8)


def lines_of(lengths, n):
    """(start, length): line i of the given length somewhere in [0, n), another place for each"""
    lengths = np.asarray(lengths, dtype=np.int64)
    assert lengths.size and lengths.max() <= n and lengths.min() >= 0
    return (np.arange(lengths.size, dtype=np.int64) * 37 + 11) % (n - lengths + 1), lengths


def lengths_through(*marks):
    """line lengths of 20 .. 116 bytes whose text has a line start at each of the ascending `marks`; the last mark is the size of the text"""
    out, at = [], 0
    for to in marks:
        assert to > at
        while to - at > 130:
            out.append(20 + (len(out) * 29) % 97)
            at += out[-1] + 1
        out.append(to - at - 1)
        at = to
    return out


# ---------------------------------------------------------------------------------------------------------------- A: the two searches of a tile

A_OFFSETS = (0, 1, 15)
A_TOTAL = 3 * TILE + 1000               # tiles 0 .. 3; tile 1 is whole, tile 3 the last
A_PLACES = ((1, "oLo", -1), (1, "oLo", 0), (1, "oLo", 1), (1, "oHi", -1), (1, "oHi", 0), (1, "oHi", -STEP), (1, "oHi", 1 - STEP),
            (-1, "oLo", -1), (-1, "oLo", 0), (-1, "oLo", 1), (-1, "oHi", -1))       # the last tile's oHi is the end of the text: no line starts there


def tile_searches():
    """FAMILY A.  off[mid] <= oLo and off[mid] < oHi with a start on, in front of and behind either bound; the '\\n' in front of a start on
    oHi is the tile's last byte, the one in front of a start on oLo + 1 its first"""
    data = payload(3 * TILE, 1)
    out = []
    for mis in A_OFFSETS:
        for tile, where, delta in A_PLACES:
            number = last_tile(mis, A_TOTAL) if tile < 0 else tile
            assert number == (3 if tile < 0 else 1)
            at = tile_bounds(number, mis, A_TOTAL)[where == "oHi"] + delta
            start, length = lines_of(lengths_through(at, A_TOTAL), data.size)
            claims = [("start", tile, where, delta), ("total", A_TOTAL)]
            if (where, delta) == ("oHi", 0):
                claims.append(("newline", number, "last"))
            if (where, delta) == ("oLo", 1):
                claims.append(("newline", number, "first"))
            name = "A-out%d-%s-%s%+d" % (mis, "last" if tile < 0 else "tile1", where, delta)
            out.append(Case(name, data, start, length, 0, mis, None, claims))
    return out


# ---------------------------------------------------------------------------------------------------------------- B: the staging of a tile

B_OFFSETS = (0, 7)


def b_full(data, mis, shift, empties):
    """a line that ends `shift` bytes into tile 1, `empties` empty lines, a line of 50 bytes, three short ones"""
    o_lo = TILE - mis
    return lines_of([o_lo + shift - 1] + [0] * empties + [50, 7, 0, 12], data.size)


def staging():
    """FAMILY B.  sCount <= kOutTile and rel[]: tiles with 4096 staged offsets, and a tile with one"""
    data = payload(3 * TILE, 2)
    out = []
    for mis in B_OFFSETS:
        zeros = np.zeros(2 * TILE + 5, dtype=np.int64)
        out.append(Case("B-out%d-empty-lines" % mis, data, zeros, zeros, 0, mis, None,
                        [("stages", 1, TILE), ("starts_in", 1, TILE), ("starts_in", 0, TILE - mis), ("total", 2 * TILE + 5)]))
        # 4095 empty lines from oLo on and a line of 50 bytes whose first byte is the tile's last: 4096 starts, the first of them on oLo
        out.append(Case("B-out%d-4096-starts" % mis, data, *b_full(data, mis, 0, TILE - 1), 0, mis, None,
                        [("starts_in", 1, TILE), ("stages", 1, TILE), ("start", 1, "oLo", 0), ("nonempty_start", 1, "oHi", -1)]))
        # the same one byte later: 4095 starts in the tile behind a line that began in tile 0 -- 4096 staged --, the line of 50 bytes on oHi
        out.append(Case("B-out%d-4095-starts-line-on-oHi" % mis, data, *b_full(data, mis, 1, TILE - 1), 0, mis, None,
                        [("starts_in", 1, TILE - 1), ("stages", 1, TILE), ("start", 1, "oLo", 1), ("nonempty_start", 1, "oHi", 0)]))
        # ... and with one empty line fewer: the line of 50 bytes is the 4096th staged offset
        out.append(Case("B-out%d-4095-starts" % mis, data, *b_full(data, mis, 1, TILE - 2), 0, mis, None,
                        [("starts_in", 1, TILE - 1), ("stages", 1, TILE), ("nonempty_start", 1, "oHi", -1)]))
        # one line of 2 TILE + 100 bytes between short ones: tile 1 lies inside it -- cnt == 1, every thread starts cLo - off[first] bytes into it
        out.append(Case("B-out%d-long-line" % mis, data, *lines_of([5, 0, 17, 2 * TILE + 100, 3, 0, 9], data.size), 0, mis, None,
                        [("stages", 1, 1), ("starts_in", 1, 0)]))
    return out


# ---------------------------------------------------------------------------------------------------------------- C: a thread's 16 bytes

C_RUNS = (15, 16, 17, 33)
C_TOTALS = (1, 15, 16, 17, TILE - 1, TILE + 1, 2 * TILE + 5)
C_END_OFFSETS = (0, 9)


def c_run_lengths():
    out = []
    for j in range(80):
        out += [1 + j % 40] + [0] * C_RUNS[j % 4]
    return out


def c_end_lengths(total):
    """lines that make `total` bytes of text: 40 of about equal length where total admits 40, else lengths 0 .. 3"""
    if total < 40:
        out, rest = [], total
        while rest:
            out.append(min((len(out) * 3) % 4, rest - 1))
            rest -= out[-1] + 1
        return out
    base = (total - 40) // 40
    out = [base] * 39 + [total - 40 - 39 * base]
    if base:
        for j in range(19):
            out[2 * j] += 1
            out[2 * j + 1] -= 1
    return out


def thread_steps():
    """FAMILY C.  next(): sixteen line changes in one thread, a line's '\\n' as a thread's last and as its first byte at every out_offset;
    a list that ends inside a thread's 16 bytes, capacity == the text"""
    data = payload(TILE, 3)
    out = []
    start, length = lines_of(c_run_lengths(), data.size)
    for mis in range(STEP):
        out.append(Case("C-out%d-runs" % mis, data, start, length, 0, mis, None,
                        [("line_newline_at_byte", 0), ("line_newline_at_byte", STEP - 1), ("sixteen_newlines",)]))
    for total in C_TOTALS:
        lengths = c_end_lengths(total)
        for mis in C_END_OFFSETS:
            claims = [("capacity_is_total", total), ("lines", min(total, 40) if total >= 40 else len(lengths))]
            if (total + mis) % STEP:
                claims.append(("ends_mid_thread",))
            out.append(Case("C-out%d-total%d" % (mis, total), data, *lines_of(lengths, data.size), 0, mis, total, claims))
    return out


# ---------------------------------------------------------------------------------------------------------------- D: the cut of the offset passes

def d_counts(compute_units):
    """name -> (lines, (blocks, per) by hand)"""
    c = int(compute_units)
    full = BLOCKS_PER_CU * c * THREADS
    return {"255": (255, (1, 256)), "256": (256, (1, 256)), "257": (257, (2, 256)), "513": (513, (3, 256)),
            "full-1": (full - 1, (8 * c, 256)), "full": (full, (8 * c, 256)), "full+1": (full + 1, (4 * c + 1, 512))}


D_NAMES = tuple("D-" + k for k in d_counts(1))


def offset_cuts(compute_units):
    """FAMILY D.  line i has (i * 7) % 5 bytes somewhere in 4 KiB: a wrong base of one block moves every line behind it"""
    data = payload(TILE + 3, 4)
    out = []
    for key, (count, cut) in d_counts(compute_units).items():
        i = np.arange(count, dtype=np.int64)
        claims = [("lines", count), ("cut", *cut), ("scan_steps", (cut[0] + SCAN_STEP - 1) // SCAN_STEP)]
        if key == "full+1":
            claims.append(("per_one_line_fewer", 256))
        out.append(Case("D-" + key, data, (i * 13) % (data.size - 4), (i * 7) % 5, 0, 5 if key == "full+1" else 0, None, claims))
    return out


# ---------------------------------------------------------------------------------------------------------------- E: grid passes, 2^32

E_INPUT = 65535
E_NAMES = ("E-past-one-pass", "E-2^32-capacity0", "E-2^32-capacity%d" % TILE)


def e_pass_lines(compute_units):
    return TILE_BLOCKS_PER_CU * int(compute_units) * TILE // (E_INPUT + 1) + 8


def grid_passes(compute_units):
    """FAMILY E.  every line is the whole input of 65535 bytes, 65536 bytes of text: 8 lines more than one pass of the copy's grid writes;
    and 65536 of them, 2^32 bytes, into no room and into one tile"""
    data = payload(E_INPUT, 5)
    many = e_pass_lines(compute_units)
    out = [Case(E_NAMES[0], data, np.zeros(many), np.full(many, E_INPUT), 0, 3, None,
                [("lines", many), ("total", many << 16), ("tiles_past_one_pass",)])]
    for name, capacity in zip(E_NAMES[1:], (0, TILE)):
        out.append(Case(name, data, np.zeros(1 << 16), np.full(1 << 16, E_INPUT), 0, 0, capacity, [("total", 1 << 32), ("truncated",)]))
    return out


# ---------------------------------------------------------------------------------------------------------------- F: list order

F_INPUT = 2 * TILE
F_OFFSETS = (0, 11)
F_CAPACITIES = (0, 100, None)


def f_lists():
    """name -> (start, length, claim)"""
    n = F_INPUT
    down = np.arange(n - 40, 0, -37)
    over = np.arange(0, 3000, 10)
    hostile_start = [-7, -1, -INT_MAX, INT_MIN, n, n + 1, INT_MAX, n - 2, 5, 100, 200, 0, n - 1, 300]
    hostile_len = [3, 100, INT_MAX, 5, 1, 5, INT_MAX, INT_MAX, INT_MIN, -1, 0, INT_MAX, 2, 7]
    return {"descending": (down, 5 + np.arange(down.size) % 30, ("descending",)),
            "overlapping": (over, np.full(over.size, 100), ("overlapping",)),
            "the-same-3000-times": (np.full(3000, 5), np.full(3000, 9), ("repeated", 3000)),
            "hostile": (hostile_start, hostile_len, ("hostile",))}


def list_orders():
    """FAMILY F.  "in list order": the text of a list that is not ascending, and of one that means harm, is the clamped reference's"""
    data = payload(F_INPUT, 6)
    out = []
    for what, (start, length, claim) in f_lists().items():
        for capacity in F_CAPACITIES:
            for mis in F_OFFSETS:
                claims = [claim] + ([("truncated",)] if capacity is not None else [])
                out.append(Case("F-out%d-%s-capacity-%s" % (mis, what, "full" if capacity is None else capacity), data, start, length, mis // 2, mis,
                                capacity, claims))
    return out


# ---------------------------------------------------------------------------------------------------------------- G: the end of the input

G_INPUT = 1531


def input_edges():
    """FAMILY G.  the input's last byte is the last byte the device holds: a line that ends at n, a line that starts at n, the pointer at
    every offset from a 16-byte boundary"""
    n = G_INPUT
    data = payload(n, 7)
    start = [0, n - 40, n, n - 1, 100, n - 16, n, n - 33]
    length = [10, 40, 5, 1, 0, 16, 0, 33]
    return [Case("G-in%d" % mis, data, start, length, mis, (mis * 3) % STEP, None, [("last_ends_at_n",), ("start_is_n",)]) for mis in range(STEP)]


# ---------------------------------------------------------------------------------------------------------------- all of them

def families(compute_units):
    return {"A": tile_searches(), "B": staging(), "C": thread_steps(), "D": offset_cuts(compute_units), "E": grid_passes(compute_units),
            "F": list_orders(), "G": input_edges()}


def by_name(cases):
    out = {c[0]: c for c in cases}
    assert len(out) == len(cases), "case names are unique"
    return out


NAMES = {family: tuple(c[0] for c in cases) for family, cases in families(1).items()}      # the names do not depend on the device
