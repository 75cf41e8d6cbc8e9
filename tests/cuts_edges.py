"""The cases of tests/test_cuts_edges_host.py and tests/test_cuts_edges_gpu.py, and their model: PFACX_locate* and PFACX_capture* (scan_locate.hip,
scan_capture.hip, scan_cuts.h) past one pass of a grid over the tiles, past one pass of the mark kernels over the list, over three steps of
pfac_locate_carry, with slow pairs in several tiles of one block, and at the top of the 32-bit range.

The launch shapes the cases are built around (each builder takes `grid`, the blocks of a pass: 8 per compute unit of the device it runs on):

    tile_grid(grid, tiles)     scan_cuts.h: tileGrid -- pfac_split_count, pfac_locate_pairs, pfac_capture_pairs: block k takes tiles k, k + grid, ...
    mark_pass(grid)            scan_passes.h: gridFor -- pfac_locate_mark, pfac_capture_mark: thread j takes pairs j, j + 256 grid, ...
    STEP                       pfac_locate_carry: tiles [0, 1024), [1024, 2048), ... a step each, the last cut carried from step to step

THE MODEL never calls the library and never walks a byte: a text is a class index (ClassIndex: the sorted positions of a class's bytes, or of the
bytes outside it, whichever are fewer), every question a searchsorted.  model_locate states scan_cuts.h's rule in its a / b form; model_capture the
six rules of include/pfac_ext.h and, for the slow count, the statement in scan_capture.hip's header.  A text is a Text: a fill byte and special
bytes.  Families A to D make it dense (Text.dense) and index the array; family E, 2 GiB, is indexed from the special bytes alone.

Every case carries CLAIMS, (kind, args) tuples that claim_holds() re-derives from the case's own text and list for the grid it was built with:
that is how a test asserts that the case still reaches its edge on the device it runs on.
"""
import ctypes as C

import numpy as np

from pfac_amd import api

T = api.PFACX_SPLIT_TILE
R = api.PFACX_CAPTURE_REACH
STEP = api.PFACX_LOCATE_CARRY_STEP
MARK_BLOCK = api.PFACX_PAIRS_MARK_BLOCK
PER_CU = api.PFACX_GRID_BLOCKS_PER_CU
BEFORE, RUNS, AT_POS = api.PFACX_SPLIT_BEFORE, api.PFACX_SPLIT_RUNS, api.PFACX_CAPTURE_AT_POS
ALL_FLAGS = (0, BEFORE, RUNS, BEFORE | RUNS)
INT_MAX = (1 << 31) - 1

KEYS = [b"k=", b"key:", b"longerkey=", b"q" * (R + 76)]                    # ids 1 .. 4; the last is longer than the reach
PATTERNS = b"".join(k + b"\n" for k in KEYS)
LENS = np.asarray([0] + [len(k) for k in KEYS], dtype=np.int32)            # by id; numLens = 5
X, NL, SEMI, BLANK = ord("x"), ord("\n"), ord(";"), ord(" ")

ONE, TABLE = b"\n", b"\n;"                                                 # a class of one member (SINGLE) and one that goes through the table in LDS


def tile_grid(grid, tiles):
    return min(tiles, grid)


def mark_pass(grid):
    """the pairs one pass of a mark kernel takes when the list is longer than that"""
    return MARK_BLOCK * grid


# --------------------------------------------------------------------------------------------------------------------------- texts

class Text:
    """n bytes: `fill` but for the special bytes put() names (a later put wins)"""

    def __init__(self, n, fill=X):
        self.n, self.fill, self._at, self._by, self._dense, self._index = int(n), fill, [], [], None, {}

    def put(self, at, byte):
        at = np.atleast_1d(np.asarray(at, dtype=np.int64))
        at = at[(at >= 0) & (at < self.n)]
        self._at.append(at)
        self._by.append(np.full(at.size, byte, dtype=np.uint8))
        self._dense, self._index = None, {}
        return self

    def sparse(self):
        """-> (the special positions, ascending and unique; their bytes)"""
        if not self._at:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint8)
        at, by = np.concatenate(self._at)[::-1], np.concatenate(self._by)[::-1]
        at, first = np.unique(at, return_index=True)
        return at, by[first]

    def dense(self):
        if self._dense is None:
            data = np.full(self.n, self.fill, dtype=np.uint8)
            for at, by in zip(self._at, self._by):
                data[at] = by
            self._dense = data
        return self._dense


def class_table(cls, default=b""):
    table = np.zeros(256, dtype=bool)
    members = default if cls is None else bytes(cls)
    if len(members):
        table[np.frombuffer(members, dtype=np.uint8)] = True
    return table


class ClassIndex:
    """where the bytes of a class lie in a text of n bytes: `members` ascending -- the positions inside the class, or, `inverted`, those outside"""

    def __init__(self, n, members, inverted):
        self.n, self.members, self.inverted = int(n), members.astype(np.int64), inverted
        if inverted and members.size:                                      # the first position behind the run of neighbours that holds members[i]
            last = np.flatnonzero(np.append(np.diff(self.members) != 1, True))
            run = np.searchsorted(last, np.arange(self.members.size), side="left")
            self.behind = self.members[last[run]] + 1

    def first_from(self, x):
        """the first position >= x inside the class, n where there is none; x: int64 array of [0, n]"""
        m = self.members
        if m.size == 0:
            return x.copy() if self.inverted else np.full(x.shape, self.n, dtype=np.int64)
        k = np.searchsorted(m, x, side="left")
        kk = np.minimum(k, m.size - 1)
        if self.inverted:
            return np.minimum(np.where((k < m.size) & (m[kk] == x), self.behind[kk], x), self.n)
        return np.where(k < m.size, m[kk], self.n)

    def positions(self):
        assert not self.inverted, "a class that holds most of the text: no case cuts by one"
        return self.members


def index_of(text, table, dense):
    """the ClassIndex of a Text: from the array (`dense`) or from the special bytes alone; made once per class"""
    key = (table.tobytes(), dense)
    if key not in text._index:
        if dense:
            mask = table[text.dense()]
            inverted = 2 * int(np.count_nonzero(mask)) > text.n
            text._index[key] = ClassIndex(text.n, np.flatnonzero(~mask if inverted else mask), inverted)
        else:
            at, by = text.sparse()
            inverted = bool(table[text.fill])
            text._index[key] = ClassIndex(text.n, at[~table[by]] if inverted else at[table[by]], inverted)
    return text._index[key]


# --------------------------------------------------------------------------------------------------------------------------- the model

def model_cuts(text, cls, flags, dense=True):
    """scan_cuts.h: position c of [1, n - 1] is a cut if, with a = (in[c - 1] in D) and b = (in[c] in D) --
    flags 0: a; BEFORE: b; RUNS: a and not b; both: b and not a"""
    d = index_of(text, class_table(cls, b"\n"), dense).positions()
    if flags & RUNS:
        lone = np.ones(d.size, dtype=bool)
        if flags & BEFORE:
            lone[1:] = d[1:] != d[:-1] + 1                                 # b and not a
            c = d[lone]
        else:
            lone[:-1] = d[:-1] + 1 != d[1:]                                # a and not b
            c = d[lone] + 1
    else:
        c = d if flags & BEFORE else d + 1
    return c[(c >= 1) & (c <= text.n - 1)]


def model_locate(text, positions, cls, flags, dense=True):
    """-> (record, column as int32, the number of records)"""
    c = model_cuts(text, cls, flags, dense)
    p = np.asarray(positions, dtype=np.int64)
    inside = (p >= 0) & (p < text.n)
    r = np.searchsorted(c, p, side="right")
    start = np.where(r > 0, c[np.maximum(r, 1) - 1], 0) if c.size else np.zeros(p.size, dtype=np.int64)
    return np.where(inside, r, -1).astype(np.int32), np.where(inside, p - start, -1).astype(np.int32), int(c.size) + 1


def model_capture(text, ids, positions, skip, stop, window, flags, lens=LENS, dense=True):
    """-> (valStart, valLen as int32, slow: which pairs leave the bitmaps of their tile)"""
    n = text.n
    D = class_table(stop, b"\n")
    S = class_table(skip) & ~D
    go, d = index_of(text, ~S, dense), index_of(text, D, dense)
    p = np.asarray(positions, dtype=np.int64)
    ok = (p >= 0) & (p < n)                                                # rule 1
    b = p.copy()
    if not flags & AT_POS:
        i = np.asarray(ids, dtype=np.int64)
        has = (i >= 1) & (i < len(lens))
        ok &= has
        b = p + np.maximum(np.asarray(lens, dtype=np.int64)[np.where(has, i, 0)], 0)   # rule 2
    b = np.clip(b, 0, n)
    w = np.full(p.size, n, dtype=np.int64) if window == 0 else np.minimum(n, b + window)  # rule 3
    s = np.minimum(go.first_from(b), w)                                    # rule 4
    e = np.minimum(d.first_from(s), w)                                     # rule 5
    hi = np.clip(p, 0, n) // T * T + T + R                                 # scan_capture.hip: the bitmaps of the pair's tile answer up to here
    map_end = np.minimum(w, hi)
    unanswered = map_end < w
    slow = ok & (((b >= hi) & (b < w)) | ((b < hi) & (s >= map_end) & unanswered) | ((s >= hi) & (s < w)) | ((s < hi) & (e >= map_end) & unanswered))
    return np.where(ok, s, -1).astype(np.int32), np.where(ok, e - s, 0).astype(np.int32), slow


# --------------------------------------------------------------------------------------------------------------------------- cases

class Case:
    """a text, a list (pos, ids: None for a list that is only located or captured at the position), the calls to make of it and its claims"""

    def __init__(self, name, grid, text, pos, ids=None, locate=(), capture=(), claims=(), dense=True):
        self.name, self.grid, self.text, self.dense = name, grid, text, dense
        self.pos = np.ascontiguousarray(pos, dtype=np.int64).astype(np.int32)
        self.ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
        self.locate = list(locate)                                         # (cls, flags)
        self.capture = list(capture)                                       # (skip, stop, window, flags)
        self.claims = list(claims)
        self._want = {}
        self.n, self.tiles = text.n, (text.n - 1) // T + 1
        assert self.ids is None or self.ids.size == self.pos.size
        inside = self.pos[(self.pos >= 0) & (self.pos < self.n)]
        assert np.all(np.diff(inside.astype(np.int64)) >= 0) and np.all(np.diff(self.pos.astype(np.int64)) >= 0), "a non-decreasing list"

    def want_locate(self, cls, flags):
        """the model's answer, computed once and never changed"""
        if (cls, flags) not in self._want:
            self._want[(cls, flags)] = model_locate(self.text, self.pos, cls, flags, self.dense)
        return self._want[(cls, flags)]

    def want_capture(self, skip, stop, window, flags):
        if (skip, stop, window, flags) not in self._want:
            self._want[(skip, stop, window, flags)] = model_capture(self.text, self.ids, self.pos, skip, stop, window, flags, LENS, self.dense)
        return self._want[(skip, stop, window, flags)]


def pairs_in(case, tile):
    return np.flatnonzero((case.pos >= 0) & (case.pos < case.n) & (case.pos // T == tile))


def claim_holds(case, claim):
    kind, a = claim[0], claim[1:]
    grid, pos = case.grid, case.pos
    if kind == "tiles":                                                    # (tiles, bytes of the last)
        return case.tiles == a[0] and case.n - (case.tiles - 1) * T == a[1] and case.tiles > grid
    if kind == "same block":                                               # (tile, later tile, pairs in the first, in the second)
        return (a[0] % grid == a[1] % grid and a[1] // grid > a[0] // grid and a[1] < case.tiles and (pairs_in(case, a[0]).size > 0) == a[2]
                and (pairs_in(case, a[1]).size > 0) == a[3])
    if kind == "delimiters":                                               # (tile, "all" | "none" | "some", class)
        at = case.text.dense()[a[0] * T:(a[0] + 1) * T]
        hits = int(np.count_nonzero(class_table(a[2])[at]))
        return {"all": hits == at.size, "none": hits == 0, "some": 0 < hits < at.size}[a[1]]
    if kind == "pair at":                                                  # (position)
        return bool(np.any(pos == a[0]))
    if kind == "second pass":                                              # (index, "outside" | "inside" | "no such id")
        i = a[0]
        if not mark_pass(grid) <= i < pos.size:
            return False
        inside = 0 <= pos[i] < case.n
        return {"outside": not inside, "inside": inside, "no such id": inside and case.ids is not None and not 1 <= case.ids[i] < len(LENS)}[a[1]]
    if kind == "first pair in the second pass":                            # (tile)
        at = pairs_in(case, a[0])
        return at.size > 0 and at[0] >= mark_pass(grid)
    if kind == "first entry outside":
        return not 0 <= pos[0] < case.n
    if kind == "steps with a cut":                                         # (class, flags, one bool per carry step)
        c = model_cuts(case.text, a[0], a[1], case.dense)
        steps = (case.tiles - 1) // a[3] + 1
        return tuple(bool(np.any(c // T // a[3] == s)) for s in range(steps)) == tuple(a[2])
    if kind == "cut at":                                                   # (class, flags, position)
        return bool(np.any(model_cuts(case.text, a[0], a[1], case.dense) == a[2]))
    if kind == "pairs in step":                                            # (step, tiles a step)
        inside = pos[(pos >= 0) & (pos < case.n)]
        return bool(np.any(inside // T // a[1] == a[0]))
    if kind == "slow":                                                     # (tile, the call, slow pairs, fast pairs): exactly
        slow = case.want_capture(*a[1])[2]
        at = pairs_in(case, a[0])
        return int(np.count_nonzero(slow[at])) == a[2] and int(at.size - np.count_nonzero(slow[at])) == a[3]
    if kind == "n":
        return case.n == a[0]
    raise AssertionError(kind)


def check_claims(case):
    for claim in case.claims:
        assert claim_holds(case, claim), (case.name, case.grid, claim)


def a_tiles(grid):
    """more tiles than one pass of the grid and than two steps of the one-block passes"""
    return max(grid, 2 * STEP) + 3


def _sprinkle(text, rng, tile, every, byte, runs=0):
    lo = tile * T
    text.put(lo + rng.integers(0, T, size=max(1, T // every)), byte)
    for start in rng.integers(0, T - 8, size=runs):
        text.put(lo + int(start) + np.arange(int(rng.integers(2, 7))), byte)


def _pairs(rng, tile, count, n):
    lo = tile * T
    hi = min(lo + T, n)
    return np.concatenate([[lo, hi - 1], rng.integers(lo, hi, size=count)])  # the first and the last byte of the tile among them


A_VARIANTS = {0: ("both", "first"), 1: ("second", "all-none"), 2: ("none-all", "both")}
A_CALLS = {                                                                 # locate: all four flag combinations on one case, two on the rest
    0: [(ONE, f) for f in ALL_FLAGS] + [(TABLE, 0), (TABLE, RUNS | BEFORE)],
    1: [(ONE, 0), (ONE, RUNS), (TABLE, BEFORE), (TABLE, RUNS | BEFORE)],
    2: [(ONE, BEFORE), (ONE, RUNS | BEFORE), (TABLE, 0), (TABLE, RUNS)],
}


def tiles_beyond_a_pass(grid, variant, tiles=None):
    """FAMILY A.  Two blocks whose first two tiles pair up as A_VARIANTS says, and the block of the last tile: a tile full of delimiters and
    pairs, then -- its next trip -- the last tile of 5 bytes"""
    tiles = tiles or a_tiles(grid)
    n = (tiles - 1) * T + 5
    last = tiles - 1
    full = last - grid
    blocks = [k for k in range(grid) if k + grid <= tiles - 2 and full not in (k, k + grid)][:2]
    assert len(blocks) == 2 and full >= 0, "too few tiles for this grid"
    rng = np.random.Generator(np.random.PCG64(1000 + variant))
    text = Text(n)
    pos, claims = [], [("tiles", tiles, 5)]
    for k, kind in zip(blocks, A_VARIANTS[variant]):
        first, second = k, k + grid
        if kind in ("both", "first", "second"):
            _sprinkle(text, rng, first, 40, NL, runs=6)
            _sprinkle(text, rng, first, 300, SEMI)
            _sprinkle(text, rng, first, 25, BLANK, runs=10)
            _sprinkle(text, rng, second, 700, NL, runs=2)                 # other cuts, other classes, in other words of the bitmaps
            _sprinkle(text, rng, second, 90, SEMI, runs=9)
            _sprinkle(text, rng, second, 400, BLANK)
            claims += [("delimiters", first, "some", ONE), ("delimiters", second, "some", ONE)]
        else:
            everywhere, nowhere = (first, second) if kind == "all-none" else (second, first)
            text.put(everywhere * T + np.arange(T), NL)
            _sprinkle(text, rng, nowhere, 30, BLANK, runs=4)
            claims += [("delimiters", everywhere, "all", ONE), ("delimiters", nowhere, "none", TABLE)]
        in_first, in_second = kind != "second", kind != "first"
        if in_first:
            pos.append(_pairs(rng, first, 300, n))
        if in_second:
            pos.append(_pairs(rng, second, 300, n))
            claims += [("pair at", second * T), ("pair at", second * T + T - 1)]
        claims.append(("same block", first, second, in_first, in_second))
    text.put(full * T + np.arange(T), NL)                                  # every bit of its bitmaps set: what the last tile's 5 bytes are written over
    text.put(full * T + np.arange(7, T, 64), SEMI)
    assert full + 1 < last and full + 1 not in [t for k in blocks for t in (k, k + grid)]
    text.put((full + 1) * T + 2000, NL)                                    # a value of the full tile's last bytes ends here, not a grid of tiles on:
    text.put((full + 1) * T + 2001, SEMI)                                  # the slow path is a lane alone
    text.put(last * T + np.asarray([1, 2]), BLANK)
    text.put(last * T + 3, NL)
    pos += [_pairs(rng, full, 500, n), last * T + np.asarray([0, 0, 1, 2, 3, 4, 4])]
    claims += [("same block", full, last, True, True), ("delimiters", full, "all", TABLE), ("pair at", n - 1), ("pair at", last * T)]
    ids = rng.integers(1, 4, size=sum(p.size for p in pos))
    capture = [(b" ", ONE, 0, 0), (b" ", TABLE, 0, AT_POS), (None, ONE, 48, 0), (b" \n", b";", 0, 0)]
    return Case("A%d-%d" % (variant, grid), grid, text, np.sort(np.concatenate(pos)), ids, A_CALLS[variant], capture, claims)


B_KINDS = ("tail", "first-outside", "head", "on-A")


def lists_beyond_a_pass(grid, kind, tiles=None):
    """FAMILY B.  A list of 256 grid + 257 pairs, many at equal positions, over 40 tiles (on-A: over family A's input):
    tail            entries n, n + 1, INT_MAX, ids 0 and numLens and a whole tile's pairs, all at indices of the second pass
    first-outside   the same list with -1 in front
    head            -1 up to an index of the second pass, every pair inside behind them"""
    num = mark_pass(grid) + MARK_BLOCK + 1
    rng = np.random.Generator(np.random.PCG64(2000 + B_KINDS.index(kind)))
    if kind == "on-A":
        a = tiles_beyond_a_pass(grid, 0, tiles)
        text, n = a.text, a.n
        inside = a.pos[(a.pos >= 0) & (a.pos < n)]
        one_a_tile = inside[np.unique(inside // T, return_index=True)[1]]  # every tile of A's list keeps a pair
        pos = np.sort(np.concatenate([one_a_tile, rng.choice(inside, size=num - one_a_tile.size - 3)]))
        pos = np.concatenate([pos, [n, n, INT_MAX]])
        claims = [c for c in a.claims if c[0] in ("tiles", "same block")] + [("second pass", num - 1, "outside"), ("second pass", num - 4, "inside")]
    else:
        tiles = tiles or 40
        n = (tiles - 1) * T + 7777
        text = Text(n)
        for tile in range(tiles):
            _sprinkle(text, rng, tile, 60, NL, runs=2)
            _sprinkle(text, rng, tile, 200, SEMI, runs=1)
            _sprinkle(text, rng, tile, 20, BLANK, runs=3)
        last = tiles - 1
        outside = np.asarray([n, n, n + 1, INT_MAX, INT_MAX])
        in_last = 200
        if kind == "head":
            front = np.full(mark_pass(grid) + 9, -1)
            body = np.sort(rng.integers(0, n, size=num - front.size - outside.size) // 5 * 5)
            claims = [("second pass", mark_pass(grid) + 8, "outside"), ("second pass", mark_pass(grid) + 9, "inside"), ("first entry outside",),
                      ("first pair in the second pass", int(body[0]) // T)]
        else:
            front = np.full(1 if kind == "first-outside" else 0, -1)
            early = np.sort(rng.integers(0, (last - 1) * T, size=num - front.size - outside.size - in_last) // 7 * 7)   # tile last - 1: no pair
            body = np.concatenate([early, np.sort(rng.integers(last * T, n, size=in_last) // 3 * 3)])
            claims = [("first pair in the second pass", last), ("second pass", num - 1, "outside"), ("second pass", num - 5, "outside")]
            claims += [("first entry outside",)] if kind == "first-outside" else []
        pos = np.concatenate([front, body, outside])
    assert pos.size == num
    ids = rng.integers(1, 5, size=num)
    bad = np.flatnonzero((pos >= 0) & (pos < n))
    bad = bad[bad >= mark_pass(grid)][:6]
    ids[bad[0::2]], ids[bad[1::2]] = 0, len(LENS)
    claims += [("second pass", int(bad[0]), "no such id"), ("second pass", int(bad[1]), "no such id")]
    locate = [(ONE, 0), (TABLE, RUNS | BEFORE)]
    capture = [(b" ", ONE, 0, 0), (b" ", TABLE, 0, AT_POS)]
    return Case("B-%s-%d" % (kind, grid), grid, text, pos, ids, locate, capture, claims)


C_KINDS = ("only-cut-in-step-0", "cut-at-the-last-byte-of-step-1", "first-cut-opens-step-2", "no-cut-behind-step-1")


def carry_steps(grid, kind, tiles=None, step=STEP):
    """FAMILY C.  Three steps of pfac_locate_carry (`step`: the tiles of a step; the kernel's is STEP) on family A's tile count"""
    tiles = tiles or a_tiles(grid)
    n = (tiles - 1) * T + 5
    assert 2 * step < tiles <= 3 * step
    text = Text(n)
    edge = 2 * step * T                                                    # the first byte of step 2
    pos = [3, 5 * T // 2, step * T + 9, edge - 1]                          # steps 0 and 1 are asked too
    if kind == "only-cut-in-step-0":
        text.put(T + 100, NL)
        pos += [edge, edge + 1, edge + T + 17, n - 1]
        calls = [(ONE, 0), (TABLE, BEFORE)]
        claims = [("steps with a cut", ONE, 0, (True, False, False), step)]
    elif kind == "cut-at-the-last-byte-of-step-1":
        text.put([edge - 1, 77], NL)
        pos += [edge, edge, edge + 1, edge + 2, n - 1]
        calls = [(ONE, BEFORE), (ONE, 0), (TABLE, RUNS | BEFORE)]          # BEFORE: the cut is step 1's last byte; flags 0: step 2's first
        claims = [("cut at", ONE, BEFORE, edge - 1), ("cut at", ONE, 0, edge), ("steps with a cut", ONE, BEFORE, (True, True, False), step),
                  ("pair at", edge)]
    elif kind == "first-cut-opens-step-2":
        text.put(edge, NL)
        pos += [edge, edge + 1, edge + T, n - 1]
        calls = [(ONE, BEFORE), (ONE, 0), (TABLE, RUNS)]
        claims = [("cut at", ONE, BEFORE, edge), ("steps with a cut", ONE, BEFORE, (False, False, True), step)]
    else:
        text.put([9, step * T + T + 4000, step * T + T + 4001], NL)        # step 1's last cut is carried over a step without one, not step 0's and not 0
        pos += [edge, edge + 5, n - 1]
        calls = [(ONE, 0), (ONE, RUNS), (TABLE, BEFORE)]
        claims = [("steps with a cut", ONE, 0, (True, True, False), step)]
    claims += [("pairs in step", 2, step), ("pairs in step", 0, step)] + ([("tiles", tiles, 5)] if tiles > grid else [])
    return Case("C-%s-%d" % (kind, grid), grid, text, np.sort(np.asarray(pos)), None, calls, [], claims)


D_WINDOWS = (0, 64)


def D_TILES(grid):
    return (0, grid, 1, grid + 1)


def slow_pairs(grid, window, tiles=None):
    """FAMILY D.  Two blocks, in the first two tiles of each the same pairs: slow ones of every kind, fast ones between them.  `lo` the tile's
    first byte, `hi` = lo + T + R the end of its bitmaps, blanks the skip class, ';' the stop class; the first stop byte behind lo + 9000 is hi + 200"""
    tiles = tiles or a_tiles(grid)
    n = (tiles - 1) * T + 5
    assert grid + 1 <= tiles - 2 and window in D_WINDOWS
    text = Text(n)
    call_ids, call_at = (b" ", b";", window, 0), (b" ", b";", window, AT_POS)
    pos, ids, claims = [], [], [("tiles", tiles, 5)]
    for tile in D_TILES(grid):
        lo, hi = tile * T, tile * T + T + R
        text.put(lo + np.arange(6000, 9000, 50), SEMI)                     # the fast zone
        text.put(lo + 6000 + 50 * np.arange(0, 60, 4)[:, None] + np.arange(2, 9), BLANK)
        text.put(hi + 200, SEMI)
        text.put(np.arange(lo + T - 38, hi + 30), BLANK)                   # a skip run through the bitmaps' end
        here = [(1, lo + 6000 + 50 * k) for k in range(0, 60, 7)]          # fast
        here += [(1, lo + T - 500),                                        # b + 64 <= hi: e unanswered without a window, fast with it
                 (2, lo + T - 300),
                 (1, lo + T - 40), (1, lo + T - 40),                       # b on the skip run: s unanswered, then s >= hi
                 (4, lo + T - 10),                                         # b >= hi by the pattern's length
                 (3, lo + T - 10)]
        if window:
            here += [(4, hi - window - int(LENS[4])), (4, hi - window - int(LENS[4]) + 1)]   # by the longest pattern: b + window = hi, and hi + 1
        ids += [i for i, _ in here]
        pos += [p for _, p in here]
    order = np.argsort(np.asarray(pos), kind="stable")
    case = Case("D-%d-%d" % (window, grid), grid, text, np.asarray(pos)[order], np.asarray(ids)[order], [(b";", 0), (b";\n", RUNS)],
                [call_ids, call_at], claims)
    # counted by hand from the list above, (slow, fast) of one tile.  No window: the two that find no stop byte, the two on the skip run and the
    # two at lo + T - 10 are slow under both calls.  Window 64: by ids only the pattern that ends behind hi and the one whose window ends at
    # hi + 1; at the position every window ends inside the bitmaps.  A tile whose bitmaps reach the input's end (on 256 compute units: tile
    # grid + 1) has nothing behind them: fast
    by_hand = {(0, 0): (6, 9), (0, AT_POS): (6, 9), (64, 0): (2, 15), (64, AT_POS): (0, 17)}
    for call in (call_ids, call_at):
        slow, fast = by_hand[(window, call[3])]
        case.claims += [("slow", tile, call, slow, fast) if tile <= tiles - 3 else ("slow", tile, call, 0, slow + fast) for tile in D_TILES(grid)]
    case.claims += [("same block", 0, grid, True, True), ("same block", 1, grid + 1, True, True)]
    return case


E_KINDS = ("delimiters", "open-end")


def top_of_range(kind, n=INT_MAX):
    """FAMILY E.  n = 2^31 - 1 (the host test: a copy of three tiles with the same bytes at the same distances from the end), fill 0, the model from
    the special bytes alone.  `mid`: 2^30; `last`: the last tile's first byte.  No pair lies far in front of a special byte: a value that runs
    on behind its tile's bitmaps is read by a lane alone, and 2^30 bytes of that are minutes"""
    text = Text(n, fill=0)
    last, mid = (n - 1) // T * T, (n + 1) // 2
    assert n - last > R + 600 and mid + 100 < last - 100
    text.put([mid - 1, mid, mid + 1, mid + 40], NL)
    text.put([mid - 4, mid - 3, mid + 2], BLANK)
    pos = [-1, mid - 300, mid - 7, mid - 7, mid - 1, mid, mid + 1, mid + 2, last - T + 9]
    ids = [1, 1, 1, 3, 2, 1, 1, 1, 1]
    if kind == "delimiters":
        text.put([last - 1, last, n - 2, n - 1, last + R + 500], NL)
        text.put([last + 1, last + 2, n - 3], BLANK)
        pos += [last - 50, last - 1, last, last, last + 1, n - 600, n - 100, n - 3, n - 2, n - 2, n - 1, n - 1, n, n]
        ids += [1, 1, 1, 3, 2, 4, 1, 1, 1, 2, 1, 4, 1, 2]                  # n - 2 + 2, n - 600 + R + 76, n - 1 + 2: b reaches and passes n
        locate = [(None, RUNS | BEFORE), (None, 0), (b"\n ", RUNS), (b"\n ", BEFORE)]
        capture = [(b" ", None, 0, 0), (b" ", None, 0, AT_POS), (b" ", b"\n ", 0, 0), (b"\0 ", None, 0, AT_POS), (None, None, 1 << 33, 0)]
    else:
        text.put(last - 60, NL)                                            # the last stop byte: a value from the tile in front of the last runs to n
        text.put(np.arange(n - 40, n), BLANK)                              # ... and a skip run ends with the input
        pos += [last - 50, last - 50, last, n - 100, n - 100, n - 41, n - 40, n - 1, n]
        ids += [1, 4, 1, 1, 2, 1, 1, 1, 1]
        locate = [(None, 0), (None, RUNS | BEFORE)]
        capture = [(b" ", None, 0, AT_POS), (b" ", None, 0, 0), (b"\0 ", None, 0, AT_POS)]
        capture += [(b" ", None, w, AT_POS) for w in (99, 100, 101, 60, 61)]   # from n - 100: b + window one below, on and one above n
        capture += [(b" ", None, 98, 0), (b" ", None, 97, 0)]              # ... by a length of 2: on and one below
    order = np.argsort(np.asarray(pos), kind="stable")
    return Case("E-%s-%d" % (kind, n), 0, text, np.asarray(pos)[order], np.asarray(ids)[order], locate, capture, [("n", n), ("pair at", n - 1)] +
                [("pair at", last)], dense=False)


# --------------------------------------------------------------------------------------------------------------------------- the slow count

class CaptureRun(C.Structure):              # include/pfac_module.h: PFACX_captureRun_t
    _fields_ = [("d_input", C.c_void_p), ("size", C.c_size_t), ("skip", C.c_uint * 8), ("stop", C.c_uint * 8), ("window", C.c_size_t),
                ("flags", C.c_uint), ("d_ids", C.c_void_p), ("d_pos", C.c_void_p), ("numPairs", C.c_size_t), ("d_patternLen", C.c_void_p),
                ("numLens", C.c_size_t), ("d_valStart", C.c_void_p), ("d_valLen", C.c_void_p)]


_module = None


def capture_run(handle, d_input, size, skip, stop, window, flags, d_ids, d_pos, num_pairs, d_lens, num_lens, d_val_start, d_val_len):
    """the module entry PFACX_captureRun (as tools/capture_sweep.py asks it) -> (status, *h_slowPairs); `skip`: S, the stop bytes are taken out here,
    as the entry wants them; `stop`: None for {'\\n'}"""
    global _module
    if _module is None:
        _module = C.CDLL(api.library_paths()[1])
        _module.PFACX_captureRun.argtypes = [C.c_void_p, C.POINTER(CaptureRun), C.POINTER(C.c_size_t)]
        _module.PFACX_captureRun.restype = C.c_int
    stop = b"\n" if stop is None else stop
    run = CaptureRun(d_input, size, api.word_class(bytes(set(skip or b"") - set(stop))), api.word_class(stop), window, flags,
                     None if flags & AT_POS else d_ids, d_pos, num_pairs, None if flags & AT_POS else d_lens, 0 if flags & AT_POS else num_lens,
                     d_val_start, d_val_len)
    slow = C.c_size_t(0)
    st = _module.PFACX_captureRun(handle._h, C.byref(run), C.byref(slow))
    return st, slow.value


# --------------------------------------------------------------------------------------------------------------------------- every case

def builders(grid, small=False):
    """name -> a call that builds the case of families A to D for `grid`; `small`: the same families over a few tiles (and a carry step of two
    tiles), for the byte-by-byte references"""
    a, b, c, d, step = (7, 5, 5, 5, 2) if small else (None, None, None, None, STEP)
    out = {}
    for variant in A_VARIANTS:
        out["A%d" % variant] = lambda v=variant: tiles_beyond_a_pass(grid, v, a)
    for kind in B_KINDS:
        out["B-" + kind] = lambda k=kind: lists_beyond_a_pass(grid, k, a if k == "on-A" else b)
    for kind in C_KINDS:
        out["C-" + kind] = lambda k=kind: carry_steps(grid, k, c, step)
    for window in D_WINDOWS:
        out["D-%d" % window] = lambda w=window: slow_pairs(grid, w, d)
    return out


NAMES = tuple(builders(0))
