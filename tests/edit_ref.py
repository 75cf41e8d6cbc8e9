"""References for the edit-distance calls (PFACX_edit*: patterns matched within k edits, indels included) that share no code with the library.

model_pieces / refusal   the documented cut, that of PFACX_approxOpen -> what PFACX_editGetPieces must return, and whom PFACX_editOpen refuses
edit_columns             the definition: Sellers' recurrence per pattern, row by row over all n + 1 columns in numpy; cost and start are packed as
                         cost << 32 | (2^31 - start), so a plain minimum prefers the lower cost, then the larger start; the horizontal term of a
                         row is c + minimum.accumulate(V - c) -> (D, start) per column
edit_brute               the set of (id, start, end, d) from edit_columns, every end or only the ends the three-point rule keeps (best_ends)
edit_naive               for small inputs only: min over s of a plain recursive Levenshtein of pat against in[s:e], the largest s on ties; it
                         pins edit_columns
edit_pigeonhole          the filter the library is built on, restated: every occurrence of a piece is a candidate with the diagonal d0 = p - o; a
                         dynamic program over the band of 2 k + 1 diagonals on either side of d0 gives (D, start) at the covered ends
                         |e - L - d0| <= k and at their neighbours; an end is kept by the covering candidate with the smallest piece index, of
                         those the smallest position -> the set of (id, start, end, d); it must equal the brute force as a set
ordered                  the brute-force set in the order of the contract: owning candidate position ascending, at one position the longer piece
                         first, within one piece string pattern ids descending, then piece indices descending, within one (candidate, entry)
                         ends ascending -- NOT sorted by start or end -> (ids, start, end, dist) int32
Patterns are bytes, ids are 1-based.  Test infrastructure only."""

import functools

import numpy as np

DEFAULT_MIN_PIECE = 4
DEFAULT_MAX_PIECE = 32
MAX_EDITS = 7
MAX_PATTERN_LEN = 65535
BEST_ENDS = 1
ONE = 1 << 32
TOP = 1 << 31


def as_array(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)


def part_start(j, length, k):
    return j * length // (k + 1)


def cut(pattern, k, max_len=0):
    """[(start, length)] of the k + 1 pieces of one pattern"""
    most, length = max_len or DEFAULT_MAX_PIECE, len(pattern)
    return [(part_start(j, length, k), min(part_start(j + 1, length, k) - part_start(j, length, k), most)) for j in range(k + 1)]


def refusal(patterns, budgets, min_len=0, max_len=0):
    """the id of the first pattern PFACX_editOpen must refuse, 0 for none"""
    least = min_len or DEFAULT_MIN_PIECE
    for i, (p, k) in enumerate(zip(patterns, budgets), start=1):
        if len(p) == 0 or len(p) > MAX_PATTERN_LEN or not 0 <= k <= MAX_EDITS or len(p) < (k + 1) * least:
            return i
        if any(0x0A in bytes(p[s:s + n]) for s, n in cut(p, k, max_len)):
            return i
    return 0


def model_pieces(patterns, budgets, min_len=0, max_len=0):
    """what PFACX_editGetPieces must return, by the documented rule: (piece_off [S + 2] by id, piece_id, piece_start, piece_len), and the
    distinct pieces by handle id - 1"""
    assert refusal(patterns, budgets, min_len, max_len) == 0
    off, ids, starts, lens, seen, pieces = [0, 0], [], [], [], {}, []
    for p, k in zip(patterns, budgets):
        for s, n in cut(p, k, max_len):
            key = bytes(p[s:s + n])
            if key not in seen:
                pieces.append(key)
                seen[key] = len(pieces)
            ids.append(seen[key])
            starts.append(s)
            lens.append(n)
        off.append(len(ids))
    return (np.array(off, np.uint64), np.array(ids, np.int32), np.array(starts, np.int32), np.array(lens, np.int32)), pieces


# ---------------------------------------------------------------- the definition


def edit_columns(pattern, data):
    """(D, start) of one pattern at every end 0 .. n (int64 arrays of n + 1 entries)"""
    data, pat = as_array(data), as_array(pattern)
    n = data.size
    c = np.arange(n + 1, dtype=np.int64)
    v = TOP - c                                                             # row 0: cost 0, start c
    for r in range(1, pat.size + 1):
        u = v + ONE                                                         # a pattern byte left out; u[0] = r with start 0
        u[1:] = np.minimum(u[1:], v[:-1] + (data != pat[r - 1]).astype(np.int64) * ONE)
        v = c * ONE + np.minimum.accumulate(u - c * ONE)                    # ... and input bytes put in
    return v >> 32, TOP - (v & (ONE - 1))


def best_ends(dist, k):
    """the ends the three-point rule keeps: D(e) <= k, D(e - 1) > D(e), and e == n or D(e + 1) >= D(e)"""
    n = dist.size - 1
    keep = []
    for e in np.flatnonzero(dist <= k):
        e = int(e)
        if e >= 1 and dist[e - 1] > dist[e] and (e == n or dist[e + 1] >= dist[e]):
            keep.append(e)
    return keep


def edit_brute(patterns, budgets, data, flags=0):
    found = set()
    for i, (p, k) in enumerate(zip(patterns, budgets), start=1):
        dist, start = edit_columns(p, data)
        ends = best_ends(dist, k) if flags & BEST_ENDS else [int(e) for e in np.flatnonzero(dist <= k)]
        found.update((i, int(start[e]), e, int(dist[e])) for e in ends)
    return found


def levenshtein(a, b):
    @functools.lru_cache(maxsize=None)
    def go(x, y):
        if x == 0 or y == 0:
            return x + y
        return min(go(x - 1, y - 1) + (a[x - 1] != b[y - 1]), go(x - 1, y) + 1, go(x, y - 1) + 1)
    return go(len(a), len(b))


def edit_naive(patterns, budgets, data, flags=0):
    """small inputs only"""
    raw, found = bytes(as_array(data)), set()
    n = len(raw)
    for i, (p, k) in enumerate(zip(patterns, budgets), start=1):
        p = bytes(p)
        best = []
        for e in range(n + 1):
            best.append(min((levenshtein(p, raw[s:e]), -s) for s in range(e + 1)))
        dist = np.array([b[0] for b in best])
        ends = best_ends(dist, k) if flags & BEST_ENDS else [e for e in range(n + 1) if dist[e] <= k]
        found.update((i, -best[e][1], e, best[e][0]) for e in ends)
    return found


# ---------------------------------------------------------------- the pigeonhole filter, restated


def occurrences(piece, raw):
    """every start of one byte string, overlapping ones included"""
    out, at = [], 0
    while True:
        at = raw.find(piece, at)
        if at < 0:
            return out
        out.append(at)
        at += 1


def band_row(p, raw, d0, k):
    """{column: (cost, -start)} of the last row of the band of 2 k + 1 diagonals on either side of d0; None where a row is all above k"""
    n, width = len(raw), 2 * k + 1
    row = {c: (0, -c) for c in range(d0 - width, d0 + width + 1) if 0 <= c <= n}
    for r in range(1, len(p) + 1):
        new = {}
        for c in range(r + d0 - width, r + d0 + width + 1):
            if not 0 <= c <= n:
                continue
            best = []
            if c - 1 in row:
                best.append((row[c - 1][0] + (p[r - 1] != raw[c - 1]), row[c - 1][1]))
            if c in row and c - r - d0 < width:                      # the cell above lies inside the band of its row
                best.append((row[c][0] + 1, row[c][1]))
            if c - 1 in new:
                best.append((new[c - 1][0] + 1, new[c - 1][1]))
            if best:
                new[c] = min(best)
        row = new
        if not row or min(v[0] for v in row.values()) > k:
            return None
    return row


def owner(p, k, pieces, raw, e):
    """the covering candidate (j, position) with the smallest j, of those the smallest position; None where nothing covers (i, e)"""
    n, length = len(raw), len(p)
    for j, (o, plen) in enumerate(pieces):
        for at in range(max(0, e - length + o - k), min(n - plen, e - length + o + k) + 1):
            if raw[at:at + plen] == p[o:o + plen]:
                return j, at
    return None


def edit_pigeonhole(patterns, budgets, data, flags=0, max_len=0):
    raw, found = bytes(as_array(data)), set()
    n, cache = len(raw), {}
    for i, (p, k) in enumerate(zip(patterns, budgets), start=1):
        p = bytes(p)
        pieces, length = cut(p, k, max_len), len(p)
        for j, (o, plen) in enumerate(pieces):
            key = p[o:o + plen]
            if key not in cache:
                cache[key] = occurrences(key, raw)
            for at in cache[key]:
                d0 = at - o
                if d0 < -k or length + d0 - k > n:
                    continue
                row = band_row(p, raw, d0, k)
                if row is None:
                    continue
                for e in range(max(0, length + d0 - k), min(n, length + d0 + k) + 1):
                    if e not in row or row[e][0] > k:
                        continue
                    d = row[e][0]
                    if flags & BEST_ENDS:
                        before = row[e - 1][0] if e - 1 in row else k + 1
                        behind = row[e + 1][0] if e + 1 in row else k + 1
                        if not (min(before, k + 1) > d and (e == n or min(behind, k + 1) >= d)):
                            continue
                    if owner(p, k, pieces, raw, e) != (j, at):
                        continue
                    found.add((i, -row[e][1], e, d))
    return found


def ordered(found, patterns, budgets, data, max_len=0):
    """a set of (id, start, end, d) -> (ids, start, end, dist) in the order of the contract"""
    raw, keyed = bytes(as_array(data)), []
    for i, s, e, d in found:
        p, k = bytes(patterns[i - 1]), budgets[i - 1]
        pieces = cut(p, k, max_len)
        own = owner(p, k, pieces, raw, e)
        assert own is not None, "the pigeonhole: an occurrence within k edits has an untouched part among k + 1"
        j, at = own
        keyed.append((at, -pieces[j][1], -i, -j, e, i, s, e, d))
    keyed.sort()
    return tuple(np.array([x[c] for x in keyed], dtype=np.int32) for c in (5, 6, 7, 8))


def same(got, want, what):
    got, want = ([np.asarray(a, dtype=np.int64) for a in t] for t in (got, want))
    assert got[0].size == want[0].size, f"{what}: {got[0].size} entries, want {want[0].size}"
    rows_got, rows_want = list(zip(*[a.tolist() for a in got])), list(zip(*[a.tolist() for a in want]))
    for at, (g, w) in enumerate(zip(rows_got, rows_want)):
        assert g == w[:len(g)], f"{what}: entry {at}: got (id, start, end, d) {g}, want {w}"


@functools.lru_cache(maxsize=None)
def _models(patterns, budgets, data, flags, max_len):
    brute = edit_brute(patterns, budgets, data, flags)
    pigeon = edit_pigeonhole(patterns, budgets, data, flags, max_len)
    return brute, pigeon


def check_models(patterns, budgets, data, what, flags=0, max_len=0):
    """both models on one test input, as sets -> the ordered list (ids, start, end, dist); cached: a reference is computed once"""
    patterns, budgets, raw = tuple(bytes(p) for p in patterns), tuple(int(k) for k in budgets), bytes(as_array(data))
    brute, pigeon = _models(patterns, budgets, raw, flags, max_len)
    assert brute == pigeon, f"{what}: the models differ: only brute {sorted(brute - pigeon)[:5]}, only pigeonhole {sorted(pigeon - brute)[:5]}"
    return _ordered(patterns, budgets, raw, flags, max_len)


@functools.lru_cache(maxsize=None)
def _ordered(patterns, budgets, raw, flags, max_len):
    return ordered(_models(patterns, budgets, raw, flags, max_len)[0], patterns, budgets, raw, max_len)


# ---------------------------------------------------------------- the case table: (name, patterns, budgets, min_len, max_len, data)

CASES = [
    ("one-substitution", [b"abcdefgh"], [1], 0, 0, b"__abcXefgh__"),
    ("one-insertion", [b"abcdefgh"], [1], 0, 0, b"__abcdXefgh__"),
    ("one-deletion", [b"abcdefgh"], [1], 0, 0, b"__abcefgh__"),
    ("exact-copy-k2", [b"abcdefghijkl"], [2], 0, 0, b"__abcdefghijkl__"),
    ("abab", [b"abababab"], [1], 0, 0, b"__abababab__"),
    ("not-sorted-by-start", [b"abcdefgh", b"cdef"], [1, 0], 0, 0, b"_aXcdefgh_"),
    ("identical-patterns", [b"wxyzwxyz", b"wxyzwxyz"], [0, 1], 0, 0, b"wxyzwxyz"),
    ("starts-at-0-ends-at-n", [b"mnopqrstuvwx"], [2], 0, 0, b"nopqrstuvw"),
    ("short-pieces", [b"abc", b"ab"], [2, 1], 1, 0, b"xabcxacxbx"),
    ("long-piece-first", [b"abcdefgh", b"abcd"], [0, 0], 0, 0, b"..abcdefgh..abcd"),
]

# worked out by hand: the list in contract order as (id, start, end, d), all ends, and the list under PFACX_EDIT_BEST_ENDS
WANT = {
    "one-substitution": ([(1, 2, 10, 1)], [(1, 2, 10, 1)]),
    "one-insertion": ([(1, 2, 11, 1)], [(1, 2, 11, 1)]),
    "one-deletion": ([(1, 2, 9, 1)], [(1, 2, 9, 1)]),
    # five ends around an exact copy, one under the rule; all owned by piece 0 at position 2
    "exact-copy-k2": ([(1, 2, 12, 2), (1, 2, 13, 1), (1, 2, 14, 0), (1, 2, 15, 1), (1, 2, 16, 2)], [(1, 2, 14, 0)]),
    # `abab` lies at 2, 4 and 6; piece 1 at 6 and piece 0 at 2 and 4 reach these ends: piece 0 at 2 owns all three
    "abab": ([(1, 2, 9, 1), (1, 2, 10, 0), (1, 2, 11, 1)], [(1, 2, 10, 0)]),
    # the first and the last byte are missing: the occurrence starts at 0 and ends at n
    "starts-at-0-ends-at-n": ([(1, 0, 10, 2)], [(1, 0, 10, 2)]),
    # pattern 2 is found at position 3, pattern 1 (start 1) only through its second piece at position 5
    "not-sorted-by-start": ([(2, 3, 7, 0), (1, 1, 9, 1)], [(2, 3, 7, 0), (1, 1, 9, 1)]),
}


def case_of(case):
    name, patterns, budgets, min_len, max_len, data = case
    return name, list(patterns), list(budgets), min_len, max_len, as_array(data)


def want_of(name, flags):
    rows = WANT[name][1 if flags & BEST_ENDS else 0]
    return tuple(np.array([r[c] for r in rows], dtype=np.int32) for c in range(4))


# ---------------------------------------------------------------- band edges, early exit, random sets


def edge_pattern(length, salt=0):
    """`length` bytes no two of which within 75 are equal, none of them 0x0A, '.' or >= 0x80"""
    return bytes(0x30 + ((11 * i + 5 * length + salt) % 0x4B) for i in range(length))


def apply_edits(pattern, edits):
    """edits: [(kind, at)] with kind 's' (substitute pattern byte at), 'd' (delete it), 'i' (insert a byte in front of it); distinct positions"""
    out = []
    by_at = {}
    for kind, at in edits:
        by_at.setdefault(at, []).append(kind)
    for at in range(len(pattern) + 1):
        kinds = by_at.get(at, [])
        for kind in kinds:
            if kind == "i":
                out.append(0x7E)
        if at < len(pattern):
            if "d" in kinds:
                continue
            out.append(pattern[at] ^ 0x80 if "s" in kinds else pattern[at])
    return bytes(out)


def band_input(pattern, k, max_len=0):
    """the pattern with exactly k edits -- all insertions in front of the exact piece, all behind it, all deletions, mixed -- and with k + 1
    (every part touched), '.'-separated: with k edits the alignment ends k diagonals off the candidate's"""
    parts = cut(pattern, k, max_len)
    inside = [o + min(1, n - 1) for o, n in parts]
    kinds = "sid"
    variants = [
        [("i", inside[j]) for j in range(k)],                                           # the last part exact
        [("i", inside[j]) for j in range(1, k + 1)],                                    # the first part exact
        [("d", inside[j]) for j in range(k + 1) if j != k // 2],
        [(kinds[j % 3], inside[j]) for j in range(k + 1) if j != k // 2],
        [(kinds[j % 3], inside[j]) for j in range(k + 1)],                              # k + 1 edits: no part is left
    ]
    return b"....".join([b""] + [apply_edits(pattern, v) for v in variants] + [b""]) + b"................"


BAND = [(k, length) for k in range(4) for length in sorted({k + 1, 2 * k + 3, 17, 33, 64})] + [(5, 40), (7, 64)]


def random_set(alphabet, seed, count=100, size=32 << 10, min_len=0):
    """`count` patterns of 12 .. 150 bytes with budgets 0 .. 3 over `size` bytes of `alphabet`, each embedded with exactly k, k + 1 and 0 random
    edits of all three kinds -> (patterns, budgets, data)"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(alphabet, dtype=np.uint8)
    least = min_len or DEFAULT_MIN_PIECE
    data = letters[rng.integers(0, letters.size, size)].copy()
    patterns, budgets = [], []
    at = 64
    for _ in range(count):
        length = int(rng.integers(12, 151))
        k = int(rng.integers(0, min(3, length // least - 1) + 1))
        p = bytes(letters[rng.integers(0, letters.size, length)])
        patterns.append(p)
        budgets.append(k)
        for edits in (k, k + 1, 0):
            q = bytearray(p)
            for _ in range(edits):
                x = int(rng.integers(0, len(q)))
                kind = int(rng.integers(0, 3))
                other = int(letters[rng.integers(0, letters.size)])
                if kind == 0:
                    q[x] = other if other != q[x] else int(letters[(int(np.flatnonzero(letters == other)[0]) + 1) % letters.size])
                elif kind == 1:
                    q.insert(x, other)
                elif len(q) > 1:
                    del q[x]
            if at + len(q) + 8 < size:
                data[at:at + len(q)] = np.frombuffer(bytes(q), dtype=np.uint8)
                at += len(q) + int(rng.integers(1, 40))
    return patterns, budgets, data


RANDOM_SETS = {"acgt": (b"ACGT", 20261, 8), "text": (b"abcdefghijklmnopqrstuvwxyz ", 20262, 0)}


@functools.lru_cache(maxsize=None)
def random_case(name):
    alphabet, seed, min_len = RANDOM_SETS[name]
    patterns, budgets, data = random_set(alphabet, seed, min_len=min_len)
    want = check_models(patterns, budgets, data, name)
    assert 100 <= want[0].size <= 20000 and set(want[3].tolist()) == {0, 1, 2, 3}, (want[0].size, sorted(set(want[3].tolist())))
    return patterns, budgets, min_len, data, want
