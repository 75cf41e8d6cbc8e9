"""References for the approximate calls (PFACX_approx*: patterns matched within k mismatches) that share no code with the library.

model_pieces        the documented cut: part j of a pattern of L bytes with budget k is [j L // (k + 1), (j + 1) L // (k + 1)), its piece the
                    first min(part length, max_len) bytes; the distinct pieces take handle ids in order of first appearance -> what
                    PFACX_approxGetPieces must return
approx_brute        the definition: per pattern the numpy Hamming distance at every start -> the set of (id, start, d)
approx_pigeonhole   the filter the library is built on, restated: every occurrence of every distinct piece string is a candidate for the
                    (pattern, piece) entries of its class, a candidate is verified by its distance and dropped where a lower piece of the
                    pattern is exact at the same start -> the set of (id, start, d); it must equal the brute force as a set
ordered             the brute-force set in the order of the contract: candidate position start + partStart[j*] ascending (j*: the lowest exact
                    piece), at one candidate position the longer piece first, within one piece string pattern ids descending, then piece
                    indices descending -- NOT sorted by start -> (pos, ids, mis) int32
Patterns are bytes, ids are 1-based.  Test infrastructure only."""

import functools

import numpy as np

DEFAULT_MIN_PIECE = 4
DEFAULT_MAX_PIECE = 32
MAX_MISMATCHES = 7
MAX_PATTERN_LEN = 65535


def as_array(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)


def part_start(j, length, k):
    return j * length // (k + 1)


def cut(pattern, k, max_len=0):
    """[(start, length)] of the k + 1 pieces of one pattern"""
    most, length = max_len or DEFAULT_MAX_PIECE, len(pattern)
    return [(part_start(j, length, k), min(part_start(j + 1, length, k) - part_start(j, length, k), most)) for j in range(k + 1)]


def refusal(patterns, budgets, min_len=0, max_len=0):
    """the id of the first pattern PFACX_approxOpen must refuse, 0 for none"""
    least = min_len or DEFAULT_MIN_PIECE
    for i, (p, k) in enumerate(zip(patterns, budgets), start=1):
        if len(p) == 0 or len(p) > MAX_PATTERN_LEN or not 0 <= k <= MAX_MISMATCHES or len(p) < (k + 1) * least:
            return i
        if any(0x0A in bytes(p[s:s + n]) for s, n in cut(p, k, max_len)):
            return i
    return 0


def model_pieces(patterns, budgets, min_len=0, max_len=0):
    """what PFACX_approxGetPieces must return, by the documented rule: (piece_off [S + 2] by id, piece_id, piece_start, piece_len), and the
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


def distances(pattern, data):
    """the Hamming distance of one pattern at every start (uint16, n - L + 1 entries; none where the pattern is longer than the data)"""
    data, pat = as_array(data), as_array(pattern)
    length, n = pat.size, data.size
    if length > n:
        return np.zeros(0, dtype=np.uint16)
    d = np.zeros(n - length + 1, dtype=np.uint16)
    for t in range(length):
        d += data[t:t + n - length + 1] != pat[t]
    return d


def approx_brute(patterns, budgets, data):
    found = set()
    for i, (p, k) in enumerate(zip(patterns, budgets), start=1):
        d = distances(p, data)
        found.update((i, int(s), int(d[s])) for s in np.flatnonzero(d <= k))
    return found


def occurrences(piece, data):
    """every start of one byte string, overlapping ones included"""
    raw, out, at = bytes(data), [], 0
    while True:
        at = raw.find(piece, at)
        if at < 0:
            return out
        out.append(at)
        at += 1


def approx_pigeonhole(patterns, budgets, data, max_len=0):
    raw, found = bytes(as_array(data)), set()
    n = len(raw)
    cache = {}
    for i, (p, k) in enumerate(zip(patterns, budgets), start=1):
        p = bytes(p)
        pieces = cut(p, k, max_len)
        for j, (start, length) in enumerate(pieces):
            key = p[start:start + length]
            if key not in cache:
                cache[key] = occurrences(key, raw)
            for at in cache[key]:
                s = at - start
                if s < 0 or s + len(p) > n:
                    continue
                if any(raw[s + a:s + a + b] == p[a:a + b] for a, b in pieces[:j]):
                    continue                                        # a lower exact piece reports it
                d = sum(x != y for x, y in zip(raw[s:s + len(p)], p))
                if d <= k:
                    found.add((i, s, d))
    return found


def ordered(found, patterns, budgets, data, max_len=0):
    """a set of (id, start, d) -> (pos, ids, mis) in the order of the contract"""
    raw, keyed = bytes(as_array(data)), []
    for i, s, d in found:
        p, k = bytes(patterns[i - 1]), budgets[i - 1]
        exact = [(j, a, b) for j, (a, b) in enumerate(cut(p, k, max_len)) if raw[s + a:s + a + b] == p[a:a + b]]
        assert exact, "the pigeonhole: an occurrence within k substitutions has an exact part among k + 1"
        j, a, b = exact[0]
        keyed.append((s + a, -b, -i, -j, s, i, d))
    keyed.sort()
    return tuple(np.array([e[c] for e in keyed], dtype=np.int32) for c in (4, 5, 6))


def same(got, want, what):
    got, want = ([np.asarray(a, dtype=np.int64) for a in t] for t in (got, want))
    assert got[0].size == want[0].size, f"{what}: {got[0].size} entries, want {want[0].size}"
    for g, w, column in zip(got, want, ("start", "id", "distance")):
        bad = np.flatnonzero(g != w)
        if bad.size:
            e = int(bad[0])
            raise AssertionError(f"{what}: {bad.size} entries differ in their {column}, first at {e}: got (id {got[1][e]}, start {got[0][e]}, "
                                 f"d {got[2][e] if len(got) > 2 else '-'}) want (id {want[1][e]}, start {want[0][e]}, d {want[2][e] if len(want) > 2 else '-'})")


def check_models(patterns, budgets, data, what, max_len=0):
    """both models on one test input, as sets -> the ordered list (pos, ids, mis)"""
    brute = approx_brute(patterns, budgets, data)
    pigeon = approx_pigeonhole(patterns, budgets, data, max_len)
    assert brute == pigeon, f"{what}: the models differ: only brute {sorted(brute - pigeon)[:5]}, only pigeonhole {sorted(pigeon - brute)[:5]}"
    return ordered(brute, patterns, budgets, data, max_len)


# ---------------------------------------------------------------- the compare edges


def edge_pattern(length):
    """`length` bytes no two neighbours of which are equal, none of them 0x0A, '.' or >= 0x80"""
    return bytes(0x30 + ((11 * i + 5 * length) % 0x4B) for i in range(length))


def mutate(pattern, where):
    out = bytearray(pattern)
    for at in where:
        out[at] ^= 0x80
    return bytes(out)


def deciding_positions(length):
    """byte 0, bytes 15 / 16 and 31 / 32 (the early-exit test), both ends of the last whole dword, each of the length & 3 tail bytes"""
    whole = 4 * (length // 4)
    spots = {0, 15, 16, 31, 32, whole - 4, whole - 1} | set(range(whole, length))
    return sorted(x for x in spots if 0 <= x < length)


@functools.lru_cache(maxsize=None)
def edge_case(k, lengths=None):
    """patterns of every length (k + 1) .. 64 (k = 0: 1 .. 64) with budget k and minPieceLen 1, and an input that holds each of them, per deciding
    position x, with exactly k substitutions (x among them: accepted) and with k + 1 (rejected).  Where the part of x is long enough the other
    substitutions lie in it too, so every other piece stays exact and the compare itself must reject; else they are spread by a seeded draw.
    Gaps of 1 .. 4 bytes put the starts at every residue mod 4; the input ends with an accepted placement
    -> (patterns, budgets, input, [(id, start, substitutions)])"""
    rng = np.random.default_rng(1000 + k)
    lengths = tuple(lengths or range(max(1, k + 1), 65))
    patterns = [edge_pattern(length) for length in lengths]
    out, placed = bytearray(b"."), []
    for i, p in enumerate(patterns, start=1):
        length = len(p)
        for x in deciding_positions(length):
            j = next(j for j in range(k + 1) if part_start(j, length, k) <= x < part_start(j + 1, length, k))
            part = [t for t in range(part_start(j, length, k), part_start(j + 1, length, k)) if t != x]
            for extra in (k - 1, k):
                if extra < 0:
                    continue                                        # k = 0: the accepted placement is the pattern itself, placed once below
                pool = part if len(part) >= extra else [t for t in range(length) if t != x]
                if len(pool) < extra:
                    continue
                where = [x] + [int(t) for t in rng.choice(pool, size=extra, replace=False)]
                placed.append((i, len(out), len(where)))
                out += mutate(p, where) + b"." * (1 + len(placed) % 4)
        placed.append((i, len(out), 0))
        out += p + b"." * (1 + i % 4)
    last = patterns[-1]
    where = deciding_positions(len(last))[-k:] if k else []
    placed.append((len(patterns), len(out), len(where)))
    out += mutate(last, where)
    return patterns, [k] * len(patterns), bytes(out), placed


def check_edge_case(k, lengths=None):
    """the edge input holds what it is meant to -> the ordered list"""
    patterns, budgets, data, placed = edge_case(k, lengths)
    want = check_models(patterns, budgets, data, f"edges k = {k}", max_len=0)
    found = {(int(i), int(s)): int(d) for s, i, d in zip(*want)}
    for i, s, subs in placed:
        assert (found.get((i, s)) == subs) if subs <= k else ((i, s) not in found), (k, i, s, subs)
    assert any(subs == k + 1 for _, _, subs in placed) and any(subs == k for _, _, subs in placed)
    assert {s & 3 for _, s, subs in placed if subs <= k} == {0, 1, 2, 3}, "accepted starts at every residue mod 4"
    assert max(s + len(patterns[i - 1]) for i, s, _ in placed) == len(data), "the input ends with a placement"
    return want


# ---------------------------------------------------------------- the seeded random cases (tests/test_approx_gpu.py, tools/approx_sweep.py)

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
PRINTABLE = np.arange(0x20, 0x7F, dtype=np.uint8)


def random_patterns(seed, alphabet, count=100, min_len=12, max_len=150, max_k=4):
    """`count` patterns of min_len .. max_len letters with budgets 0 .. max_k, as far as the default minPieceLen lets a pattern have one"""
    rng = np.random.default_rng(seed)
    patterns, budgets = [], []
    for _ in range(count):
        length = int(rng.integers(min_len, max_len + 1))
        patterns.append(bytes(alphabet[rng.integers(0, alphabet.size, length)]))
        budgets.append(int(rng.integers(0, min(max_k, length // DEFAULT_MIN_PIECE - 1) + 1)))
    return patterns, budgets


def substitute(pattern, count, alphabet, rng):
    out = bytearray(pattern)
    for at in rng.choice(len(out), size=count, replace=False):
        others = alphabet[alphabet != out[at]]
        out[at] = int(others[rng.integers(0, others.size)])
    return bytes(out)


def embed(patterns, budgets, data, alphabet, seed):
    """`data` (uint8, modified in place) with every pattern at random places: with exactly k, with k + 1 and with 0 substitutions (a later
    placement may overwrite an earlier one: the models say what is left)"""
    rng = np.random.default_rng(seed + 1)
    n = data.size
    for p, k in zip(patterns, budgets):
        for count in (k, k + 1, 0):
            if count > len(p) or len(p) > n:
                continue
            at = int(rng.integers(0, n - len(p) + 1))
            data[at:at + len(p)] = as_array(substitute(p, count, alphabet, rng))
    return data


@functools.lru_cache(maxsize=None)
def random_case(kind, seed=20261021, count=100, n=1 << 16):
    """kind `acgt` or `text` -> (patterns, budgets, data)"""
    alphabet = ACGT if kind == "acgt" else PRINTABLE
    patterns, budgets = random_patterns(seed + (kind == "text"), alphabet, count)
    rng = np.random.default_rng(seed + 2)
    data = embed(patterns, budgets, alphabet[rng.integers(0, alphabet.size, n)].copy(), alphabet, seed)
    data.setflags(write=False)
    return patterns, budgets, data


@functools.lru_cache(maxsize=None)
def random_want(kind):
    patterns, budgets, data = random_case(kind)
    return check_models(patterns, budgets, data, f"random {kind}")


# ---------------------------------------------------------------- the case table (tools/approx_host_san.cpp has the same table)

P32 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ012345"                # k = 3: four parts of 8 bytes, each its own piece


def only_piece_exact(j):
    """P32 with one substitution in every part but part j: d = 3, found through piece j alone"""
    return mutate(P32, [8 * e + 3 for e in range(4) if e != j])


# (name, patterns, budgets, minPieceLen, maxPieceLen, input)
CASES = [
    ("keywords-with-typos", [b"password", b"username", b"creditcard", b"passport"], [1, 1, 1, 1], 0, 0,
     b"pasword password passw0rd usermame user_name creditcard cred1tcarb passp0rt pa55port xpassworx"),
    ("each-piece-alone", [P32], [3], 0, 0, b" ".join(only_piece_exact(j) for j in range(4))),
    ("all-pieces-exact-one-entry", [P32], [3], 0, 0, b"--" + P32 + b"--" + P32),
    ("pieces-1-and-3-exact", [P32], [3], 0, 0, b"-" + mutate(P32, [0, 20]) + b"-"),
    ("four-substitutions-are-too-many", [P32], [3], 0, 0,
     mutate(P32, [1, 9, 17, 25]) + b" " + mutate(P32, [9, 10, 17, 25]) + b" " + mutate(P32, [9, 17, 25])),
    ("one-piece-string-thrice", [b"abcdabcdabcd"], [2], 0, 0, b"abcd" * 8),
    ("two-patterns-share-a-piece", [b"sharedXYZW", b"QRSTshared", b"sharedshar"], [0, 1, 0], 0, 6, b"sharedXYZW QRSTshared QRSTsharex xRSTshared sharedshared"),
    ("identical-patterns-budgets-0-and-2", [b"identicalxyz", b"identicalxyz"], [0, 2], 0, 0, b"identicalxyz idemticalxyy idxnticalxyz ixentxcalxyx"),
    ("a-piece-is-a-prefix-of-another", [b"abcdefgh", b"abcdWXYZ", b"abcdefXY"], [0, 1, 0], 0, 0, b"abcdefgh abcdWXYy abcdefXY abcdWXYZabcdefgh"),
    ("newline-outside-the-pieces", [b"abc\ndefg", b"abcd\nefgh"], [1, 0], 0, 3, b"abc\ndefg abcxdefg abc\ndexg abcd\nefgh abcdxefgh xbc\ndefg"),
    ("the-cut-of-a-piece", [b"0123456789abcdefghij"], [1], 0, 5, b"0123456789abcdefghij 01234x6789abcdefghij x123456789abcdefghij 0123456789xbcdefghij"),
    ("not-sorted-by-start", [b"xxxxxxxxabcd", b"xyxx"], [1, 0], 0, 0, b"xxxxxyxxabcd"),
    ("single-bytes", [b"a", b"b", b"a"], [0, 0, 0], 1, 0, b"abab"),
    ("one-byte-parts", [b"abc", b"abd"], [2, 1], 1, 0, b"abc abd xbc axx xxc abx"),
    ("compare-edges-k1", None, None, 1, 0, None),            # edge_case(1) at a few lengths: case_of() fills it in
]
EDGE_LENGTHS = (2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 64)
# what the definition gives, worked out by hand: name -> (ids, starts, distances)
WANT = {
    "all-pieces-exact-one-entry": ([1, 1], [2, 36], [0, 0]),
    "pieces-1-and-3-exact": ([1], [1], [2]),
    # occurrences at 0, 4, .., 20, each reported by piece 0 at its own start
    "one-piece-string-thrice": ([1] * 6, [0, 4, 8, 12, 16, 20], [0] * 6),
    # xyxx at 4 is a candidate at 4; the long pattern at 0 has its piece 0 broken and is reported by piece 1 at candidate position 6
    "not-sorted-by-start": ([2, 1], [4, 0], [0, 1]),
    # at 0 the whole pattern (the piece of budget 0) is the longer piece: chain order puts pattern 1 first; 13 and 26 are found through piece 1
    "identical-patterns-budgets-0-and-2": ([1, 2, 2, 2], [0, 0, 13, 26], [0, 0, 2, 1]),
    "single-bytes": ([3, 1, 2, 3, 1, 2], [0, 0, 1, 2, 2, 3], [0] * 6),
}


def case_of(case):
    """-> (name, patterns, budgets, min_len, max_len, data)"""
    if case[1] is not None:
        return case
    patterns, budgets, data, _ = edge_case(1, EDGE_LENGTHS)
    return (case[0], patterns, budgets, case[3], case[4], data)


def test_the_models_agree_on_every_case():
    for case in CASES:
        name, patterns, budgets, min_len, max_len, data = case_of(case)
        assert refusal(patterns, budgets, min_len, max_len) == 0, name
        want = check_models(patterns, budgets, data, name, max_len)
        if name in WANT:
            ids, pos, mis = WANT[name]
            same(want, (pos, ids, mis), f"{name}: the models against the list worked out by hand")
        assert want[0].size > 0, name
    pos, ids, mis = check_models([P32], [3], CASES[1][5], "each piece alone")
    assert pos.tolist() == [0, 33, 66, 99] and mis.tolist() == [3] * 4
    assert check_models([P32], [3], CASES[4][5], "too many")[0].tolist() == [66], "d = 4 is refused with and without an exact piece"
    for k in range(4):
        check_edge_case(k, EDGE_LENGTHS if k == 1 else tuple(length for length in EDGE_LENGTHS if length > k))
    assert cut(b"x" * 10, 2) == [(0, 3), (3, 3), (6, 4)] and cut(b"x" * 100, 1) == [(0, 32), (50, 32)] and cut(b"x" * 9, 0, 4) == [(0, 4)]
    assert refusal([b"abcdefg"], [1]) == 1 and refusal([b"abcdefgh"], [1]) == 0 and refusal([b"ab"], [1], 1) == 0 and refusal([b"a"], [1], 1) == 1
    assert refusal([b"abcd", b"ab\ncdefg"], [0, 0]) == 2 and refusal([b"abcd", b"abcd\n"], [0, 0], 0, 4) == 0 and refusal([b"x" * 64], [8]) == 1
