"""Reference for PFACX_rules* (include/pfac_ext.h) that does not call the library: pattern id occurs in a segment iff `pattern in segment_bytes`
(both folded by the ASCII fold for a caseless set), a rule fires iff all of its patterns occur.  Also the case table both test files share, a seeded
random generator of (patterns, rules, data, offsets) and a numpy form of the reference for inputs of tens of MiB.  Test infrastructure only."""
import numpy as np


def fold(b):
    """the ASCII fold of PFACX_READ_NOCASE"""
    return bytes(b).lower()          # bytes.lower() folds 'A'-'Z' alone


def fired_py(pats, rules, data, offsets=None, nocase=False):
    """(seg[], rule[], segFirst[]) of the fired list: pats[i] is pattern id i + 1, rules a list of id lists, offsets numSegments + 1 byte offsets
    (None: one segment)"""
    data = bytes(data)
    offsets = [0, len(data)] if offsets is None else [int(o) for o in offsets]
    if nocase:
        data, pats = fold(data), [fold(p) for p in pats]
    seg, rule, first = [], [], []
    for k in range(len(offsets) - 1):
        first.append(len(seg))
        piece = data[offsets[k]:offsets[k + 1]]
        present = {}
        for r, ids in enumerate(rules):
            ok = True
            for i in ids:
                if i not in present:
                    present[i] = len(pats[i - 1]) > 0 and pats[i - 1] in piece
                if not present[i]:
                    ok = False
                    break
            if ok:
                seg.append(k)
                rule.append(r)
    first.append(len(seg))
    return np.array(seg, dtype=np.int32), np.array(rule, dtype=np.int32), np.array(first, dtype=np.uint64)


def csr(rules):
    """(rule_off, rule_patterns) as PFACX_rulesOpen takes them"""
    off = np.zeros(len(rules) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in rules])
    flat = np.array([i for r in rules for i in r], dtype=np.int32)
    return off, flat


def same(got, want, what):
    """got / want: (seg, rule, segFirst)"""
    for g, w, name in zip(got, want, ("seg", "rule", "segFirst")):
        g, w = np.asarray(g).astype(np.int64), np.asarray(w).astype(np.int64)
        assert g.shape == w.shape, f"{what}: {name}: {g.size} entries, want {w.size}"
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            raise AssertionError(f"{what}: {name}: {bad.size} mismatches; first at {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}")


def present_matrix(pats, data, offsets):
    """present[k, i]: pats[i] occurs inside segment k -- numpy over the whole buffer: the positions of a pattern's first byte (found once per
    byte value), narrowed byte by byte, then the segment the occurrence starts in and whether it ends there.  For inputs where the loop of
    fired_py is too slow"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offsets = np.asarray(offsets, dtype=np.int64)
    segs = offsets.size - 1
    present = np.zeros((segs, len(pats)), dtype=bool)
    starts = {}
    for i, p in enumerate(pats):
        m = len(p)
        if m == 0 or m > data.size:
            continue
        if p[0] not in starts:
            starts[p[0]] = np.nonzero(data == p[0])[0]
        at = starts[p[0]]
        at = at[at + m <= data.size]
        for j in range(1, m):
            at = at[data[at + j] == p[j]]
        if at.size == 0:
            continue
        k = np.searchsorted(offsets, at, side="right") - 1          # the last segment that starts at or in front of the occurrence
        k = np.minimum(k, segs - 1)
        inside = at + m <= offsets[k + 1]
        present[k[inside], i] = True
    return present


def fired_np(pats, rules, data, offsets):
    """fired_py by present_matrix (case-sensitive)"""
    present = present_matrix(pats, data, offsets)
    fired = np.ones((present.shape[0], len(rules)), dtype=bool)
    for r, ids in enumerate(rules):
        for i in ids:
            fired[:, r] &= present[:, i - 1]
    seg, rule = np.nonzero(fired)                                    # row-major: ascending segment, ascending rule within it
    first = np.zeros(present.shape[0] + 1, dtype=np.uint64)
    first[1:] = np.cumsum(fired.sum(axis=1))
    return seg.astype(np.int32), rule.astype(np.int32), first


def thirty_two():
    return [b"p%02d;" % i for i in range(32)]


def cut(*pieces):
    """(data, offsets) of segments given as byte strings"""
    off = [0]
    for p in pieces:
        off.append(off[-1] + len(p))
    return b"".join(pieces), off


def case(name, pats, rules, *pieces, whole=False):
    data, off = cut(*pieces)
    return (name, pats, rules, data, None if whole else off)


# (name, patterns, rules (lists of 1-based ids), data, offsets or None)
CASES = [
    case("one-pattern-rule", [b"abc", b"xyz"], [[1]], b"..abc..", whole=True),
    case("two-patterns-in-different-segments", [b"ERROR", b"payment"], [[1, 2]], b"an ERROR here|", b"payment there"),
    case("two-patterns-in-one-segment", [b"ERROR", b"payment"], [[1, 2], [2], [1]], b"nothing|", b"ERROR in payment"),
    case("proper-prefix-never-the-longest", [b"GET", b"GET /admin"], [[1], [2], [1, 2]], b"GET /admin", whole=True),
    case("only-across-a-border", [b"border", b"or"], [[1], [2], [1, 2]], b"xxbor", b"derxx"),
    case("duplicate-lines-lower-id-named", [b"dup", b"other", b"dup"], [[1], [3], [1, 2], [1, 3]], b"a dup and other|", b"dup"),
    case("id-twice-in-a-rule", [b"aa", b"bb"], [[1, 1], [1, 2, 1, 2], [2, 2, 2]], b"aa..|", b"aabb"),
    case("thirty-two-patterns-31-present", thirty_two(), [list(range(1, 33)), list(range(1, 32))], b"".join(thirty_two()[:31]), whole=True),
    case("thirty-two-patterns-all-present", thirty_two(), [list(range(1, 33)), list(range(1, 32))],
         b"junk" + b"".join(reversed(thirty_two())) + b"|", b"".join(thirty_two()[1:])),
    case("empty-segments", [b"a", b"b"], [[1], [2], [1, 2]], b"", b"a", b"", b"", b"bb", b"a", b""),
    case("no-match-at-all", [b"needle", b"pin"], [[1], [2], [1, 2]], b"a haystack without either|", b"and more of it"),
    case("one-segment-without-offsets", [b"ab", b"cd", b"zz"], [[1, 2], [3], [2]], b"cd ab cd", whole=True),
    case("nested-chain", [b"a", b"aa", b"aaa", b"aaaa", b"b"], [[1, 2, 3, 4], [4, 5], [3, 5], [1]], b"aaab|", b"baaaa|", b"b|", b"aa"),
    case("nocase", [b"Error", b"PAYMENT-service", b"get"], [[1, 2], [3], [1, 3]], b"error: Payment-Service down|", b"GET /x eRRoR"),
]


def is_nocase(name):
    return name.startswith("nocase")


def random_case(seed):
    """(patterns, rules, data, offsets): an alphabet of 2 - 3 letters, 2 - 30 patterns of 1 - 8 bytes, 1 - 60 rules of 1 - 4 ids (repeats allowed),
    1 - 4000 bytes cut into segments of 0 - 40 bytes (every third seed: one segment with offsets)"""
    rng = np.random.Generator(np.random.PCG64(7100 + seed))
    letters = np.frombuffer(b"abc", dtype=np.uint8)[:int(rng.integers(2, 4))]
    pats = sorted({rng.choice(letters, size=int(rng.integers(1, 9))).tobytes() for _ in range(int(rng.integers(2, 31)))})
    rules = [[int(i) for i in rng.integers(1, len(pats) + 1, size=int(rng.integers(1, 5)))] for _ in range(int(rng.integers(1, 61)))]
    n = int(rng.choice([1, 2, 17, 300, 4000])) if seed % 4 == 0 else int(rng.integers(1, 4001))
    data = rng.choice(letters, size=n).astype(np.uint8)
    if seed % 3 == 0:
        offsets = [0, n]
    else:
        cuts = [0]
        while cuts[-1] < n:
            cuts.append(min(n, cuts[-1] + int(rng.integers(0, 41))))
        offsets = cuts
    return pats, rules, data, np.array(offsets, dtype=np.uint64)


RANDOM_SEEDS = list(range(24))
