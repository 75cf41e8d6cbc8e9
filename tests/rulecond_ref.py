"""Reference for PFACX_rulesOpenEx (include/pfac_ext.h) that does not call the library: for each segment, member and start s with
piece[s:s + L] == pattern (both folded by the ASCII fold for a caseless set) it applies the window test of the contract -- a = s, or n - s - L with
PFACX_RULE_FROM_END; a >= offset and (depth == 0 or a + L <= offset + depth), in Python's unbounded integers --; a positive member holds if some
occurrence satisfies its window, a PFACX_RULE_NOT member if none does; a rule fires iff every member holds.  Also the case table both test files
share, the builders of the cases that depend on a size of scan_rules.hip, and a seeded random generator.  Test infrastructure only."""
import numpy as np

from tests import rules_ref

NOT, FROM_END = 1, 2                # PFACX_RULE_NOT, PFACX_RULE_FROM_END
MAX = 0xFFFFFFFF
MEMBER = np.dtype([("pattern", "<i4"), ("flags", "<u4"), ("offset", "<u4"), ("depth", "<u4")])      # PFACX_rule_member_t


def M(pattern, flags=0, offset=0, depth=0):
    """one member: (1-based pattern id, flags, offset, depth)"""
    return (pattern, flags, offset, depth)


def satisfies(s, length, n, flags, offset, depth):
    """the window test of the contract for the occurrence at segment-relative s, of `length` bytes, in a segment of n bytes"""
    a = n - s - length if flags & FROM_END else s
    return a >= offset and (depth == 0 or a + length <= offset + depth)


def member_holds(pat, piece, flags, offset, depth):
    n, length = len(piece), len(pat)
    some = False
    s = piece.find(pat) if length else -1
    while s >= 0 and not some:
        some = satisfies(s, length, n, flags, offset, depth)
        s = piece.find(pat, s + 1)
    return some != bool(flags & NOT)


def fired_py(pats, rules, data, offsets=None, nocase=False):
    """(seg[], rule[], segFirst[]) of the fired list: pats[i] is pattern id i + 1, rules a list of member lists (M), offsets numSegments + 1 byte
    offsets (None: one segment)"""
    data = bytes(data)
    offsets = [0, len(data)] if offsets is None else [int(o) for o in offsets]
    if nocase:
        data, pats = rules_ref.fold(data), [rules_ref.fold(p) for p in pats]
    seg, rule, first = [], [], []
    for k in range(len(offsets) - 1):
        first.append(len(seg))
        piece = data[offsets[k]:offsets[k + 1]]
        holds = {}                                                          # by (pattern bytes, flags, offset, depth): duplicate lines are one pattern
        for r, members in enumerate(rules):
            ok = True
            for (i, flags, offset, depth) in members:
                key = (pats[i - 1], flags, offset, depth)
                if key not in holds:
                    holds[key] = member_holds(pats[i - 1], piece, flags, offset, depth)
                if not holds[key]:
                    ok = False
                    break
            if ok:
                seg.append(k)
                rule.append(r)
    first.append(len(seg))
    return np.array(seg, dtype=np.int32), np.array(rule, dtype=np.int32), np.array(first, dtype=np.uint64)


def csr(rules):
    """(rule_off, members) as PFACX_rulesOpenEx takes them"""
    off = np.zeros(len(rules) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in rules])
    flat = np.array([tuple(m) for r in rules for m in r], dtype=MEMBER)
    return off, flat


def plain(rules):
    """lists of ids -> lists of members {id, 0, 0, 0}"""
    return [[M(i) for i in r] for r in rules]


def pairs(fired):
    return list(zip(fired[0].tolist(), fired[1].tolist()))


GUARD = 16


def host_fired(r, data, offsets, capacity=None, null_arrays=False):
    """match_host over poisoned arrays with guard words behind capacity and behind segFirst -> (status, (seg, rule, segFirst), full count); the
    input must stay untouched.  capacity None: the count query first, as a caller would.  null_arrays: capacity 0 and no arrays at all"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy() if not isinstance(data, np.ndarray) else data.copy()
    keep = buf.copy()
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uintp)
    segs = 1 if off is None else off.size - 1
    optr = None if off is None else off.ctypes.data
    if capacity is None:
        _, capacity = r.match_host(buf.ctypes.data, buf.size, optr, segs, None, None, 0, None, check=False)
    seg, rule = (np.full(capacity + GUARD, -7, dtype=np.int32) for _ in range(2))
    first = np.full(segs + 1 + GUARD, 0xDEAD, dtype=np.uintp)
    st, n = r.match_host(buf.ctypes.data if buf.size else seg.ctypes.data, buf.size, optr, segs, None if null_arrays else seg.ctypes.data,
                         None if null_arrays else rule.ctypes.data, capacity, first.ctypes.data, check=False)
    assert np.array_equal(buf, keep), "the caller's input was modified"
    k = min(n, capacity)
    assert np.all(seg[k:] == -7) and np.all(rule[k:] == -7), "wrote behind the list or behind capacity"
    assert np.all(first[segs + 1:] == 0xDEAD), "wrote behind segFirst"
    return st, (seg[:k].copy(), rule[:k].copy(), first[:segs + 1].copy()), n


def check_forms(fired, want, what):
    """fired(capacity, null_arrays) -> (status, (seg, rule, segFirst), count): the whole list, the list truncated at half its length, the count query"""
    from pfac_amd import api
    TRUNCATED = api.STATUS.OUTPUT_TRUNCATED
    total = int(want[0].size)
    st, got, n = fired(None, False)
    assert (st, n) == (0, total), f"{what}: status {st}, {n} fired, want {total}"
    rules_ref.same(got, want, what)
    half = total // 2
    if half < total:
        st, got, n = fired(half, False)
        assert (st, n) == (TRUNCATED, total), f"{what}/capacity {half}: status {st}, {n} fired, want {total}"
        rules_ref.same(got, (want[0][:half], want[1][:half], want[2]), f"{what}/capacity {half}")
    st, got, n = fired(0, True)
    assert (st, n) == (TRUNCATED if total else 0, total), f"{what}/count query: status {st}, {n} fired, want {total}"
    rules_ref.same(got, (want[0][:0], want[1][:0], want[2]), f"{what}/count query")


def case(name, pats, rules, *pieces, whole=False):
    data, off = rules_ref.cut(*pieces)
    return (name, pats, rules, data, None if whole else off)


def at(s, pat=b"abc", n=12):
    """a segment of n dots with pat at s"""
    return b"." * s + pat + b"." * (n - s - len(pat))


# one pattern of 3 bytes in segments of 12: a = s from the start, a = 9 - s from the end
EDGE_STARTS = [0, 1, 2, 3, 4, 5, 6, 7, 9]
EDGE_RULES = [
    [M(1, 0, 4, 5)],                    # 0: 4 <= s, s + 3 <= 9: s = 4, 5, 6
    [M(1, FROM_END, 4, 5)],             # 1: 4 <= 9 - s <= 6: s = 3, 4, 5
    [M(1, 0, 4, 0)],                    # 2: depth 0: no upper bound: s >= 4
    [M(1, 0, MAX, MAX)],                # 3: nothing, and no wrap
    [M(1, 0, 0, 3)],                    # 4: startswith: s = 0 alone
    [M(1, FROM_END, 0, 3)],             # 5: endswith: s = 9 alone
    [M(1, FROM_END, MAX, MAX)],         # 6: nothing
    [M(1, 0, MAX, 0)],                  # 7: nothing
    [M(1, 0, 0, MAX)],                  # 8: everything
    [M(1, 0, 1, MAX)],                  # 9: s >= 1: 1 + MAX wraps to 0 in 32 bits
    [M(1, FROM_END, 4, 0)],             # 10: 9 - s >= 4
]

THIRTY_TWO = rules_ref.thirty_two()
RULE_32 = [M(i) for i in range(1, 28)] + [M(i, NOT) for i in range(28, 33)]           # 32 members, 5 of them negated

TRIP = 256                              # scan_rules.hip: kRulesBlockPairs
BEYOND_TRIP = b"ab" * 300 + b"zz" + b"ab" * 10                                        # pair number 300 is the only zz, at byte 600

CASES = [
    case("window-edges", [b"abc"], EDGE_RULES, *[at(s) for s in EDGE_STARTS]),
    case("window-edges-one-segment", [b"abc"], EDGE_RULES, at(4), whole=True),
    case("chain-member-decides", [b"GET", b"GET /admin"],
         [[M(1, 0, 0, 3)], [M(2, 0, 0, 3)], [M(2, NOT, 0, 3), M(1)], [M(2, 0, 0, 10)], [M(1, NOT, 0, 3), M(2)]], b"GET /admin", whole=True),
    case("nested-chain-a-window-per-member", [b"a", b"aa", b"aaa", b"aaaa", b"b"],
         [[M(1, 0, 0, 1), M(2, 0, 0, 2), M(3, 0, 0, 3), M(4, 0, 0, 4)], [M(1, FROM_END, 0, 1), M(4, 0, 0, 4)], [M(4, 0, 1, 0), M(1)],
          [M(3, 0, 1, 3), M(1, NOT | FROM_END, 0, 1)], [M(2, FROM_END, 0, 2), M(3, NOT, 0, 3)], [M(4, NOT), M(3, 0, 0, 0), M(1, 0, 3, 1)]],
         b"aaaa", b"baaa", b"aaab", b"baaaa", b"aaa", b"aa", b"b"),
    case("second-segment-and-a-border", [b"bor", b"border", b"abc"],
         [[M(1, FROM_END, 0, 3)], [M(2)], [M(3, 0, 4, 5)], [M(1, 0, 2, 3), M(2, NOT)], [M(1, 0, 7, 0)]],
         b"xxbor", b"derxx", at(4), at(7), b"..border", b"bor"),
    case("negation", [b"ok", b"bad", b"x"],
         [[M(1), M(2, NOT)], [M(1), M(2, NOT, 0, 3)], [M(1, 0, 0, 2), M(1, NOT | FROM_END, 0, 2)], [M(3), M(1, NOT), M(2, NOT)],
          [M(1), M(1, NOT)]],
         b"ok...", b"ok bad", b"ok", b"bad", b"okok", b"bad ok", b"x", b"x ok", b"", b"bad"),
    case("thirty-two-members-5-negated", THIRTY_TWO, [RULE_32, RULE_32[:27]],
         b"".join(THIRTY_TWO[:27]), b"".join(THIRTY_TWO[:27]) + THIRTY_TWO[29], b"".join(THIRTY_TWO[:26]), b"".join(THIRTY_TWO[27:])),
    case("beyond-one-trip", [b"ab", b"zz", b"q"],
         [[M(1), M(2, NOT)], [M(1), M(2, 0, 600, 2)], [M(2, 0, 0, 600)], [M(1), M(2, FROM_END, 20, 2)], [M(1), M(2, NOT, 601, 0)]],
         b"ab" * 311, BEYOND_TRIP, b"q", BEYOND_TRIP),
    case("beyond-one-trip-one-segment", [b"ab", b"zz", b"q"], [[M(1), M(2, NOT)], [M(1), M(2, 0, 600, 2)], [M(2, 0, 0, 600)]], BEYOND_TRIP, whole=True),
    case("nocase-window", [b"Error", b"get"], [[M(2, 0, 0, 3), M(1, NOT)], [M(1, FROM_END, 0, 5)], [M(2, 0, 1, 0)]],
         b"GET /x", b"get eRRoR", b" GeT", b"ERROR get error"),
]

SPELLED_OUT = {         # the answers the issue spells out, as (segment, rule) pairs of the cases above restricted to the rules named
    "window-edges": {0: [4, 5, 6], 1: [3, 4, 5], 3: [], 4: [0], 5: [8]},              # rule -> the segments (indices into EDGE_STARTS) that fire
    "chain-member-decides": {0: [0], 1: [], 2: [0]},
}


def is_nocase(name):
    return name.startswith("nocase")


WINDOW = 8192                           # scan_rules.hip: kRulesWindow


def window_case():
    """8 200 rules; the conditioned ones at 8 191, 8 192 and 8 199.  Pattern 1's only memberships are rule 8 191 -- a window that `key` at 0 fails --
    and rules 8 192 and 8 199 in window 1: a segment that is `key` alone has nothing to OR in window 0 and must still visit window 1"""
    pats = [b"key", b"fill", b"no"]
    rules = [[M(2)] for _ in range(8200)]
    rules[8191] = [M(1, 0, 5, 0)]
    rules[8192] = [M(1, 0, 0, 3)]
    rules[8199] = [M(1), M(2, NOT)]
    return case("beyond-one-window", pats, rules, b"key", b".....key", b"key fill", b"fill", b"no")


TOUCHED = 1024                          # scan_rules.hip: kRulesTouched


def touched_case():
    """one segment touches 1 100 rules of window 0, negated members among them: the sweep over the whole table, with m == need"""
    pats = [b"x", b"y", b"z"]
    rules = [[[M(1), M(2, NOT)], [M(1), M(2)], [M(1, 0, 1, 0)], [M(1), M(2, NOT, 0, 1)]][r % 4] for r in range(1100)] + [[M(3)]]
    return case("touched-list-overflow", pats, rules, b"x", b"xy", b"yx", b"y", b"z")


def clean_state_case(grid):
    """segment 0 sets only the negated bit of rule 1 and half of rule 0; segment `grid` -- the same block's next one -- would complete rule 0 and
    have rule 1 vetoed by what was left behind"""
    pats = [b"x", b"y", b"z"]
    rules = [[M(1), M(2)], [M(3), M(2, NOT)], [M(1, 0, 0, 1), M(2, NOT, 1, 0)]]
    return case("clean-state", pats, rules, *([b"y"] + [b""] * (grid - 1) + [b"xz"] + [b"y"] * 3 + [b"xzy"]))


def random_case(seed):
    """(patterns, rules, data, offsets) in the style of rules_ref.random_case: an alphabet of 2 - 3 letters, 2 - 30 patterns of 1 - 8 bytes, 1 - 60
    rules of 1 - 4 members -- flags drawn from {0, NOT, FROM_END, NOT | FROM_END} (the first member of a rule is positive), offset in 0 .. 12,
    depth in {0, 1 .. 12} --, 1 - 4000 bytes cut into segments of 0 - 40 bytes (every third seed: one segment with offsets)"""
    rng = np.random.Generator(np.random.PCG64(9300 + seed))
    letters = np.frombuffer(b"abc", dtype=np.uint8)[:int(rng.integers(2, 4))]
    pats = sorted({rng.choice(letters, size=int(rng.integers(1, 9))).tobytes() for _ in range(int(rng.integers(2, 31)))})
    rules = []
    for _ in range(int(rng.integers(1, 61))):
        members = []
        for j in range(int(rng.integers(1, 5))):
            flags = (NOT if j > 0 and rng.integers(0, 3) == 0 else 0) | (FROM_END if rng.integers(0, 3) == 0 else 0)
            depth = 0 if rng.integers(0, 3) == 0 else int(rng.integers(1, 13))
            members.append(M(int(rng.integers(1, len(pats) + 1)), flags, int(rng.integers(0, 13)), depth))
        rules.append(members)
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


RANDOM_SEEDS = list(range(16))
