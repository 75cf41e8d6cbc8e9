"""Reference for PFACX_rulesOpenSeq (include/pfac_ext.h) that does not call the library and does not use the library's frontier method: per segment
and rule it lists every occurrence of every chain member with bytes.find, keeps those that satisfy the member's own window (the test of
tests/rulecond_ref.py) and decides a chain by depth-first search over all assignments, in Python's unbounded integers; the members outside a chain
go through tests/rulecond_ref.py.  For chains whose members have no window of their own the reference is itself checked against Python's `re`
(chain_regex): a regular expression backtracks over all assignments, so the two must agree.  Also the case table both test files share, the
builders of the cases that depend on a size of scan_rules.hip, and a seeded random generator.  Test infrastructure only."""
import functools
import re

import numpy as np

from tests import rulecond_ref as rc
from tests import rules_ref

NOT, FROM_END, RELATIVE = 1, 2, 4       # PFACX_RULE_NOT, PFACX_RULE_FROM_END, PFACX_RULE_RELATIVE
MAX = 0xFFFFFFFF
MEMBER = np.dtype([("pattern", "<i4"), ("flags", "<u4"), ("offset", "<u4"), ("depth", "<u4"), ("distance", "<u4"), ("within", "<u4")])  # PFACX_rule_seq_member_t
WINDOW, TOUCHED, TRIP = rc.WINDOW, rc.TOUCHED, rc.TRIP


def S(pattern, flags=0, offset=0, depth=0):
    """a member without PFACX_RULE_RELATIVE"""
    return (pattern, flags, offset, depth, 0, 0)


def R(pattern, distance=0, within=0, flags=0, offset=0, depth=0):
    """a member tied to the one in front of it"""
    return (pattern, flags | RELATIVE, offset, depth, distance, within)


def split(members):
    """(chains, singles) of one rule: a chain is a maximal run "member without RELATIVE, then RELATIVE members" of two members or more"""
    chains, singles = [], []
    for j, m in enumerate(members):
        if m[1] & RELATIVE:
            chains[-1].append(m)
        elif j + 1 < len(members) and members[j + 1][1] & RELATIVE:
            chains.append([m])
        else:
            singles.append(m)
    return chains, singles


def occurrences(pat, piece, flags, offset, depth):
    """the starts of pat in piece that satisfy the member's own window"""
    out, n = [], len(piece)
    s = piece.find(pat) if pat else -1
    while s >= 0:
        if rc.satisfies(s, len(pat), n, flags & FROM_END, offset, depth):
            out.append(s)
        s = piece.find(pat, s + 1)
    return out


def chain_holds(pats, chain, piece):
    """depth-first search over all assignments o_0 .. o_c (a link that failed behind one predecessor end is not searched from there again)"""
    occ = [occurrences(pats[m[0] - 1], piece, m[1], m[2], m[3]) for m in chain]
    lens = [len(pats[m[0] - 1]) for m in chain]

    @functools.lru_cache(maxsize=None)
    def search(j, e):
        """can links j .. c be placed behind a predecessor that ends at e?"""
        if j == len(chain):
            return True
        _, _, _, _, distance, within = chain[j]
        for s in occ[j]:
            if s >= e + distance and (within == 0 or s + lens[j] <= e + within) and search(j + 1, s + lens[j]):
                return True
        return False

    return any(search(1, s + lens[0]) for s in occ[0])


def chain_regex(pats, chain, n):
    """the chain as a regular expression over a piece of n bytes, for a chain whose members have no window of their own; None where one has"""
    if any(m[1] & ~RELATIVE or m[2] or m[3] for m in chain):
        return None
    never = b"(?!)"
    expr = re.escape(pats[chain[0][0] - 1])
    for m in chain[1:]:
        pat, distance, within = pats[m[0] - 1], m[4], m[5]
        if distance > n or (within and within < len(pat)):
            return re.compile(never)
        gap = b"{%d,}" % distance if within == 0 else b"{%d,%d}" % (distance, min(within - len(pat), n))
        if within and within - len(pat) < distance:
            return re.compile(never)
        expr += b"(?s:." + gap + b")" + re.escape(pat)
    return re.compile(expr)


def fired_py(pats, rules, data, offsets=None, nocase=False, check_re=True):
    """(seg[], rule[], segFirst[]) of the fired list: pats[i] is pattern id i + 1, rules a list of member lists (S, R), offsets numSegments + 1 byte
    offsets (None: one segment).  check_re: every chain without windows of its own is also decided by `re`, and the two must agree"""
    data = bytes(data)
    offsets = [0, len(data)] if offsets is None else [int(o) for o in offsets]
    if nocase:
        data, pats = rules_ref.fold(data), [rules_ref.fold(p) for p in pats]
    split_rules = [split(members) for members in rules]
    seg, rule, first = [], [], []
    for k in range(len(offsets) - 1):
        first.append(len(seg))
        piece = data[offsets[k]:offsets[k + 1]]
        for r, (chains, singles) in enumerate(split_rules):
            ok = all(rc.member_holds(pats[i - 1], piece, flags, offset, depth) for (i, flags, offset, depth, _, _) in singles)
            for chain in chains:
                if not ok:
                    break
                ok = chain_holds(pats, chain, piece)
                if check_re:
                    expr = chain_regex(pats, chain, len(piece))
                    assert expr is None or (expr.search(piece) is not None) == ok, (chain, piece, ok)
            if ok:
                seg.append(k)
                rule.append(r)
    first.append(len(seg))
    return np.array(seg, dtype=np.int32), np.array(rule, dtype=np.int32), np.array(first, dtype=np.uint64)


def and_stage(rules):
    """the rules with every member made an ordinary conditioned one: what fires here is a candidate"""
    return [[(i, flags & ~RELATIVE, offset, depth) for (i, flags, offset, depth, _, _) in members] for members in rules]


def csr(rules):
    """(rule_off, members) as PFACX_rulesOpenSeq takes them"""
    off = np.zeros(len(rules) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in rules])
    flat = np.array([tuple(m) for r in rules for m in r], dtype=MEMBER)
    return off, flat


def widen(rules):
    """lists of PFACX_rule_member_t tuples -> the same members as PFACX_rule_seq_member_t tuples"""
    return [[tuple(m) + (0, 0) for m in r] for r in rules]


def links(rules):
    """K of the header's MEMORY paragraph: the members of all chains"""
    return sum(len(c) for members in rules for c in split(members)[0])


case = rc.case
is_nocase = rc.is_nocase

THIRTY_TWO = rules_ref.thirty_two()     # 32 patterns of 4 bytes
CHAIN_32 = [S(1)] + [R(i) for i in range(2, 33)]
ADJACENT_32 = [S(1)] + [R(i, 0, 4) for i in range(2, 33)]
JOINED_32 = b"".join(THIRTY_TWO)

# pair number 0 is A, 256 is B, 512 is C; every x is a pair of its own: segments of 257 and 513 pairs, the links in different trips of 256
SEG_257 = b"A" + b"x" * 255 + b"B"
SEG_513 = SEG_257 + b"x" * 255 + b"C"

CASES = [
    # greedy traps
    case("trap-only-the-second-A-is-near-enough", [b"AA", b"BB"], [[S(1), R(2, 0, 4)], [S(1), R(2, 0, 3)]], b"AA......AA.BB", b"AA......AA..BB"),
    case("trap-only-the-second-B-is-far-enough", [b"AA", b"BB"], [[S(1), R(2, 5, 0)], [S(1), R(2, 10, 0)]], b"AA.BB......BB", b"AA.BB.BB"),
    case("trap-the-latest-A-leads-nowhere", [b"XX", b"AA", b"BB"], [[S(1), R(2), R(3, 0, 4)]], b"XX.AA.BB.AA", b"XX.AA..BB.AA", b"XX.BB.AA"),
    case("trap-the-earliest-A-leads-nowhere", [b"XX", b"AA", b"BB"], [[S(1), R(2), R(3, 0, 4)]], b"XX.AA......AA.BB", b"XX.AA......AA...BB"),
    case("trap-the-near-A-is-not-reachable", [b"XX", b"AA", b"BB"], [[S(1), R(2, 0, 5), R(3, 0, 4)], [S(1), R(2, 0, 12), R(3, 0, 4)]],
         b"XX.AA.....AA.BB", b"XX.AA.BB..AA.BB"),
    # bounds
    case("bounds", [b"ab", b"cde"],
         [[S(1), R(2, 0, 2)], [S(1), R(2, 0, 3)], [S(1), R(2, 100, 0)], [S(1), R(2, MAX, MAX)], [S(1), R(2, 0, 0)], [S(1), R(2, 1, 0)],
          [S(1), R(2, MAX, 0)], [S(1), R(2, 0, MAX)], [S(1), R(2, 1, 4)], [S(1), R(2, 2, 4)], [S(1), R(2, 6, 0)], [S(1), R(2, 7, 0)]],
         b"abcde", b"ab.cde", b"cdeab", b"ab......cde", b"ab", b"cde"),
    case("same-pattern-twice", [b"aa"], [[S(1), R(1)], [S(1), R(1), R(1)], [S(1), R(1, 1, 0)]], b"aaa", b"aaaa", b"aaaaa", b"aaaaaa", b"aa"),
    case("proper-prefix-member", [b"foo", b"bar", b"foobar"],
         [[S(1), R(2)], [S(1), R(2, 1, 0)], [S(3), R(2)], [S(3), R(2, 0, 3)], [S(1), R(3)], [S(1), R(2, 0, 3), S(3, NOT)]],
         b"foobar bar", b"foobar", b"foo bar", b"foobarbar"),
    case("own-window-on-a-relative-member", [b"ab", b"cd"],
         [[S(1), R(2, 0, 0, 0, 5, 0)], [S(1), R(2, 0, 4, 0, 5, 0)], [S(1), R(2, 0, 0, FROM_END, 0, 2)], [S(1, 0, 0, 2), R(2)],
          [S(1, FROM_END, 0, 2), R(2)], [S(1), R(2, 0, 0, 0, 0, 5)], [S(1, 0, 1, 0), R(2, 0, 0, FROM_END, 1, 0)]],
         b"ab.cd.cd", b"ab.cd.cd.", b".ab.cd", b"cd.ab", b"ab....cd"),
    case("two-chains-share-an-occurrence", [b"a", b"b", b"c"],
         [[S(1), R(2), S(1), R(3)], [S(1), R(2), S(2), R(3)], [S(1), R(2, 1, 0), S(3), S(1), R(3, 0, 2)]],
         b"a.b.c", b"a.b", b"abc", b"b.a.c", b"c.a.b", b"ac.b"),
    case("chain-and-a-negated-member", [b"GET", b"admin", b"local"], [[S(1, 0, 0, 3), R(2, 1, 12), S(3, NOT)], [S(3, NOT), S(1), R(2)]],
         b"GET /admin", b"GET /admin local", b"GET /x/y/z/w/admin", b"admin GET", b"local GET admin"),
    case("thirty-two-member-chain", THIRTY_TWO, [CHAIN_32, ADJACENT_32, CHAIN_32[:31] + [R(32, 1, 0)]],
         JOINED_32, JOINED_32[:-4] + b"." + THIRTY_TWO[31], b"".join(reversed(THIRTY_TWO)), JOINED_32[:60] + b"junk" + JOINED_32[60:],
         JOINED_32[:-4]),
    case("nocase-chain", [b"User-Agent:", b"SQLmap", b"x"], [[S(1, 0, 0, 11), R(2, 1, 0)], [S(2), R(3)]],
         b"user-agent: sqlMAP/1.0", b"USER-AGENT:sqlmap", b"sqlmap User-Agent:", b"SqlMap X"),
    # segments and offsets
    case("across-a-border-and-empty-segments", [b"ab", b"cd"], [[S(1), R(2)], [S(2), R(1)]], b"ab..c", b"d", b"", b"", b"ab.cd", b"", b"cd", b"ab", b"cdab"),
    case("one-segment-without-offsets", [b"ab", b"cd"], [[S(1), R(2, 2, 6)], [S(2), R(1)]], b"cd ab  cd", whole=True),
    # sized by the kernel's trip
    case("links-in-different-trips", [b"x", b"A", b"B", b"C"],
         [[S(2), R(3, 255, 0)], [S(2), R(3, 256, 0)], [S(2), R(3, 0, 256)], [S(2), R(3, 0, 255)], [S(2), R(3), R(4, 255, 256)],
          [S(2), R(3), R(4, 256, 0)], [S(1), R(1, 509, 0)], [S(1), R(1, 510, 0)], [S(1), R(3, 0, 2), R(1, 0, 1), R(4, 254, 0)],
          [S(2), R(1, 254, 0), R(3)], [S(2), R(1, 255, 0), R(3)], [S(1), R(4, 0, 2)]],
         SEG_257, SEG_513, b"x", SEG_513[1:]),
]


def window_case():
    """8 200 rules; chain rules at WINDOW - 1, WINDOW and WINDOW + 1, one that holds and one that fails on each side of the window's border"""
    pats = [b"key", b"fill", b"lock"]
    rules = [[S(2)] for _ in range(WINDOW + 8)]
    rules[WINDOW - 1] = [S(1), R(3)]
    rules[WINDOW] = [S(3), R(1)]
    rules[WINDOW + 1] = [S(1), R(3, 0, 5)]
    return case("chains-beyond-one-window", pats, rules, b"key lock", b"lock key", b"key fill lock", b"fill", b"key", b"keylock")


def touched_case():
    """one segment makes 1 100 rules of window 0 candidates, every second of which fails its verification: the sweep over the whole table, and in
    every word of the bitmap verified and failed candidates side by side"""
    pats = [b"x", b"y", b"z"]
    rules = [[[S(1), R(2)], [S(2), R(1)], [S(1), R(2, 1, 0)], [S(1), S(2)]][r % 4] for r in range(TOUCHED + 76)] + [[S(3)]]
    return case("touched-list-overflow-with-failed-candidates", pats, rules, b"xy", b"yx", b"x.y", b"y", b"z", b"xyx")


def clean_state_case(grid):
    """segment 0 leaves a candidate that fails and half a chain; segment `grid` -- the same block's next one -- must decide from its own pairs"""
    pats = [b"x", b"y", b"z"]
    rules = [[S(1), R(2)], [S(2), R(1)], [S(3), R(1), S(2, NOT)]]
    return case("clean-state-behind-a-failed-candidate", pats, rules, *([b"yx"] + [b""] * (grid - 1) + [b"xy"] + [b"zy"] * 2 + [b"zx", b"yzx"]))


# rule 1 is a candidate on every segment and fails on `xy`, rule 2 is a candidate that holds there: a list cut at 1 or 2 falls between the two
TRUNCATION = case("truncation-between-two-candidates", [b"x", b"y"], [[S(1)], [S(2), R(1)], [S(1), R(2)], [S(2)]], b"xy", b"yx", b"xy")


def random_case(seed):
    """(patterns, rules, data, offsets): an alphabet of 2 - 3 letters, 2 - 12 patterns of 1 - 4 bytes, 4 - 40 rules that are a chain of 2 - 5 links
    with distance in 0 .. 2 and within in {0, len .. len + 12} -- now and then with a window of its own on a link, a member outside the chain in
    front of it or behind it, or a second chain --, 1 - 1500 bytes cut into segments of 0 - 40 bytes (every third seed: one segment of at most 600)"""
    rng = np.random.Generator(np.random.PCG64(9500 + seed))
    letters = np.frombuffer(b"abc", dtype=np.uint8)[:int(rng.integers(2, 4))]
    pats = sorted({rng.choice(letters, size=int(rng.integers(1, 5))).tobytes() for _ in range(int(rng.integers(2, 13)))})

    def chain():
        out = []
        for j in range(int(rng.integers(2, 6))):
            i = int(rng.integers(1, len(pats) + 1))
            flags = FROM_END if rng.integers(0, 8) == 0 else 0
            offset = int(rng.integers(0, 9)) if rng.integers(0, 6) == 0 else 0
            depth = int(rng.integers(1, 30)) if rng.integers(0, 8) == 0 else 0
            if j == 0:
                out.append(S(i, flags, offset, depth))
            else:
                within = 0 if rng.integers(0, 2) == 0 else len(pats[i - 1]) + int(rng.integers(0, 13))
                out.append(R(i, int(rng.integers(0, 3)), within, flags, offset, depth))
        return out

    def single():
        return S(int(rng.integers(1, len(pats) + 1)), NOT if rng.integers(0, 2) else 0, int(rng.integers(0, 5)), 0)

    rules = []
    for _ in range(int(rng.integers(4, 41))):
        members = ([single()] if rng.integers(0, 6) == 0 else []) + chain()
        if rng.integers(0, 6) == 0:
            members += [single()]
        if rng.integers(0, 8) == 0:
            members += chain()
        rules.append(members)
    if seed % 3 == 0:
        n = int(rng.integers(1, 601))
        offsets = [0, n]
    else:
        n = int(rng.integers(1, 1501))
        offsets = [0]
        while offsets[-1] < n:
            offsets.append(min(n, offsets[-1] + int(rng.integers(0, 41))))
    data = rng.choice(letters, size=n).astype(np.uint8)
    return pats, rules, data, np.array(offsets, dtype=np.uint64)


# picked on the CPU so that among the rules that pass the AND stage both outcomes occur (test_ruleseq_host.py asserts it on the reference alone)
RANDOM_SEEDS = [2, 5, 7, 9, 10, 11, 13, 14, 15, 18, 22, 23]
