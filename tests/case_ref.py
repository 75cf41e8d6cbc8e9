"""References for the case calls (PFACX_case*: per-pattern case sensitivity over a caseless set) that share no code with the library.

case_brute          the definition of include/pfac_ext.h, line by line: the distinct patterns (same flag, same bytes -- folded bytes for a caseless
                    line -- are one pattern under the highest id), every position of every pattern (bytes.find from each start: in the caller's
                    bytes for a sensitive pattern, in the folded ones for a caseless one), then the two orderings
case_naive          the same as two nested loops over (position, line), for the small cases
case_re             Python's re in bytes mode: each pattern as a lookahead, a caseless one inside a scoped (?i:...), per position
All return (pos, ids) int32: ascending position, then length descending, then id descending; all_matches=False keeps the first pair of a position.
`sensitive` is the flag of every line, line 1 first.  Test infrastructure only."""

import re

import numpy as np

from tests.spans_ref import fold


def distinct_patterns(pats, sensitive):
    """(flag, bytes as they are compared) -> the highest id: what is reported"""
    found = {}
    for k, (pat, s) in enumerate(zip(pats, sensitive)):
        found[(bool(s), bytes(pat) if s else fold(pat))] = k + 1
    return found


def flags_by_id(sensitive):
    """the array PFACX_caseOpen takes: indexed by id, entry 0 unused"""
    return np.array([0] + [1 if s else 0 for s in sensitive], dtype=np.uint8)


def _ordered(found, all_matches):
    found.sort()
    if not all_matches:
        found = [f for k, f in enumerate(found) if k == 0 or found[k - 1][0] != f[0]]
    return np.array([f[0] for f in found], dtype=np.int32), np.array([-f[2] for f in found], dtype=np.int32)


def case_brute(pats, sensitive, data, all_matches=False):
    raw = bytes(data)
    folded = fold(raw)
    found = []                                                  # (position, -length, -id)
    for (s, text), pid in distinct_patterns(pats, sensitive).items():
        hay = raw if s else folded
        at = hay.find(text)
        while at >= 0:
            found.append((at, -len(text), -pid))
            at = hay.find(text, at + 1)
    return _ordered(found, all_matches)


def case_naive(pats, sensitive, data, all_matches=False):
    raw = bytes(data)
    n = len(raw)
    reported = set(distinct_patterns(pats, sensitive).values())
    found = []
    for p in range(n):
        for k, (pat, s) in enumerate(zip(pats, sensitive)):
            if k + 1 not in reported or p + len(pat) > n:
                continue
            piece = raw[p:p + len(pat)]
            if (piece == bytes(pat)) if s else (fold(piece) == fold(pat)):
                found.append((p, -len(pat), -(k + 1)))
    return _ordered(found, all_matches)


def case_re(pats, sensitive, data, all_matches=False):
    raw = bytes(data)
    found = []
    for (s, _), pid in distinct_patterns(pats, sensitive).items():
        text = re.escape(bytes(pats[pid - 1]))
        rx = re.compile(b"(?=" + (text if s else b"(?i:" + text + b")") + b")", re.S)
        found.extend((m.start(), -len(pats[pid - 1]), -pid) for m in rx.finditer(raw))
    return _ordered(found, all_matches)


def max_per_position(pats, sensitive):
    """the largest ALL list one position can have: over the folded texts, the distinct patterns among the lines whose folded text is a prefix of it"""
    keys = list(distinct_patterns(pats, sensitive))
    texts = {fold(pats[k]) for k in range(len(pats))}
    return max([sum(1 for _, text in keys if t.startswith(fold(text))) for t in texts] or [1])


def same(got, want, what):
    (gp, gi), (wp, wi) = got, want
    gp, gi, wp, wi = (np.asarray(a, dtype=np.int64) for a in (gp, gi, wp, wi))
    assert gp.size == wp.size, f"{what}: {gp.size} pairs, want {wp.size}"
    bad = np.flatnonzero((gp != wp) | (gi != wi))
    if bad.size:
        k = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} pairs differ, first at {k}: got ({gi[k]}, {gp[k]}) want ({wi[k]}, {wp[k]})")


# ---------------------------------------------------------------- the compare edges

EDGE_LENGTHS = [1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 64]        # 64: the set's longest pattern


def edge_pattern(length):
    """one letter per length, case alternating from lower: no pattern of the set is a prefix of another"""
    letter = b"abcdefghijklmnopqrstuvwxyz"[EDGE_LENGTHS.index(length)]
    return bytes(letter ^ (0x20 if i & 1 else 0) for i in range(length))


def flipped(pat, at):
    return pat[:at] + bytes([pat[at] ^ 0x20]) + pat[at + 1:]


def edge_input():
    """every pattern as it is, then with the case of only its first byte, only its last byte and only a byte of a middle dword flipped; the pieces
    have many lengths, so the candidates start at every residue mod 4; the buffer ends with an exact match, behind a candidate cut short by n"""
    pieces = []
    for k, length in enumerate(EDGE_LENGTHS):
        pat = edge_pattern(length)
        four = [pat, flipped(pat, 0), flipped(pat, length - 1), flipped(pat, min(length - 1, 4 * (length // 8) + 1))]
        pieces += four[-(k % 4):] + four[:-(k % 4)] + [b"-" * (k % 3)]
    longest = edge_pattern(EDGE_LENGTHS[-1])
    return b" ".join(pieces) + b" " + longest[:-1] + b" " + edge_pattern(33)


EDGE_PATS = [edge_pattern(length) for length in EDGE_LENGTHS]

# ---------------------------------------------------------------- the case table

# (name, patterns, the flag of every line, input)
CASES = [
    ("three-variants", [b"GET", b"get", b"Get"], [1, 1, 0], b"GET get gEt Get"),
    ("exact-duplicates-of-each-kind", [b"ab", b"AB", b"ab", b"Ab", b"aB", b"AB"], [1, 1, 1, 0, 0, 1], b"ab AB Ab aB"),
    ("a-class-of-one-caseless-line", [b"Key", b"other"], [0, 1], b"key KEY kEy ke Key other OTHER"),
    ("longest-sensitive-fails-or-passes-over-a-caseless-prefix", [b"foo", b"fooBar"], [0, 1], b"foobar fooBar FOOBAR fooBa"),
    ("every-member-fails", [b"Ab", b"AbC"], [1, 1], b"abc ABC aBc xab"),
    ("sensitive-prefix-caseless-longer", [b"Foo", b"foobar"], [1, 0], b"FooBAR foobar Foo fOO fooba"),
    ("three-deep-chain", [b"a", b"Ab", b"ab", b"aBc", b"ABC", b"abc"], [0, 1, 0, 1, 1, 1], b"abc ABC aBc Abc aBC ab a"),
    ("a-match-ends-at-n", [b"Tail", b"TailXY"], [1, 1], b"TailXY TailX tail Tail"),
    ("a-candidate-runs-past-n", [b"Tail", b"TailXY"], [1, 0], b"xx Tail tailxy TAILX"),
    ("fold-edges", [b"@a[", b"`A{", b"\xc1b", b"\xe1B", b"z@", b"Z`"], [0, 1, 0, 1, 0, 1],
     b"@A[ @a[ `a{ `A{ \xc1B \xc1b \xe1b \xe1B \xe1\x42 Z` z` z@ Z@ {a[ [A{"),
    ("compare-edges", EDGE_PATS, [1] * len(EDGE_PATS), edge_input()),
    ("compare-edges-under-a-caseless-twin", EDGE_PATS + [fold(p) for p in EDGE_PATS], [1] * len(EDGE_PATS) + [0] * len(EDGE_PATS), edge_input()),
]
# what the definition gives, worked out by hand: name -> ((ids, positions) of the list, of ALL)
WANT = {
    "three-variants": (([3, 3, 3, 3], [0, 4, 8, 12]), ([3, 1, 3, 2, 3, 3], [0, 0, 4, 4, 8, 12])),
    "exact-duplicates-of-each-kind": (([5, 6, 5, 5], [0, 3, 6, 9]), ([5, 3, 6, 5, 5, 5], [0, 0, 3, 3, 6, 9])),
    "every-member-fails": (([], []),) * 2,
    "longest-sensitive-fails-or-passes-over-a-caseless-prefix": (([1, 2, 1, 1], [0, 7, 14, 21]), ([1, 2, 1, 1, 1], [0, 7, 7, 14, 21])),
    "sensitive-prefix-caseless-longer": (([2, 2, 1], [0, 7, 14]), ([2, 1, 2, 1], [0, 0, 7, 14])),
}


def test_the_references_agree_on_every_case():
    for name, pats, sens, data in CASES:
        for all_matches in (False, True):
            brute = case_brute(pats, sens, data, all_matches)
            same(case_naive(pats, sens, data, all_matches), brute, f"{name}/all {all_matches}: the nested loops against brute force")
            same(case_re(pats, sens, data, all_matches), brute, f"{name}/all {all_matches}: re against brute force")
            if name in WANT:
                ids, pos = WANT[name][1 if all_matches else 0]
                same(brute, (pos, ids), f"{name}/all {all_matches}: brute force against the list worked out by hand")
    # the edges hold what they are meant to: each sensitive pattern occurs exactly where it stands unflipped
    pos, ids = case_brute(EDGE_PATS, [1] * len(EDGE_PATS), edge_input(), True)
    assert np.bincount(ids, minlength=len(EDGE_PATS) + 1).tolist() == [0] + [1] * 8 + [1, 1, 2, 1]
    assert int(pos[-1]) + 33 == len(edge_input()), "the buffer ends with a match"
    assert set(int(p) & 3 for p in pos) == {0, 1, 2, 3}, "candidates at every residue mod 4"
    assert max_per_position([b"GET", b"get", b"Get"], [1, 1, 0]) == 3 and max_per_position(*CASES[6][1:3]) == 6
