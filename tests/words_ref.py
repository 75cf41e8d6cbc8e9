"""References for the words calls (PFACX_matchWords* / PFACX_wordsPairsFromDevice) that share no code with the library or with each other.

words_from_result   numpy: a longest-match vector (the oracle's, or spans_ref.brute_result) walked down the prefix table of tests/allmatch_ref.py, each
                    member of a chain tested against the bytes around it; any class
words_re            Python's re in bytes mode, the default class only: (?<![0-9A-Za-z_]) in front of and (?![0-9A-Za-z_]) behind each pattern, overlapping
                    occurrences found through a lookahead
Both return (pos, ids) int32, ascending position, longest pattern first within a position; all_matches=False keeps the first pair of each position.
A class is None (the default [0-9A-Za-z_]) or the bytes that are in it.  Test infrastructure only."""

import re

import numpy as np

from tests import allmatch_ref as am
from tests.spans_ref import brute_result, fold

DEFAULT = b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz_"
EMPTY = b""
FULL = bytes(range(256))


def all_but(excluded):
    return bytes(sorted(set(range(256)) - set(bytes(excluded))))


NOT_NEWLINE = all_but(b"\n")                                    # grep -x
CSV = all_but(b",\n")                                           # whole fields


def members(cls):
    return DEFAULT if cls is None else bytes(cls)


def in_class(cls):
    t = np.zeros(256, dtype=bool)
    t[list(members(cls))] = True
    return t


def words_from_result(result, prefix_table, lengths, data, cls=None, all_matches=False):
    """result: the longest-match vector over `data` (matched however the set matches: folded, for a caseless set); the class is tested on `data` itself.
    prefix_table: (prefixPattern, chainLen) by id; lengths: by id"""
    data = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.asarray(data, dtype=np.uint8)
    n = int(data.size)
    prefix, lengths = np.asarray(prefix_table[0], dtype=np.int64), np.asarray(lengths, dtype=np.int64)
    inw = in_class(cls)
    r = np.asarray(result)
    p = np.flatnonzero(r > 0).astype(np.int64)
    p = p[(p == 0) | ~inw[data[np.maximum(p - 1, 0)]]]          # the byte in front is the same for the whole chain
    q = r[p].astype(np.int64)
    out_p, out_q, out_level = [], [], []
    level = 0
    while p.size:
        e = p + lengths[q]
        ok = (e == n) | ((e < n) & ~inw[data[np.minimum(e, n - 1)]])
        out_p.append(p[ok])
        out_q.append(q[ok])
        out_level.append(np.full(int(ok.sum()), level))
        keep = np.ones(p.size, dtype=bool) if all_matches else ~ok
        p, q = p[keep], prefix[q[keep]]
        p, q = p[q > 0], q[q > 0]
        level += 1
    if not out_p:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    P, Q, L = np.concatenate(out_p), np.concatenate(out_q), np.concatenate(out_level)
    order = np.lexsort((L, P))
    return P[order].astype(np.int32), Q[order].astype(np.int32)


def words_brute(pats, data, cls=None, all_matches=False, nocase=False):
    """words_from_result over the brute-force longest vector"""
    folded = [fold(p) for p in pats] if nocase else [bytes(p) for p in pats]
    prefix, chain, _ = am.prefix_table(folded)
    return words_from_result(brute_result(pats, data, nocase), (prefix, chain), [0] + [len(p) for p in pats], data, cls, all_matches)


def words_re(pats, data, all_matches=False, nocase=False):
    """the default class (it is case-symmetric: the fold of a caseless set changes no byte's membership)"""
    hay = fold(data) if nocase else bytes(data)
    found = []
    for pat, pid in am.pattern_ids([fold(p) for p in pats] if nocase else pats).items():
        rx = re.compile(rb"(?=(?<![0-9A-Za-z_])" + re.escape(pat) + rb"(?![0-9A-Za-z_]))", re.S)
        found.extend((m.start(), -len(pat), pid) for m in rx.finditer(hay))
    found.sort()
    if not all_matches:
        found = [f for k, f in enumerate(found) if k == 0 or found[k - 1][0] != f[0]]
    return np.array([f[0] for f in found], dtype=np.int32), np.array([f[2] for f in found], dtype=np.int32)


def per_pattern_counts(pats, pos_ids):
    return np.bincount(pos_ids[1], minlength=len(pats) + 1).astype(np.uint64)


def same(got, want, what):
    (gp, gi), (wp, wi) = got, want
    gp, gi, wp, wi = (np.asarray(a, dtype=np.int64) for a in (gp, gi, wp, wi))
    assert gp.size == wp.size, f"{what}: {gp.size} pairs, want {wp.size}"
    bad = np.flatnonzero((gp != wp) | (gi != wi))
    if bad.size:
        k = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} pairs differ, first at {k}: got ({gi[k]}, {gp[k]}) want ({wi[k]}, {wp[k]})")


NESTED = [b"a" * k for k in range(1, 9)]                       # a, aa, ..., a x 8
SPACED = [b"a", b"a a", b"a a a", b"a a a a", b"a a a a a"]
# (name, patterns, input, class, caseless): the edge cases of the definition
CASES = [
    ("at-0-and-ends-at-n", [b"foo", b"bar"], b"foo x bar", None, False),
    ("longest-fails-prefix-passes", [b"foo", b"foobar"], b"foo bar foobar foobarx foo", None, False),
    ("every-member-fails", [b"ab", b"abc"], b"xabcd abcd", None, False),
    ("one-byte-patterns", [b"a", b"I", b"-"], b"a I am-a - aa", None, False),
    ("edge-bytes-outside-the-class", [b"-x-", b"+", b"c++"], b"a -x- b-x-c c++ d+e +", None, False),
    ("nested-a", NESTED, b"a" * 5 + b" " + b"a" * 8 + b" " + b"a" * 9 + b".aa", None, False),
    ("fifteen-pairs-in-nine-bytes", SPACED, b"a a a a a", None, False),
    ("empty-class", [b"ab", b"abc", b"b", b"cab"], b"abcab.b abc", EMPTY, False),
    ("empty-class-nested", NESTED, b"b" + b"a" * 11 + b"b" + b"a" * 3, EMPTY, False),
    ("full-class", [b"whole", b"whole buffer", b"buffer"], b"whole buffer", FULL, False),
    ("full-class-nothing", [b"ab", b"b"], b"abab", FULL, False),
    ("grep-x-with-a-last-newline", [b"line", b"line two", b"x"], b"line\nline two\nline twox\nx line\nx\n", NOT_NEWLINE, False),
    ("grep-x-without-a-last-newline", [b"line", b"line two", b"x"], b"x\n\nline two\nline", NOT_NEWLINE, False),
    ("csv-fields", [b"key", b"key1", b"k"], b"key,key1,xkey,k\nkey1x,k,key", CSV, False),
    ("caseless-asymmetric-class", [b"Key", b"KEYS"], b"xKEYx XkeyX akeysa AKeYsA AKEYSa", b"abcdefghijklmnopqrstuvwxyz", True),
    ("caseless-default-class", [b"Needle", b"NEE", b"get"], b"a NEEDLE, nEe-GeT needles Get", None, True),
    ("duplicate-lines", [b"ab", b"cd", b"ab"], b"ab cd abcd ab", None, False),
]
# what the definition gives, worked out by hand: name -> ((ids, positions) of the word list, of ALL)
WANT = {
    "at-0-and-ends-at-n": (([1, 2], [0, 6]),) * 2,
    "longest-fails-prefix-passes": (([1, 2, 1], [0, 8, 23]),) * 2,
    "every-member-fails": (([], []),) * 2,
    "one-byte-patterns": (([1, 2, 1, 3], [0, 2, 7, 9]),) * 2,
    "nested-a": (([5, 8, 2], [0, 6, 25]),) * 2,
    "fifteen-pairs-in-nine-bytes": (([5, 4, 3, 2, 1], [0, 2, 4, 6, 8]),
                                    ([5, 4, 3, 2, 1, 4, 3, 2, 1, 3, 2, 1, 2, 1, 1], [0, 0, 0, 0, 0, 2, 2, 2, 2, 4, 4, 4, 6, 6, 8])),
    "full-class": (([2], [0]),) * 2,
    "full-class-nothing": (([], []),) * 2,
    "grep-x-with-a-last-newline": (([1, 2, 3], [0, 5, 31]),) * 2,
    "grep-x-without-a-last-newline": (([3, 2, 1], [0, 3, 12]),) * 2,
    "csv-fields": (([1, 2, 3, 3, 1], [0, 4, 14, 22, 24]),) * 2,
    "caseless-asymmetric-class": (([1, 2, 1], [7, 20, 27]),) * 2,
    "duplicate-lines": (([3, 2, 3], [0, 3, 11]),) * 2,
}


def test_the_two_references_agree_on_every_case():
    for name, pats, data, cls, nocase in CASES:
        for all_matches in (False, True):
            brute = words_brute(pats, data, cls, all_matches, nocase)
            if cls is None:
                same(words_re(pats, data, all_matches, nocase), brute, f"{name}/all {all_matches}: re against brute force")
            if name in WANT:
                ids, pos = WANT[name][1 if all_matches else 0]
                same(brute, (pos, ids), f"{name}/all {all_matches}: brute force against the list worked out by hand")
        # the empty class: the lists of the calls that know no class
        if cls == EMPTY:
            folded = [fold(p) for p in pats] if nocase else pats
            same(words_brute(pats, data, cls, True, nocase), am.brute_all(folded, np.frombuffer(fold(data) if nocase else data, dtype=np.uint8)), name)
            r = brute_result(pats, data, nocase)
            same(words_brute(pats, data, cls, False, nocase), (np.flatnonzero(r), r[r > 0]), name)
    assert words_brute(SPACED, b"a a a a a", None, True)[0].size == 15
