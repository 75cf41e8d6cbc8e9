"""References for the count calls (PFACX_count*) that share no code with the library or with each other.

counts_py           the all-match list by brute force (tests/allmatch_ref.py: every position, every pattern length, a dict lookup) through np.bincount;
                    longest: the first pair of each position alone
counts_from_result  numpy: np.bincount of a longest-match vector (the oracle's), pushed up the prefix table from the longest chains to the shortest
Both return uint64[F + 1] by pattern id, entry 0 = 0.  Test infrastructure only."""

import numpy as np

from tests import allmatch_ref as am


def fold(b):
    """the ASCII fold of PFACX_READ_NOCASE: 'A'-'Z' -> 'a'-'z', nothing else"""
    return bytes(c + 32 if 65 <= c <= 90 else c for c in bytes(b))


def counts_py(pats, data, nocase=False, longest=False):
    if nocase:
        pats, data = [fold(p) for p in pats], fold(data)
    pos, ids = am.brute_all(pats, np.frombuffer(bytes(data), dtype=np.uint8))
    if longest and pos.size:                                   # the list is longest first within a position
        first = np.ones(pos.size, dtype=bool)
        first[1:] = pos[1:] != pos[:-1]
        ids = ids[first]
    return np.bincount(ids, minlength=len(pats) + 1).astype(np.uint64)


def counts_from_result(result, prefix_table, longest=False):
    """prefix_table: (prefixPattern[F + 1], chainLen[F + 1]) by id, as PFACX_TABLE_PREFIX_PATTERN defines them"""
    prefix, chain = (np.asarray(t) for t in prefix_table)
    r = np.asarray(result)
    counts = np.bincount(r[r > 0], minlength=prefix.size).astype(np.uint64)
    if not longest:
        for i in sorted(range(1, prefix.size), key=lambda i: -int(chain[i])):       # a pattern's count is complete before its prefix takes it
            if prefix[i]:
                counts[prefix[i]] += counts[i]
    return counts


def total_of(result, prefix_table, longest=False):
    """what a count call reports as added: the pairs, or the sum of their chain lengths"""
    r = np.asarray(result)
    r = r[r > 0]
    return int(r.size) if longest else int(np.asarray(prefix_table[1], dtype=np.int64)[r].sum())


def same(got, want, what):
    got, want = np.asarray(got, dtype=np.uint64), np.asarray(want, dtype=np.uint64)
    assert got.size == want.size, f"{what}: {got.size} entries, want {want.size}"
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} counts differ, first at id {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}")


NESTED = [b"a" * k for k in range(1, 9)]                       # a, aa, ..., a x 8: chains of every depth up to 8
# (name, patterns, input): the edge cases of the definition
CASES = [
    ("no-match", [b"ab", b"needle"], b"nothing here"),
    ("one-byte-of-input", [b"a", b"ab"], b"a"),
    ("one-byte-no-match", [b"ab"], b"a"),
    ("a-over-a-run", [b"a"], b"a" * 300),
    ("nested-a-broken-runs", NESTED, b"b" + b"a" * 30 + b"b" + b"a" * 3 + b"bb" + b"a" * 8 + b"c" + b"a" * 7 + b"b" + b"a"),
    ("nested-a-one-long-run", NESTED, b"a" * 200),
    ("duplicate-lines", [b"ab", b"cd", b"ab"], b"ab.cd.abcd"),
    ("siblings-under-a-prefix", [b"ab", b"abc", b"abd"], b"abc abd ab abcabd abx"),
    ("prefix-only-of-long", [b"needle", b"nee"], b"nee needl needle"),
    ("nocase-mixed", [b"Needle", b"AB", b"get /admin", b"Nee"], b"a NEEDLE in GeT /AdMiN HTTP aB Ab plain nEeDlEab nEe"),
    ("pattern-is-the-whole-buffer", [b"whole buffer", b"whole"], b"whole buffer"),
]


def test_the_two_references_agree_on_every_case():
    from tests.spans_ref import brute_result
    for name, pats, data in CASES:
        nocase = name.startswith("nocase")
        folded = [fold(p) for p in pats] if nocase else pats
        prefix, chain, _ = am.prefix_table(folded)
        result = brute_result(pats, data, nocase)
        for longest in (False, True):
            a = counts_py(pats, data, nocase, longest)
            same(counts_from_result(result, (prefix, chain), longest), a, f"{name}/longest {longest}")
            assert int(a.sum()) == total_of(result, (prefix, chain), longest), name
            assert a[0] == 0
    want = {"a-over-a-run": [0, 300], "duplicate-lines": [0, 0, 2, 2], "siblings-under-a-prefix": [0, 6, 2, 2],
            "nested-a-one-long-run": [0] + [201 - k for k in range(1, 9)], "pattern-is-the-whole-buffer": [0, 1, 1], "no-match": [0, 0, 0]}
    for name, pats, data in CASES:
        if name in want:
            assert counts_py(pats, data).tolist() == want[name], name
    assert counts_py(NESTED, b"a" * 200, longest=True).tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 193]
