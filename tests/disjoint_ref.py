"""References for the disjoint and the replace calls (PFACX_matchDisjoint* / PFACX_replace*) that share no code with the library or with each other.

disjoint_py           Python's re: the alternation of the escaped patterns in descending length is leftmost-longest for literals, finditer is
                      non-overlapping; of duplicate lines the highest id
disjoint_from_result  the loop of the definition over a longest-match vector (the oracle's, or spans_ref.brute_result)
replace_py            the replacement text of a token list, from the pattern lengths and a list of replacements by id
Both list references return (ids, pos) as int32 arrays.  Behind them the helpers the two test files share: the replacement table as the calls take
it, the host calls over poisoned arrays with guard words.  Test infrastructure only."""

import re

import numpy as np

from pfac_amd import api
from tests.spans_ref import brute_result, fold, pattern_lengths

GUARD = 64
RANDOM_SEEDS = list(range(40))          # of spans_helpers.random_case: alphabets of 2 - 3 letters, overlaps everywhere


def disjoint_py(patterns, data, nocase=False):
    pats = [fold(p) if nocase else bytes(p) for p in patterns]
    hay = fold(data) if nocase else bytes(data)
    id_of = {p: k + 1 for k, p in enumerate(pats)}                       # the last line wins: the highest id
    rx = re.compile(b"|".join(re.escape(p) for p in sorted(set(pats), key=len, reverse=True)))
    found = [(id_of[m.group()], m.start()) for m in rx.finditer(hay)]
    return np.array([f[0] for f in found], dtype=np.int32), np.array([f[1] for f in found], dtype=np.int32)


def disjoint_from_result(result_vector, lengths):
    """lengths: by id (entry 0 unused)"""
    r = np.asarray(result_vector)
    ids, pos, p, n = [], [], 0, int(r.size)
    while p < n:
        if r[p] > 0:
            ids.append(int(r[p]))
            pos.append(p)
            p += int(lengths[r[p]])
        else:
            p += 1
    return np.array(ids, dtype=np.int32), np.array(pos, dtype=np.int32)


def replace_py(data, ids, pos, lengths, repls):
    """repls: by id (entry 0 unused)"""
    data = bytes(data)
    out, at = [], 0
    for i, p in zip(ids, pos):
        out.append(data[at:int(p)])
        out.append(bytes(repls[int(i)]))
        at = int(p) + int(lengths[int(i)])
    out.append(data[at:])
    return b"".join(out)


def same(got, want, what):
    """exact equality of two (ids, pos) results"""
    for name, g, w in zip(("ids", "pos"), got, want):
        assert g.size == w.size, f"{what}: {g.size} tokens, want {w.size}"
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError(f"{what}: {name} differs in {bad.size} tokens, first at {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}")


def covered_of(tokens, lengths):
    return int(np.asarray(lengths, dtype=np.int64)[tokens[0]].sum())


# (name, patterns, input): the edge cases of the definition
CASES = [
    ("empty", [b"ab"], b""),
    ("no-match", [b"ab", b"needle"], b"nothing here"),
    ("match-at-byte-0", [b"ab"], b"ab.."),
    ("match-ends-at-last-byte", [b"ab"], b"..ab"),
    ("touching", [b"ab", b"cde"], b".abcdeab.abab"),
    ("abba-even", [b"ab", b"ba"], b"ab" * 50),
    ("abba-odd", [b"ab", b"ba"], b"x" + b"ab" * 50),
    ("short-inside-long-reaches-beyond", [b"abcd", b"cdef", b"efg", b"g"], b".abcdefg.cdefg"),
    ("a-to-a8", [b"a" * k for k in range(1, 9)], b"b" + b"a" * 30 + b"b" + b"a" * 3 + b"b" + b"a" * 8 + b"a" * 8),
    ("duplicate-lines", [b"ab", b"cd", b"ab"], b"ab.cd.abcd"),
    ("prefix-only-of-long", [b"needle", b"nee"], b"nee needl needle"),
    ("nocase-mixed", [b"Needle", b"AB", b"get /admin", b"le"], b"a NEEDLE in GeT /AdMiN HTTP aB Ab plain nEeDlEab LE"),
]


def replacements_for(patterns, kind):
    """a list of replacements by id (entry 0 unused): delete, shrink, same (length kept), grow, mixed"""
    out = [b""]
    for k, p in enumerate(patterns):
        n = len(p)
        tag = b"<%d>" % (k + 1)
        out.append({"delete": b"", "shrink": tag[:max(n - 1, 0)], "same": (tag * n)[:n], "grow": tag + p.upper() + tag,
                    "mixed": [b"", tag, (tag * n)[:n], tag + p + tag][k % 4]}[kind])
    return out


KINDS = ["delete", "shrink", "same", "grow", "mixed"]


def repl_table(repls):
    """the replacement table as the calls take it: (offsets int32 [F + 2], bytes uint8); entry 0 unused"""
    off = np.concatenate(([0], np.cumsum([len(r) for r in repls]))).astype(np.int32)
    blob = b"".join(bytes(r) for r in repls)
    return off, np.frombuffer(blob, dtype=np.uint8).copy() if blob else np.zeros(0, dtype=np.uint8)


def host_disjoint(h, data):
    """matchDisjointFromHost over poisoned arrays of capacity == size (+ GUARD) -> ((ids, pos), covered bytes, the input bytes after the call)"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    n = buf.size
    ids, pos = (np.full(n + GUARD, -7, dtype=np.int32) for _ in range(2))
    st, nt, cb = h.matchDisjointFromHost(buf.ctypes.data if n else ids.ctypes.data, n, ids.ctypes.data, pos.ctypes.data, n)
    assert st == 0 and nt <= n
    assert np.all(ids[n:] == -7) and np.all(pos[n:] == -7), "wrote behind capacity"
    return (ids[:nt].copy(), pos[:nt].copy()), cb, buf.tobytes()


def host_replace(h, data, ids, pos, repls, capacity=None, num_tokens=None, table=None):
    """replaceFromHost with guard bytes on both sides of the output -> (status, outBytes, the first min(outBytes, capacity) bytes)"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    ids, pos = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(pos, dtype=np.int32)
    off, blob = table if table is not None else repl_table(repls)
    count = int(ids.size) if num_tokens is None else num_tokens
    if capacity is None:
        st, capacity = h.replaceFromHost(buf.ctypes.data, buf.size, ids.ctypes.data, pos.ctypes.data, count, off.ctypes.data, off.size,
                                         blob.ctypes.data, blob.size, None, 0, check=False)
        assert st == (api.STATUS.OUTPUT_TRUNCATED if capacity else 0), "the size query"
    out = np.full(GUARD + capacity + GUARD, 0xEE, dtype=np.uint8)
    st, total = h.replaceFromHost(buf.ctypes.data, buf.size, ids.ctypes.data, pos.ctypes.data, count, off.ctypes.data, off.size,
                                  blob.ctypes.data, blob.size, out.ctypes.data + GUARD, capacity, check=False)
    assert np.all(out[:GUARD] == 0xEE) and np.all(out[GUARD + capacity:] == 0xEE), "wrote outside h_out[0, outCapacity)"
    assert buf.tobytes() == bytes(data), "the input was modified"
    return st, total, out[GUARD:GUARD + min(total, capacity)].tobytes()


def test_the_two_references_agree_on_every_case():
    for name, pats, data in CASES:
        nocase = name.startswith("nocase")
        a = disjoint_py(pats, data, nocase)
        b = disjoint_from_result(brute_result(pats, data, nocase), pattern_lengths(pats))
        same(b, a, name)
        assert np.all(a[1][1:] >= a[1][:-1] + pattern_lengths(pats)[a[0][:-1]]), f"{name}: ascending and disjoint"
    want = {"touching": ([1, 2, 1, 1, 1], [1, 3, 6, 9, 11]),
            "abba-even": ([1] * 50, list(range(0, 100, 2))),
            "abba-odd": ([1] * 50, list(range(1, 101, 2))),
            "short-inside-long-reaches-beyond": ([1, 3, 2, 4], [1, 5, 9, 13]),
            "a-to-a8": ([8, 8, 8, 6, 3, 8, 8], [1, 9, 17, 25, 32, 36, 44]),
            "duplicate-lines": ([3, 2, 3, 2], [0, 3, 6, 8]),
            "prefix-only-of-long": ([2, 2, 1], [0, 4, 10])}
    for name, pats, data in CASES:
        if name in want:
            i, p = disjoint_py(pats, data)
            assert (i.tolist(), p.tolist()) == want[name], name
    name, pats, data = next(c for c in CASES if c[0] == "short-inside-long-reaches-beyond")
    i, p = disjoint_py(pats, data)
    assert replace_py(data, i, p, pattern_lengths(pats), [b"", b"<1>", b"<2>", b"", b"GG"]) == b".<1>.<2>GG"
    assert replace_py(b"abc", [], [], [0], [b""]) == b"abc"
