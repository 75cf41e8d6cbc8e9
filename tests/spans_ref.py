"""References for the spans calls (PFACX_matchSpans* / PFACX_redactSpansFromDevice) that share no code with the library or with each other.

spans_py           pure Python: every occurrence of every pattern (bytes.find) marked in a bytearray, then the runs read off
spans_from_result  numpy: np.maximum.accumulate over p + len at the non-zero positions of a longest-match vector (the oracle's)
redact_py          the buffer with the bytes of a list of spans overwritten
Both span references return (start, len) as int32 arrays.  Test infrastructure only."""

import numpy as np


def fold(b):
    """the ASCII fold of PFACX_READ_NOCASE: 'A'-'Z' -> 'a'-'z', nothing else"""
    return bytes(c + 32 if 65 <= c <= 90 else c for c in bytes(b))


def spans_py(patterns, data, nocase=False):
    hay = fold(data) if nocase else bytes(data)
    mark = bytearray(len(hay))
    for p in patterns:
        p = fold(p) if nocase else bytes(p)
        at = hay.find(p)
        while at >= 0:
            mark[at:at + len(p)] = b"\x01" * len(p)
            at = hay.find(p, at + 1)
    start, length, b = [], [], 0
    while b < len(mark):
        if mark[b]:
            e = b
            while e < len(mark) and mark[e]:
                e += 1
            start.append(b)
            length.append(e - b)
            b = e
        else:
            b += 1
    return np.array(start, dtype=np.int32), np.array(length, dtype=np.int32)


def spans_from_result(result_vector, pattern_lengths):
    """pattern_lengths: by id (entry 0 unused)"""
    r = np.asarray(result_vector)
    pos = np.flatnonzero(r > 0).astype(np.int64)
    if pos.size == 0:
        z = np.zeros(0, dtype=np.int32)
        return z, z
    end = pos + np.asarray(pattern_lengths, dtype=np.int64)[r[pos]]
    top = np.maximum.accumulate(end)
    head = np.ones(pos.size, dtype=bool)
    head[1:] = pos[1:] > top[:-1]
    first = np.flatnonzero(head)
    last = np.append(first[1:] - 1, pos.size - 1)
    return pos[first].astype(np.int32), (top[last] - pos[first]).astype(np.int32)


def pattern_lengths(patterns):
    """by id of a pattern file written in this order: ids count from 1"""
    return np.array([0] + [len(p) for p in patterns], dtype=np.int64)


def pattern_lengths_of_file(path):
    """by id: pattern k is line k of the file"""
    lines = open(path, "rb").read().split(b"\n")
    return np.array([0] + [len(p) for p in lines[:-1]], dtype=np.int64)


def brute_result(patterns, data, nocase=False):
    """the longest-match vector of a pattern file written in this order: the id of the longest pattern at each position (of
    duplicate lines the highest id), 0 where none starts"""
    hay = fold(data) if nocase else bytes(data)
    out = np.zeros(len(hay), dtype=np.int32)
    best = np.zeros(len(hay), dtype=np.int32)
    for k, p in enumerate(patterns):
        p = fold(p) if nocase else bytes(p)
        at = hay.find(p)
        while at >= 0:
            if len(p) >= best[at]:
                best[at] = len(p)
                out[at] = k + 1
            at = hay.find(p, at + 1)
    return out


def redact_py(data, start, length, fill):
    out = bytearray(bytes(data))
    for s, l in zip(start, length):
        out[int(s):int(s) + int(l)] = bytes([fill]) * int(l)
    return bytes(out)


def same(got, want, what):
    """exact equality of two (start, len) results"""
    for name, g, w in zip(("start", "len"), got, want):
        assert g.size == w.size, f"{what}: {g.size} spans, want {w.size}"
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError(f"{what}: {name} differs in {bad.size} spans, first at {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}")


LONG = b"L" + b"x" * 58 + b"R"                                           # a 60-byte pattern full of the 1-byte pattern x
# (name, patterns, input): the edge cases of the definition
CASES = [
    ("empty", [b"ab"], b""),
    ("no-match", [b"ab", b"needle"], b"nothing here"),
    ("match-at-byte-0", [b"ab"], b"ab.."),
    ("match-ends-at-last-byte", [b"ab"], b"..ab"),
    ("touching", [b"ab"], b"abab"),
    ("touching-different-patterns", [b"ab", b"cde"], b".abcde.cdeab."),
    ("one-byte-apart", [b"ab"], b"ab.ab"),
    ("nested-short-in-long", [b"needle", b"ed"], b"a needle here"),
    ("overlap-chain", [b"abc", b"cde", b"efg", b"ghi"], b"..abcdefghi.."),
    ("long-outlasts-short", [LONG, b"x"], b".." + LONG + b".x." + LONG + b"x"),
    ("a-to-a8", [b"a" * k for k in range(1, 9)], b"b" + b"a" * 30 + b"b" + b"a" * 3 + b"b"),
    ("every-byte-covered", [b"a", b"b"], b"abba" * 25),
    ("every-second-byte", [b"a"], b"ab" * 50),
    ("duplicate-lines", [b"ab", b"cd", b"ab"], b"ab.cd.abcd"),
    ("prefix-only-of-long", [b"needle", b"nee"], b"nee needl needle"),
    ("nocase-mixed", [b"Needle", b"AB", b"get /admin"], b"a NEEDLE in GeT /AdMiN HTTP aB Ab plain nEeDlEab"),
]


def test_the_two_references_agree_on_every_case():
    for name, pats, data in CASES:
        nocase = name.startswith("nocase")
        a = spans_py(pats, data, nocase)
        b = spans_from_result(brute_result(pats, data, nocase), pattern_lengths(pats))
        same(b, a, name)
        assert redact_py(data, a[0], a[1], 0).count(0) == int(a[1].sum()), name            # (no case holds a zero byte)
    want = {"touching": ([0], [4]), "one-byte-apart": ([0, 3], [2, 2]), "overlap-chain": ([2], [9]), "every-byte-covered": ([0], [100]),
            "every-second-byte": (list(range(0, 100, 2)), [1] * 50), "nested-short-in-long": ([2], [6]), "a-to-a8": ([1, 32], [30, 3]),
            "long-outlasts-short": ([2, 63, 65], [60, 1, 61])}
    for name, pats, data in CASES:
        if name in want:
            s, l = spans_py(pats, data)
            assert (s.tolist(), l.tolist()) == want[name], name
