"""References for the lines calls (PFACX_matchLines* / PFACX_gatherLinesFromDevice) that use none of the library's line code.

lines_py           pure Python: bytes.split and `in`, for inputs small enough for it
lines_from_result  numpy: the newline positions and a searchsorted of the non-zero positions of a longest-match vector (the oracle's), for
                   inputs too big for the first
gather_py          the text a list of lines stands for
Each returns (numLines, start, len, index) as int32 arrays (gather_py: bytes).  Test infrastructure only."""

import numpy as np


def fold(b):
    """the ASCII fold of PFACX_READ_NOCASE: 'A'-'Z' -> 'a'-'z', nothing else"""
    return bytes(c + 32 if 65 <= c <= 90 else c for c in bytes(b))


def split_lines(data):
    """[(start, bytes)] of the lines of `data`: a trailing '\\n' ends the last line, it does not start an empty one"""
    data = bytes(data)
    if not data:
        return []
    parts = data.split(b"\n")
    if data.endswith(b"\n"):
        parts.pop()
    out, at = [], 0
    for p in parts:
        out.append((at, p))
        at += len(p) + 1
    return out


def lines_py(patterns, data, invert=False, nocase=False):
    pats = [fold(p) if nocase else bytes(p) for p in patterns]
    start, length, index = [], [], []
    lines = split_lines(data)
    for k, (at, line) in enumerate(lines):
        hay = fold(line) if nocase else line
        if any(p in hay for p in pats) != bool(invert):
            start.append(at)
            length.append(len(line))
            index.append(k)
    return len(lines), np.array(start, dtype=np.int32), np.array(length, dtype=np.int32), np.array(index, dtype=np.int32)


def lines_from_result(result_vector, data, invert=False):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = data.size
    if n == 0:
        z = np.zeros(0, dtype=np.int32)
        return 0, z, z, z
    ends = np.flatnonzero(data == 10)
    if data[-1] != 10:
        ends = np.append(ends, n)
    starts = np.concatenate(([0], ends[:-1] + 1))
    hit = np.zeros(ends.size, dtype=bool)
    hit[np.searchsorted(ends, np.flatnonzero(np.asarray(result_vector)[:n]), side="right")] = True
    sel = np.flatnonzero(hit != bool(invert))
    return int(ends.size), starts[sel].astype(np.int32), (ends[sel] - starts[sel]).astype(np.int32), sel.astype(np.int32)


def gather_py(data, start, length):
    data = bytes(data)
    return b"".join(data[int(s):int(s) + int(l)] + b"\n" for s, l in zip(start, length))


def brute_result(patterns, data, nocase=False):
    """a vector that is non-zero exactly where some pattern starts (what lines_from_result needs of a longest-match vector)"""
    hay = fold(data) if nocase else bytes(data)
    out = np.zeros(len(hay), dtype=np.int32)
    for p in patterns:
        p = fold(p) if nocase else bytes(p)
        at = hay.find(p)
        while at >= 0:
            out[at] = 1
            at = hay.find(p, at + 1)
    return out


def same(got, want, what):
    """exact equality of two (numLines, start, len, index) results"""
    assert got[0] == want[0], f"{what}: {got[0]} lines, want {want[0]}"
    for name, g, w in zip(("start", "len", "index"), got[1:], want[1:]):
        assert g.size == w.size, f"{what}: {g.size} selected lines, want {w.size}"
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError(f"{what}: {name} differs in {bad.size} lines, first at {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}")


PATS = [b"ab", b"needle", b"x", b"whole line", b"end"]
# (name, patterns, input): the edge cases of the line definition and of matches at line ends
CASES = [
    ("empty", PATS, b""),
    ("one-newline", PATS, b"\n"),
    ("three-newlines", PATS, b"\n\n\n"),
    ("no-newline", PATS, b"a needle in one line"),
    ("no-newline-no-match", PATS, b"nothing here"),
    ("trailing-newline", PATS, b"first needle\nsecond\nthird end\n"),
    ("no-trailing-newline", PATS, b"first needle\nsecond\nthird end"),
    ("match-in-unterminated-last-line", PATS, b"first\nsecond\nthe needle"),
    ("match-at-first-byte-of-line", PATS, b"zzz\nneedle first\nzzz\n"),
    ("match-at-last-byte-of-line", PATS, b"zzz\nlast is x\nzzz\n"),
    ("match-behind-newline", PATS, b"q\nab\nq\nabq\n"),
    ("match-in-front-of-newline", PATS, b"qq ab\nqq\nqab\n"),
    ("pattern-split-by-newline", PATS, b"nee\ndle\na\nb\nwhole\n line\n"),
    ("fifty-matches-in-one-line", PATS, b"zz\n" + b"ab " * 50 + b"\nzz\n"),
    ("crlf", PATS, b"one ab\r\ntwo\r\n\r\nthree needle\r\n"),
    ("one-byte-patterns", [b"q", b"Z", b"\r"], b"q\nz\nZ\n\n\r\nqq\nyy"),
    ("pattern-equals-whole-line", PATS, b"whole line\nwhole lin\nwhole line"),
    ("empty-lines-between", PATS, b"\n\nab\n\n\nq\n\n"),
]
NOCASE_CASES = [
    ("nocase-mixed", [b"Needle", b"AB", b"get /admin"], b"a NEEDLE\nnothing\nGeT /AdMiN HTTP\naB\nAb\n\nplain\n"),
]


def test_the_two_references_agree_on_the_small_cases():
    for name, pats, data in CASES + NOCASE_CASES:
        nocase = name.startswith("nocase")
        for invert in (False, True):
            a = lines_py(pats, data, invert, nocase)
            b = lines_from_result(brute_result(pats, data, nocase), np.frombuffer(data, dtype=np.uint8), invert)
            same(b, a, f"{name}/invert {invert}")
            assert gather_py(data, a[1], a[2]) == b"".join(data[s:s + l] + b"\n" for s, l in zip(a[1].tolist(), a[2].tolist()))
    assert lines_py(PATS, b"\n\n\n", True)[0] == 3 and lines_py(PATS, b"a\nb", True)[0] == 2 and lines_py(PATS, b"a\nb\n", True)[0] == 2
