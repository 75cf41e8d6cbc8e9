"""The model of the lines calls with context (PFACX_matchLinesContext*) and the inputs of tests/test_linesctx_host.py and
tests/test_linesctx_gpu.py.  It uses none of the library's line code: H comes from the references of tests/lines_ref.py, the widening is
the definition of include/pfac_ext.h spelled out as a loop over H.

context_model  (start, len, index, tag, (numLines, numSelected, numMatching, numGroups)) as int32 arrays and a tuple of ints
grep_listing   the same facts parsed from `grep -n -F -f patterns -A a -B b` (the cross-check of the model itself)
Test infrastructure only."""

import os
import shutil
import subprocess

import numpy as np

from tests import lines_ref as ref

MAX = 0xFFFFFFFF


def all_lines(data):
    """(start, len) of every line of `data`, int64 arrays"""
    data = np.frombuffer(bytes(data), dtype=np.uint8)
    if data.size == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z
    ends = np.flatnonzero(data == 10)
    if data[-1] != 10:
        ends = np.append(ends, data.size)
    starts = np.concatenate(([0], ends[:-1] + 1))
    return starts, ends - starts


def members(patterns, data, invert=False, nocase=False):
    """H: the line numbers the plain call selects"""
    data = bytes(data)
    if len(data) <= 4096:
        return ref.lines_py(patterns, data, invert, nocase)[3].astype(np.int64)
    return ref.lines_from_result(ref.brute_result(patterns, data, nocase), np.frombuffer(data, dtype=np.uint8), invert)[3].astype(np.int64)


def widen(num_lines, H, before, after):
    """the selected lines by the definition: k is selected if some h of H has h - before <= k <= h + after (no wrap-around)"""
    sel = np.zeros(num_lines, dtype=bool)
    for h in H.tolist():
        sel[max(0, h - before):min(num_lines - 1, h + after) + 1] = True
    return sel


def context_model(patterns, data, before, after, invert=False, nocase=False, H=None):
    starts, lens = all_lines(data)
    n = int(starts.size)
    H = members(patterns, data, invert, nocase) if H is None else H
    sel = widen(n, H, before, after)
    index = np.flatnonzero(sel)
    is_member = np.zeros(n, dtype=bool)
    is_member[H] = True
    # a group starts at a selected line whose predecessor is not selected
    first = sel & ~np.concatenate(([False], sel[:-1]))
    group = np.cumsum(first) - 1
    tag = (group[index] << 1) | is_member[index]
    counts = (n, int(index.size), int(H.size), int(np.count_nonzero(first)))
    return starts[index].astype(np.int32), lens[index].astype(np.int32), index.astype(np.int32), tag.astype(np.int32), counts


def same(got, want, what):
    """exact equality of two model-shaped results"""
    assert tuple(got[4]) == tuple(want[4]), f"{what}: (lines, selected, matching, groups) = {tuple(got[4])}, want {tuple(want[4])}"
    for name, g, w in zip(("start", "len", "index", "tag"), got[:4], want[:4]):
        assert g.size == w.size, f"{what}: {name} has {g.size} entries, want {w.size}"
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError(f"{what}: {name} differs in {bad.size} lines, first at {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}")


def text_of(data, got):
    """the text a list stands for, and the same as grep prints it: NUM:line / NUM-line, '--' where the group changes"""
    data = bytes(data)
    out, prev = [], None
    for s, l, k, t in zip(got[0].tolist(), got[1].tolist(), got[2].tolist(), got[3].tolist()):
        if prev is not None and t >> 1 != prev:
            out.append(b"--")
        prev = t >> 1
        out.append(b"%d%s%s" % (k + 1, b":" if t & 1 else b"-", data[s:s + l]))
    return ref.gather_py(data, got[0], got[1]), b"".join(o + b"\n" for o in out)


def have_grep():
    return shutil.which("grep") is not None


def grep_listing(workdir, patterns, data, before, after, invert=False, nocase=False):
    """the output of grep -n -F -f patterns -A after -B before [-v] [-i] over `data` (no NUL bytes): bytes"""
    pf = os.path.join(workdir, "linesctx_grep.pat")
    df = os.path.join(workdir, "linesctx_grep.txt")
    with open(pf, "wb") as f:
        f.write(b"".join(bytes(p) + b"\n" for p in patterns))
    with open(df, "wb") as f:
        f.write(bytes(data))
    cmd = ["grep", "-a", "-n", "-F", "-f", pf, "-A", str(after), "-B", str(before)] + (["-v"] if invert else []) + (["-i"] if nocase else []) + [df]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, LC_ALL="C"))
    assert p.returncode in (0, 1), p.stderr
    return p.stdout


# ---------------------------------------------------------------- inputs

X = [b"x"]                              # the pattern of the inputs made of empty and one-byte lines: a line matches if it is "x"


def tiny_lines(num, hits, terminated=True):
    """`num` lines, empty at odd numbers and "z" at even ones, "x" at the numbers in `hits`"""
    hits = set(hits)
    lines = [b"x" if k in hits else (b"" if k & 1 else b"z") for k in range(num)]
    body = b"\n".join(lines)
    assert terminated or lines[-1], "an unterminated empty last line is no line"
    return body + b"\n" if terminated else body


WORD_EDGE_LINES = 100
WORD_EDGE_HITS = [0, 31, 32, 33, 63, 64, WORD_EDGE_LINES - 1]
WORD_EDGE_WINDOWS = [0, 1, 31, 32, 33]

WAVE_LINES, WAVE_HIT = 5000, 2500
WAVE_WINDOWS = [100, 2047, 2048, 2049, 4999, MAX]


def wave_input():
    """WAVE_LINES lines, all empty but line WAVE_HIT, which is "x" """
    data = bytearray(b"\n" * WAVE_LINES)
    data[WAVE_HIT:WAVE_HIT + 1] = b"x\n"
    assert all_lines(bytes(data))[0].size == WAVE_LINES
    return bytes(data)

# (name, patterns, input, before, after, invert): clipping at both ends, groups, INVERT
SMALL = [
    ("hit-on-line-0-before-3", X, tiny_lines(9, [0]), 3, 0, False),
    ("hit-on-last-line-after-3", X, tiny_lines(9, [8]), 0, 3, False),
    ("hit-on-unterminated-last-line-after-3", X, tiny_lines(9, [8], terminated=False), 0, 3, False),
    ("hit-on-unterminated-last-line-before-3", X, tiny_lines(9, [8], terminated=False), 3, 1, False),
    ("a-single-line", X, b"x\n", 2, 2, False),
    ("a-single-unterminated-line", X, b"x", MAX, MAX, False),
    ("a-single-line-without-a-match", X, b"z\n", 2, 2, False),
    ("only-a-newline", X, b"\n", 1, 1, False),
    ("only-a-newline-inverted", X, b"\n", 1, 1, True),
    # hits on lines 10 and 20: windows [10 - b, 10 + a], [20 - b, 20 + a]
    ("windows-one-line-apart", X, tiny_lines(40, [10, 20]), 4, 4, False),      # 14 | 15 | 16: two groups
    ("windows-touching", X, tiny_lines(40, [10, 20]), 5, 4, False),            # 14 | 15: one group
    ("windows-overlapping", X, tiny_lines(40, [10, 20]), 7, 6, False),
    ("adjacent-hits-no-context", X, tiny_lines(40, [3, 4, 5, 9, 11, 12, 39]), 0, 0, False),
    ("groups-across-a-word", X, tiny_lines(80, [1, 30, 33, 62, 66, 79]), 1, 0, False),
    ("inverted-hits-are-the-gaps", X, tiny_lines(70, [31, 32, 33, 64]), 1, 1, True),
    ("inverted-unterminated-last-line", [b"z"], b"q\nz\nq\nz\nz\nz\nz\nq", 0, 1, True),
    ("inverted-unterminated-matching-last-line", [b"z"], b"z\nz\nq\nz\nz\nz\nz\nz", 1, 0, True),
    ("after-is-max-before-is-0", X, tiny_lines(70, [40]), 0, MAX, False),
    ("before-is-max-after-is-0", X, tiny_lines(70, [40]), MAX, 0, False),
    ("no-hit-windows-max", X, tiny_lines(70, []), MAX, MAX, False),
    ("ordinary-text", ref.PATS, b"first needle\nsecond\nthird\nfourth\nfifth end\nsixth\nseventh\neighth\nninth ab\ntenth", 1, 1, False),
    ("crlf", ref.PATS, b"one ab\r\ntwo\r\n\r\nthree needle\r\nfour\r\nfive\r\n", 0, 1, False),
]

INVERT_LINE_COUNTS = [1, 31, 32, 33, 2049]          # every line matches the pattern: H is empty under INVERT, whatever lies behind numLines


def every_line_matches(num):
    return b"x\n" * num


def fold_input():
    """about 320 KiB of short lines: more than 8192 words of bitmap, hits only in the first and the last 10 lines"""
    num = 163840
    hits = [0, 3, 9, num - 10, num - 4, num - 1]
    data = bytearray(b"z\n" * num)
    for k in hits:
        data[2 * k] = ord("x")
    return bytes(data)


FOLD_WINDOWS = [70000, 5]

NOCASE = ([b"Needle"], b"plain\nnothing\na NEEDLE here\nplain\nmore\nneedle\nlast\n", 1, 1)


def test_the_model_equals_grep(workdir):
    """selected line numbers, ':' / '-' marks and the places of '--' against grep itself (skipped without a grep binary)"""
    import pytest
    if not have_grep():
        pytest.skip("no grep on this machine")
    cases = [(name, pats, data, b, a, inv, False) for name, pats, data, b, a, inv in SMALL]
    cases += [(f"word-edge-{hit}", X, tiny_lines(WORD_EDGE_LINES, [hit]), b, a, inv, False)
              for hit in WORD_EDGE_HITS for b in (0, 1, 32) for a in (0, 31, 33) for inv in (False, True)]
    cases += [(f"every-line-matches-{n}", X, every_line_matches(n), 2, 2, True, False) for n in INVERT_LINE_COUNTS]
    cases.append(("nocase", NOCASE[0], NOCASE[1], NOCASE[2], NOCASE[3], False, True))
    cases.append(("nocase-inverted", NOCASE[0], NOCASE[1], 0, 1, True, True))
    for name, pats, data, b, a, inv, nocase in cases:
        b, a = min(b, 1 << 20), min(a, 1 << 20)              # (grep takes an int; a megaline is every line of these inputs)
        model = context_model(pats, data, b, a, inv, nocase)
        assert text_of(data, model)[1] == grep_listing(workdir, pats, data, b, a, inv, nocase), f"{name}: the model and grep disagree"
