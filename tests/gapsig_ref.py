"""References for the gapped-signature calls (PFACX_gapsig*: signatures with bounded gaps between parts) that share no code with the library.

A signature here is (parts, gaps): parts a list of (values, masks) uint8 arrays, gaps a list of (lo, hi), one fewer than parts.

parse_line          one line of the text form -> (parts, gaps), by the rules of include/pfac_ext.h; ValueError for a line it refuses
choose_anchor       the documented choice rule over all parts -> (part, offset, length)
brute               the definition: every start, a recursion over every gap width, the smallest end -> {start: end}
owner_list          an independent model of the owner rule and the list order: per start the offsets of the anchor part that the head reaches
                    (sets of offsets, forwards) and those from which the tail completes (a recursion), the owner the smallest common one
starts_re           Python's re: parts written as in sig_ref.py, gaps as .{lo,hi} under DOTALL, the whole inside a lookahead; it says only
                    WHICH starts occur, never the end
ON `end`.  Let E(j, o) be the smallest end of the parts j .. behind part j at offset o.  The offsets part j + 1 may take behind o are an interval
that moves right with o, so by induction from the last part E(j, .) ascends over the offsets where it is finite: among the choices that can be
completed the nearest is never worse.  A lazy left-to-right choice therefore differs from the minimum only where it runs into a dead end -- it
takes the nearest place at which the next part holds and finds no way on from there; the case `end-lazy-dead-end` is that.
Test infrastructure only."""

import re
from functools import lru_cache

import numpy as np

from tests import sig_ref

DEFAULT_ANCHOR = 32
MAX_SLACK = 63
MAX_PARTS = 64
MAX_GAP = 65535

_GAP = re.compile(rb"[{\[]([0-9]*)(-?)([0-9]*)[}\]]")


def parse_line(line):
    """b'4D 5A {2-6} 50 45' -> (parts, gaps)"""
    line = bytes(line)
    if line.endswith(b"\r"):
        line = line[:-1]
    parts, gaps, at, want_part = [], [], 0, True
    for tok in re.finditer(rb"[{\[][^}\]]*[}\]]?", line):
        body = line[at:tok.start()]
        if not body.strip(b" \t"):
            raise ValueError("a gap without a part in front of it")
        parts.append(sig_ref.parse_line(body))
        text = tok.group(0)
        m = _GAP.fullmatch(text)
        if not m or (text[:1] == b"{") != (text[-1:] == b"}"):
            raise ValueError(f"refused gap {text!r}")
        first, dash, second = m.group(1), m.group(2), m.group(3)
        if not dash:
            if not first or second:
                raise ValueError(f"refused gap {text!r}")
            lo = hi = int(first)
        else:
            if not second:
                raise ValueError(f"an unbounded gap {text!r}")
            lo, hi = int(first or b"0"), int(second)
        if lo > hi or hi > MAX_GAP:
            raise ValueError(f"refused gap {text!r}")
        gaps.append((lo, hi))
        at = tok.end()
    parts.append(sig_ref.parse_line(line[at:]))       # ValueError for an empty tail: a gap at the end, or an empty line
    return parts, gaps


def parse_lines(lines):
    return [parse_line(line.encode() if isinstance(line, str) else line) for line in lines]


text_of = sig_ref.text_of


def check_limits(sig):
    """None, or why PFACX_gapsigOpen refuses the signature"""
    parts, gaps = sig
    if not 1 <= len(parts) <= MAX_PARTS:
        return "parts"
    if any(not 1 <= len(v) <= 65535 for v, _ in parts):
        return "part length"
    if any(lo > hi or hi > MAX_GAP for lo, hi in gaps):
        return "gap"
    if sum(hi - lo for lo, hi in gaps) > MAX_SLACK:
        return "slack"
    if sum(len(v) for v, _ in parts) + sum(hi for _, hi in gaps) >= 2 ** 31 - 1:
        return "span"
    return None if choose_anchor(sig) else "anchor"


def csr_of(sigs):
    """-> (values, masks, part_off, sig_part, gap_lo, gap_hi) as PFACX_gapsigOpen takes them; the gap entry behind a last part is poison"""
    flat = [p for parts, _ in sigs for p in parts]
    values, masks, part_off = sig_ref.csr_of(flat)
    sig_part = np.zeros(len(sigs) + 1, dtype=np.uint64)
    sig_part[1:] = np.cumsum([len(parts) for parts, _ in sigs])
    lo, hi = [], []
    for parts, gaps in sigs:
        lo += [g[0] for g in gaps] + [0xDEAD0000]
        hi += [g[1] for g in gaps] + [7]
    return values, masks, part_off, sig_part, np.array(lo, dtype=np.uint32), np.array(hi, dtype=np.uint32)


def choose_anchor(sig, max_len=0):
    """(part, offset, length), None for a signature without a candidate byte: the longest run inside one part, the lowest part, the leftmost"""
    best = None
    for j, (v, m) in enumerate(sig[0]):
        got = sig_ref.choose_anchor(v, m, 1 << 30)
        if got and (best is None or got[1] > best[2]):
            best = (j, got[0], got[1])
    return (best[0], best[1], min(best[2], max_len or DEFAULT_ANCHOR)) if best else None


def model_anchors(sigs, max_len=0):
    """what PFACX_gapsigGetAnchors must return: (anchor_id, anchor_part, anchor_off, anchor_len) by id, and the distinct anchors"""
    cols, seen, anchors = [[0], [0], [0], [0]], {}, []
    for sig in sigs:
        part, at, length = choose_anchor(sig, max_len)
        v, m = sig[0][part]
        key = bytes(np.asarray(v, dtype=np.uint8)[at:at + length] & np.asarray(m, dtype=np.uint8)[at:at + length])
        if key not in seen:
            anchors.append(key)
            seen[key] = len(anchors)
        for col, value in zip(cols, (seen[key], part, at, length)):
            col.append(value)
    return tuple(np.array(c, np.int32) for c in cols), anchors


def _holds(sig, data):
    """per part the set of offsets at which it holds"""
    return [set(int(s) for s in sig_ref.starts_of(v, m, data)) for v, m in sig[0]]


def brute(sig, data):
    """{start: smallest end}: the definition, gap width by gap width"""
    parts, gaps = sig
    holds, last = _holds(sig, data), len(parts) - 1

    @lru_cache(maxsize=None)
    def best_end(j, o):                                         # part j at o holds: the smallest end behind it, or None
        behind = o + len(parts[j][0])
        if j == last:
            return behind
        ends = [best_end(j + 1, behind + g) for g in range(gaps[j][0], gaps[j][1] + 1) if behind + g in holds[j + 1]]
        ends = [e for e in ends if e is not None]
        return min(ends) if ends else None

    out = {}
    for s in sorted(holds[0]):
        e = best_end(0, s)
        if e is not None:
            out[s] = e
    return out


def owners(sig, data, anchor_part):
    """{start: (owner offset x of the anchor part, the first offset of it that the head reaches)}: sets forwards, a recursion for the tail"""
    parts, gaps = sig
    holds, last = _holds(sig, data), len(parts) - 1

    @lru_cache(maxsize=None)
    def completes(j, o):
        if j == last:
            return True
        behind = o + len(parts[j][0])
        return any(behind + g in holds[j + 1] and completes(j + 1, behind + g) for g in range(gaps[j][0], gaps[j][1] + 1))

    out = {}
    for s in sorted(holds[0]):
        reach = {s}
        for j in range(anchor_part):
            reach = {o + len(parts[j][0]) + g for o in reach for g in range(gaps[j][0], gaps[j][1] + 1)} & holds[j + 1]
        good = sorted(o for o in reach if completes(anchor_part, o))
        if good:
            out[s] = (good[0], min(reach))
    return out


def owner_list(sigs, data, anchors):
    """(pos, ids, end) in the order of the contract, and per entry (owner offset, first reachable offset)"""
    _, a_part, a_off, a_len = anchors
    found = []
    for i, sig in enumerate(sigs, 1):
        ends = brute(sig, data)
        own = owners(sig, data, int(a_part[i]))
        assert set(ends) == set(own), f"signature {i}: the two models disagree on which starts occur"
        found += [(own[s][0] + int(a_off[i]), -int(a_len[i]), -i, s, ends[s], own[s]) for s in ends]
    found.sort(key=lambda f: f[:4])
    col = lambda k, sign=1: np.array([sign * f[k] for f in found], dtype=np.int32)  # noqa: E731
    return (col(3), col(2, -1), col(4)), [f[5] for f in found]


def regex_of(sig):
    parts, gaps = sig
    body = b""
    for j, (v, m) in enumerate(parts):
        body += sig_ref.regex_of(v, m).pattern[3:-1]
        if j < len(gaps):
            body += b".{%d,%d}" % gaps[j]
    return re.compile(b"(?=" + body + b")", re.S)


def starts_re(sig, data):
    return [m.start() for m in regex_of(sig).finditer(bytes(data))]


def same(got, want, what):
    got, want = [np.asarray(a, dtype=np.int64) for a in got], [np.asarray(a, dtype=np.int64) for a in want]
    assert got[0].size == want[0].size, f"{what}: {got[0].size} entries, want {want[0].size}"
    bad = np.flatnonzero(np.any([g != w for g, w in zip(got, want)], axis=0)) if want[0].size else np.zeros(0, int)
    if bad.size:
        k = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} entries differ, first at {k}: got (pos, id, end) {[int(g[k]) for g in got]} want {[int(w[k]) for w in want]}")


def check_models(sigs, data, anchors, what):
    """the models against each other and re on one input -> the list"""
    want, _ = owner_list(sigs, data, anchors)
    for i, sig in enumerate(sigs, 1):
        assert starts_re(sig, data) == sorted(brute(sig, data)), f"{what}: signature {i}: re against the definition"
    return want


# ---------------------------------------------------------------- the case table (tools/gapsig_host_san.cpp drives a part of it)


def hex_of(raw):
    return " ".join("%02X" % b for b in bytes(raw))


def _part(j):
    return bytes([0x80 + j, 0x30 + j % 10])


def _instance(parts, widths):
    out = b""
    for j, p in enumerate(parts):
        out += p + (b"." * widths[j] if j < len(widths) else b"")
    return out


SEP = b"|" * 70                                   # wider than any slack: nothing reaches across it


def _slack_case(gaps):
    """the parts _part(j) with `gaps` between them; every gap at hi, every gap at lo, a middle choice, and one byte too wide"""
    parts = [_part(j) for j in range(len(gaps) + 1)]
    line = "".join(hex_of(p) + (" {%d-%d} " % g if j < len(gaps) else "") for j, (p, g) in enumerate(zip(parts, gaps + [(0, 0)])))
    his, los = [g[1] for g in gaps], [g[0] for g in gaps]
    mid = [g[1] if j % 2 else g[0] for j, g in enumerate(gaps)]
    wide = his[:-1] + [his[-1] + 1]
    return [line], SEP.join(_instance(parts, w) for w in (his, los, mid, wide)) + SEP


def _class_of_300():
    lines = ["51 52 53 54 {0-2} %02X %02X" % (0x21 + k // 20, 0x41 + k % 20) for k in range(300)]
    data = b" ".join(b"QRST" + b"." * (k % 4) + bytes([0x21 + k // 20, 0x41 + k % 20]) for k in (0, 1, 19, 20, 150, 298, 299, 7))
    return lines, data


def _tail_lengths():
    """part lengths 1 .. 20 at the end of a signature: exact, then with only its last and only its first byte wrong"""
    lines, pieces = [], []
    for length in range(1, 21):
        tail = bytes(0xA0 + (3 * i + length) % 0x50 for i in range(length))
        head = bytes([0x41 + length, 0x23])
        lines.append(hex_of(head) + " {1-3} " + hex_of(tail))
        bad_last, bad_first = tail[:-1] + bytes([tail[-1] ^ 1]), bytes([tail[0] ^ 0x10]) + tail[1:]
        pieces += [head + b".." + tail, head + b"." + bad_last, head + b"..." + bad_first, b"-" * (length % 3)]
    return lines, b" ".join(pieces)


# (name, the lines of the text form, input, maxAnchorLen)
CASES = [
    ("gap-0", ["61 62 {0} 63 64"], b"abcd abxcd ab cd abcd", 0),
    ("gap-n", ["61 62 {3} 63 64", "61 62 [3] 63 64"], b"abxxxcd abxxcd abxxxxcd ab\n\n\ncd", 0),
    ("gap-0-1", ["61 62 {0-1} 63 64", "61 62 {-1} 63 64", "61 62 [0-1] 63 64"], b"abcd abxcd abxxcd", 0),
    ("gap-0-63", ["41 42 43 {0-63} 58 59"], SEP.join(b"ABC" + b"." * d + b"XY" for d in range(66)), 0),
    ("slack-63-over-2", *_slack_case([(0, 31), (0, 32)]), 0),
    ("slack-63-over-3", *_slack_case([(2, 23), (0, 21), (5, 26)]), 0),
    ("slack-63-over-63", *_slack_case([(0, 1)] * 63), 0),
    ("anchor-in-the-first-part", ["61 62 63 64 {1-2} 65 ?? {0-2} 66"], b"abcd.e!f abcd..e!.f abcde!f abcd...e!f abcd.e!...f", 0),
    ("anchor-in-a-middle-part", ["61 {1-2} 62 63 64 65 {0-2} 66 ??"], b"a.bcdef! a..bcde..f! abcdef! a.bcde...f! a.bcdef", 0),
    ("anchor-in-the-last-part", ["6? {1-2} 62 ?? {0-2} 63 64 65 66"], b"a.b!cdef o..b!..cdef abb!cdef a.b!...cdef", 0),
    ("anchor-cut", ["61 62 63 64 65 {0-2} 66", "78 {0-1} 61 62 63 7A"], b"abcdef abcde..f abcz xabcz x.abcz abcde...f", 2),
    ("a-shared-anchor-at-different-parts", ["78 79 7A {0-2} 61", "62 {1-3} 78 79 7A", "78 79 7A"], b"xyza b.xyz b..xyz.a bxyz b...xyz..a", 0),
    ("class-of-300", *_class_of_300(), 0),
    ("identical-signatures", ["61 ?? {1-2} 63 64", "61 ?? {1-2} 63 64"], b"ab.cd ab..cd abcd", 0),
    ("one-part", ["61 ?? 63", "4D 5A ?? ?? 50 45"], b"abc axc MZ..PE MZ.PE", 0),
    ("owner-both-complete", ["61 {0-2} 4B 4B {0-2} 7A"], b"aKKK.z", 0),
    ("owner-nearer-dead", ["61 {0-2} 4B 4B {0} 7A"], b"aKKKz", 0),
    ("owner-neither", ["61 {0-2} 4B 4B {0} 7A"], b"aKKK.z aKKK", 0),
    ("owner-many-starts", ["61 {0-63} 4B 4C"], b"aaKL" + SEP + b"aaaKL" + SEP + b"a" * 64 + b"KL" + SEP + b"a" * 70 + b"KL", 0),
    ("end-lazy-dead-end", ["61 {0-1} 6? {0-1} 63 {0} 64"], b"abccd", 0),
    ("half-bytes-and-newlines", ["6? 0A {0-2} ?A 62 63 {1} 0A ?1"], b"a\n\nbc.\nq o\n..*bc.\n1 a\n...\nbc.\na", 0),
    ("tail-lengths", *_tail_lengths(), 0),
    ("input-end", ["61 62 {0-2} 63 64"], b"xx ab..cd ab.cd abcd ab.cd", 0),            # the last embedding ends exactly at n
    ("input-end-cut", ["61 62 {0-2} 63 64 {0-2} 65"], b"ab.cd.e ab.cd..e ab..cd.", 0),  # ... the last one needs byte n
]
# worked out by hand: name -> (ids, starts, ends)
WANT = {
    "owner-both-complete": ([1], [0], [5 + 1]),
    "owner-nearer-dead": ([1], [0], [5]),
    "owner-neither": ([], [], []),
    "end-lazy-dead-end": ([1], [0], [5]),          # 6? at 1 -> 63 at 2 (the nearest) -> 64 at 3: dead; the list has 6? at 1 or 2 -> 63 at 3 -> 64 at 4
    "gap-0": ([1, 1], [0, 17], [4, 21]),
    "identical-signatures": ([2, 1, 2, 1], [0, 0, 6, 6], [5, 5, 12, 12]),
}


def case_sigs(case):
    return parse_lines(case[1])


def test_the_models_agree_on_every_case():
    for case in CASES:
        name, lines, data, cut = case
        sigs = parse_lines(lines)
        assert all(check_limits(s) is None for s in sigs), name
        anchors, _ = model_anchors(sigs, cut)
        want = check_models(sigs, data, anchors, name)
        if name in WANT:
            ids, pos, end = WANT[name]
            same(want, (pos, ids, end), f"{name}: the models against the list worked out by hand")
        assert want[0].size > 0 or name == "owner-neither", name
    # the cases hold what they are meant to
    by = {c[0]: c for c in CASES}
    sig = case_sigs(by["gap-0-63"])[0]
    assert len(brute(sig, by["gap-0-63"][2])) == 64, "each of the 64 distances, and neither 64 nor 65"
    for name in ("slack-63-over-2", "slack-63-over-3", "slack-63-over-63"):
        sig = case_sigs(by[name])[0]
        assert sum(hi - lo for lo, hi in sig[1]) == 63 and len(brute(sig, by[name][2])) == 3, name
    many = owners(case_sigs(by["owner-many-starts"])[0], by["owner-many-starts"][2], 1)
    assert len(many) == 2 + 3 + 64 + 64
    assert owners(case_sigs(by["owner-nearer-dead"])[0], b"aKKKz", 1) == {0: (2, 1)}, "the owner is not the first offset the head reaches"
    assert max(brute(case_sigs(by["input-end"])[0], by["input-end"][2]).values()) == len(by["input-end"][2])
    assert sorted(brute(case_sigs(by["input-end-cut"])[0], by["input-end-cut"][2])) == [0, 8]
    assert choose_anchor(parse_line(b"61 62 {0} 63 64 65")) == (1, 0, 3) and choose_anchor(parse_line(b"61 62 {0} 63 64")) == (0, 0, 2)
    assert choose_anchor(parse_line(b"0A {1} ?? 4?")) is None and choose_anchor(parse_line(b"?? {1} 61 62 63"), 2) == (1, 0, 2)
    for line in (b"{1} 61", b"61 {1}", b"61 {1} {2} 62", b"61 {2-1} 62", b"61 * 62", b"61 {1-} 62", b"61 {65536} 62", b"61 {} 62", b"61 {1] 62",
                 b"61 {1 62", b"61 { 1} 62", b"", b"6 {1} 62", b"61 {-} 62", b"61 {1--2} 62"):
        try:
            parse_line(line)
        except ValueError:
            continue
        raise AssertionError(f"{line!r} must be refused")


# ---------------------------------------------------------------- the seeded random case (tests/test_gapsig_*.py, tools/gapsig_sweep.py)


def random_signatures(seed, count=200, max_parts=5, max_gap=16, min_len=2, max_len=24, min_parts=1):
    """`count` signatures of min_parts .. max_parts parts of min_len .. max_len bytes -- every other signature: of at most 6 bytes, which fit into gaps -- (up to a fifth of them wildcards or half bytes, never a part's
    first byte), gaps lo .. lo + width with lo <= 8, width <= max_gap, the slack kept within 63"""
    rng = np.random.default_rng(seed)
    sigs = []
    for _ in range(count):
        parts, gaps, slack, short = [], [], 0, bool(rng.integers(0, 2))
        for j in range(int(rng.integers(min_parts, max_parts + 1))):
            length = int(rng.integers(min_len, (6 if short else max_len) + 1))
            values = rng.integers(0, 256, length, dtype=np.uint8)
            masks = np.full(length, 0xFF, dtype=np.uint8)
            for at in rng.choice(np.arange(1, length), size=int(rng.uniform(0, 0.2) * length), replace=False):
                masks[at] = (0xF0, 0x0F)[int(rng.integers(0, 2))] if rng.integers(0, 4) == 0 else 0x00
            if j:
                lo, width = int(rng.integers(0, 9)), min(int(rng.integers(0, max_gap + 1)), MAX_SLACK - slack)
                slack += width
                gaps.append((lo, lo + width))
            parts.append((values, masks))
        sigs.append((parts, gaps))
    return sigs


def embed(sigs, data, seed, per_sig=3, near_misses=1):
    """`data` (uint8, modified in place) with per_sig embeddings of every signature at random places and random gap widths, and near misses:
    the same with one masked bit of one part flipped.  Where the widths allow it, the first embedding of a signature gets a DECOY of its anchor
    part a in the gap in front of it, with the gap behind a at hi: the head reaches the decoy, the tail does not complete from it, so the owner
    is not the first offset the head reaches; the second one gets a copy of part 0 in front of it, with the first gap at lo: two starts that
    one anchor occurrence lists"""
    rng = np.random.default_rng(seed + 1)
    n = data.size
    for sig in sigs:
        parts, gaps = sig
        a, last = choose_anchor(sig)[0], len(parts) - 1
        for k in range(per_sig + near_misses):
            widths = [int(rng.integers(lo, hi + 1)) for lo, hi in gaps]
            decoy = k == 0 and 1 <= a < last and len(parts[a][0]) <= gaps[a - 1][1] - gaps[a - 1][0]
            twin = k == 1 and a >= 1 and len(parts[0][0]) <= gaps[0][1] - gaps[0][0]
            if decoy:
                widths[a - 1], widths[a] = gaps[a - 1][1], gaps[a][1]
            if twin:
                widths[0] = gaps[0][0]
            body = []
            for j, (v, m) in enumerate(parts):
                piece = (v & m) | (rng.integers(0, 256, len(v), dtype=np.uint8) & ~m)
                if k >= per_sig and j == k % len(parts):
                    where = int(rng.choice(np.flatnonzero(m)))
                    piece[where] ^= np.uint8(int(m[where]) & -int(m[where]))
                if twin and j == 0:
                    body.append(piece.copy())
                body.append(piece)
                if j < len(gaps):
                    fill = rng.integers(0, 256, widths[j], dtype=np.uint8)
                    if decoy and j == a - 1:
                        nxt = parts[a][0] & parts[a][1]
                        fill[len(fill) - len(nxt):] = nxt
                    body.append(fill)
            body = np.concatenate(body)
            if body.size <= n:
                at = int(rng.integers(0, n - body.size + 1))
                data[at:at + body.size] = body
    return data


def random_case(seed=20261022, count=200, n=1 << 16):
    sigs = random_signatures(seed, count)
    data = embed(sigs, np.random.default_rng(seed + 2).integers(0, 256, n, dtype=np.uint8), seed)
    return sigs, data


def random_case_figures(sigs, data, anchors):
    """the list and what makes the random case worth running: entries, entries of signatures with three or more parts, entries whose owner is
    not the first offset the head reaches, anchor occurrences that list more than one start"""
    want, own = owner_list(sigs, data, anchors)
    pos, ids, _ = want
    deep = sum(1 for i in ids if len(sigs[int(i) - 1][0]) >= 3)
    late = sum(1 for x, first in own if x != first)
    per = {}
    for i, (x, _) in zip(ids, own):
        per[(int(i), x)] = per.get((int(i), x), 0) + 1
    return want, {"entries": int(pos.size), "deep": deep, "late_owner": late, "multi_start": sum(1 for c in per.values() if c > 1)}
