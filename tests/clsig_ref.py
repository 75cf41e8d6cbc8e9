"""References for the class-signature calls (PFACX_clsig*: signatures of byte classes with bounded repeats) that share no code with the library
or with each other.

A signature here is (elems, not_before, not_after): elems a list of (frozenset of byte values, lo, hi), the boundaries frozensets or None.

parse_line          one line of the text form -> a signature, by the rules of include/pfac_ext.h; ValueError for a line it refuses
fuse                the parts after fusion -> [(kind, payload, first element)], kind 'lit' (bytes) or 'cls' ((set, lo, hi))
choose_anchor       the documented choice rule over the literal parts -> (part, offset, length)
ends_recursive      model 1: a recursion over every run length -> {start: set of valid ends}
ends_by_sets        model 2: sets of offsets, element by element
ends_re             model 3: Python's re compiled from the text line itself under DOTALL: existence from match() at each start, the set of ends
                    from fullmatch(data, s, e) over the core for every e in reach (the end of a greedy or lazy match is never used), the two
                    boundary tests by the line's own lookarounds
owner_list          an independent model of the owner rule and of the list order: per start the offsets of the anchor part that the head reaches
                    (sets) and those from which the tail completes to a valid end (a recursion); the owner is the smallest common one
Test infrastructure only."""

import re
from functools import lru_cache

import numpy as np

DEFAULT_ANCHOR = 32
MAX_SLACK = 63
MAX_PARTS = 64
MAX_REPEAT = 65535
SHORTEST = 1

META = b"\\.[](){}?*+|^$"
_SIMPLE = {ord("n"): 10, ord("r"): 13, ord("t"): 9, ord("f"): 12, ord("v"): 11}
_DIGIT = frozenset(range(48, 58))
_WORD = frozenset(list(range(48, 58)) + list(range(65, 91)) + list(range(97, 123)) + [95])
_SPACE = frozenset([32, 9, 10, 11, 12, 13])
_ALL = frozenset(range(256))
_CLASSES = {ord("d"): _DIGIT, ord("D"): _ALL - _DIGIT, ord("w"): _WORD, ord("W"): _ALL - _WORD, ord("s"): _SPACE, ord("S"): _ALL - _SPACE}


def _escape(line, j, in_set):
    """the escape behind the backslash at line[j - 1] -> (a byte value or a frozenset, the index behind it)"""
    if j >= len(line):
        raise ValueError("a backslash at the end")
    e = line[j]
    if e in _SIMPLE:
        return _SIMPLE[e], j + 1
    if e == ord("0"):
        if j + 1 < len(line) and chr(line[j + 1]).isdigit():
            raise ValueError("an octal escape")
        return 0, j + 1
    if e == ord("x"):
        digits = line[j + 1:j + 3]
        if len(digits) != 2 or not re.fullmatch(rb"[0-9a-fA-F]{2}", digits):
            raise ValueError("\\x without two hex digits")
        return int(digits, 16), j + 3
    if e in _CLASSES:
        return _CLASSES[e], j + 1
    if e in META or (in_set and e == ord("-")):
        return e, j + 1
    raise ValueError(f"unknown escape \\{chr(e)}")


def _set(line, j):
    """the body of a bracket set behind its '[' -> (frozenset, the index behind its ']')"""
    members, negated = set(), False
    if j < len(line) and line[j] == ord("^"):
        negated, j = True, j + 1
    while True:
        if j >= len(line):
            raise ValueError("an unclosed set")
        if line[j] == ord("]"):
            j += 1
            break
        if line[j] == ord("\\"):
            lhs, j = _escape(line, j + 1, True)
        else:
            lhs, j = line[j], j + 1
        if j + 1 < len(line) and line[j] == ord("-") and line[j + 1] != ord("]"):
            if not isinstance(lhs, int):
                raise ValueError("a class escape as the start of a range")
            j += 1
            if line[j] == ord("\\"):
                rhs, j = _escape(line, j + 1, True)
            else:
                rhs, j = line[j], j + 1
            if not isinstance(rhs, int) or rhs < lhs:
                raise ValueError("a bad range")
            members |= set(range(lhs, rhs + 1))
        elif isinstance(lhs, int):
            members.add(lhs)
        else:
            members |= lhs
    if not members:
        raise ValueError("an empty set")
    members = _ALL - members if negated else frozenset(members)
    if not members:
        raise ValueError("an empty set")
    return frozenset(members), j


def _number(line, j):
    k = j
    while k < len(line) and 48 <= line[k] <= 57:
        k += 1
    if k == j or int(line[j:k]) > MAX_REPEAT:
        raise ValueError("a bad number")
    return int(line[j:k]), k


def parse_line(line):
    """b'AKIA[0-9A-Z]{16}(?![0-9A-Z])' -> (elems, not_before, not_after)"""
    line = bytes(line)
    if line.endswith(b"\r"):
        line = line[:-1]
    j, elems, nb, na, quantifiable = 0, [], None, None, False
    if line.startswith(b"(?<!"):
        if not line.startswith(b"(?<!["):
            raise ValueError("a lookbehind without a set")
        nb, j = _set(line, 5)
        if line[j:j + 1] != b")":
            raise ValueError("an unclosed lookbehind")
        j += 1
    while j < len(line):
        ch = line[j]
        if ch == ord("("):
            if not line.startswith(b"(?![", j):
                raise ValueError("a group")
            na, j = _set(line, j + 4)
            if line[j:] != b")":
                raise ValueError("something behind the lookahead")
            break
        if ch in b"{?":
            if not quantifiable:
                raise ValueError("a quantifier without a unit")
            lo, hi, j = 0, 1, j + 1
            if ch == ord("{"):
                lo, j = _number(line, j)
                hi = lo
                if line[j:j + 1] == b",":
                    hi, j = _number(line, j + 1)
                if line[j:j + 1] != b"}" or lo > hi:
                    raise ValueError("a bad quantifier")
                j += 1
            elems[-1] = (elems[-1][0], lo, hi)
            quantifiable = False
            continue
        j += 1
        if ch == ord("["):
            members, j = _set(line, j)
        elif ch == ord("."):
            members = _ALL
        elif ch == ord("\\"):
            got, j = _escape(line, j, False)
            members = frozenset([got]) if isinstance(got, int) else got
        elif ch in b"])}*+|^$":
            raise ValueError(f"a bare {chr(ch)!r}")
        else:
            members = frozenset([ch])
        elems.append((members, 1, 1))
        quantifiable = True
    if not elems:
        raise ValueError("no unit")
    return elems, nb, na


def parse_lines(lines):
    return [parse_line(line.encode("latin-1") if isinstance(line, str) else line) for line in lines]


def text_of(lines):
    return b"".join((line.encode("latin-1") if isinstance(line, str) else bytes(line)) + b"\n" for line in lines)


def fuse(sig):
    """[(kind, payload, index of the first element)]"""
    parts = []
    for k, (members, lo, hi) in enumerate(sig[0]):
        if len(members) == 1 and lo == hi:
            piece = bytes(members) * lo
            if parts and parts[-1][0] == "lit":
                parts[-1] = ("lit", parts[-1][1] + piece, parts[-1][2])
            else:
                parts.append(("lit", piece, k))
        else:
            parts.append(("cls", (members, lo, hi), k))
    return parts


def choose_anchor(sig, max_len=0):
    """(part, offset, length) or None: the longest run of bytes other than 0x0A inside one literal part, the lowest part, the leftmost"""
    best = None
    for j, (kind, payload, _) in enumerate(fuse(sig)):
        if kind != "lit":
            continue
        for m in re.finditer(rb"[^\n]+", payload):
            if best is None or len(m.group()) > best[2]:
                best = (j, m.start(), len(m.group()))
    return (best[0], best[1], min(best[2], max_len or DEFAULT_ANCHOR)) if best else None


def check_limits(sig):
    """None, or why PFACX_clsigOpen refuses the signature"""
    elems = sig[0]
    if not elems:
        return "elements"
    if any(lo > hi or hi == 0 or hi > MAX_REPEAT or not members for members, lo, hi in elems):
        return "element"
    if sum(hi - lo for _, lo, hi in elems) > MAX_SLACK:
        return "slack"
    parts = fuse(sig)
    if len(parts) > MAX_PARTS:
        return "parts"
    if any(kind == "lit" and len(payload) > MAX_REPEAT for kind, payload, _ in parts):
        return "literal length"
    if sum(hi for _, _, hi in elems) >= 2 ** 23:
        return "span"
    return None if choose_anchor(sig) else "anchor"


def words_of(members):
    w = [0] * 8
    for b in members:
        w[b >> 5] |= 1 << (b & 31)
    return tuple(w)


def csr_of(sigs):
    """-> (classes, elem_class, elem_lo, elem_hi, sig_elem, not_before, not_after) as PFACX_clsigOpen takes them; equal classes stored once"""
    table, rows = {}, []

    def index(members):
        key = words_of(members)
        if key not in table:
            table[key] = len(rows)
            rows.append(key)
        return table[key]

    cls, lo, hi, sig_elem, nb, na = [], [], [], [0], [], []
    for elems, before, after in sigs:
        for members, a, b in elems:
            cls.append(index(members))
            lo.append(a)
            hi.append(b)
        sig_elem.append(len(cls))
        nb.append(-1 if before is None else index(before))
        na.append(-1 if after is None else index(after))
    return (np.array(rows, dtype=np.uint32).reshape(-1, 8), np.array(cls, dtype=np.uint32), np.array(lo, dtype=np.uint32),
            np.array(hi, dtype=np.uint32), np.array(sig_elem, dtype=np.uint64), np.array(nb, dtype=np.int32), np.array(na, dtype=np.int32))


def model_anchors(sigs, max_len=0):
    """what PFACX_clsigGetAnchors must return: (anchor_id, anchor_part, anchor_off, anchor_len) by id, and the distinct anchors"""
    cols, seen, anchors = [[0], [0], [0], [0]], {}, []
    for sig in sigs:
        part, at, length = choose_anchor(sig, max_len)
        key = fuse(sig)[part][1][at:at + length]
        if key not in seen:
            anchors.append(key)
            seen[key] = len(anchors)
        for col, value in zip(cols, (seen[key], part, at, length)):
            col.append(value)
    return tuple(np.array(c, np.int32) for c in cols), anchors


def _start_ok(sig, data, s):
    return s == 0 or sig[1] is None or data[s - 1] not in sig[1]


def _end_ok(sig, data, e):
    return e == len(data) or sig[2] is None or data[e] not in sig[2]


def ends_recursive(sig, data):
    """model 1: {start: the set of valid ends}, run length by run length"""
    data, elems, n = bytes(data), sig[0], len(data)

    @lru_cache(maxsize=None)
    def ends(k, o):
        if k == len(elems):
            return frozenset([o]) if _end_ok(sig, data, o) else frozenset()
        members, lo, hi = elems[k]
        out, r = set(), 0
        while True:
            if r >= lo:
                out |= ends(k + 1, o + r)
            if r == hi or o + r >= n or data[o + r] not in members:
                break
            r += 1
        return frozenset(out)

    found = {}
    for s in range(n):
        if _start_ok(sig, data, s):
            e = ends(0, s)
            if e:
                found[s] = set(e)
    return found


def _reach(elems, data, s):
    """sets of offsets: where the boundary behind `elems` can lie from start s"""
    reach, n = {s}, len(data)
    for members, lo, hi in elems:
        nxt = set()
        for o in reach:
            run = 0
            while run < hi and o + run < n and data[o + run] in members:
                run += 1
            nxt |= {o + r for r in range(lo, run + 1)}
        reach = nxt
        if not reach:
            break
    return reach


def ends_by_sets(sig, data):
    """model 2"""
    data, found = bytes(data), {}
    for s in range(len(data)):
        if _start_ok(sig, data, s):
            e = {o for o in _reach(sig[0], data, s) if _end_ok(sig, data, o)}
            if e:
                found[s] = e
    return found


def _split_line(line):
    """(the lookbehind or b'', the core, the lookahead or b'') of a text line"""
    line = bytes(line)
    sig = parse_line(line)
    front = b""
    if sig[1] is not None:
        front = line[:line.index(b"])") + 2]
    behind = b""
    if sig[2] is not None:
        behind = line[line.rindex(b"(?!["):]
    return front, line[len(front):len(line) - len(behind)], behind


def ends_re(line, data):
    """model 3: Python's re on the text line"""
    data = bytes(data)
    front, core, behind = _split_line(line)
    whole, start_ok, body = re.compile(front + core + behind, re.S), re.compile(front, re.S), re.compile(core, re.S)
    end_ok = re.compile(behind, re.S)
    reach = sum(hi for _, _, hi in parse_line(line)[0])
    found = {}
    for s in range(len(data)):
        if not start_ok.match(data, s):
            continue
        e = {e for e in range(s, min(len(data), s + reach) + 1) if body.fullmatch(data, s, e) and end_ok.match(data, e)}
        assert bool(e) == bool(whole.match(data, s)), f"re against itself at {s}"
        if e:
            found[s] = e
    return found


def owners(sig, data, anchor_part):
    """{start: (the owner offset x of the anchor part, the first offset of it that the head reaches)}"""
    data, elems, n = bytes(data), sig[0], len(data)
    first_elem = fuse(sig)[anchor_part][2]

    @lru_cache(maxsize=None)
    def completes(k, o):
        if k == len(elems):
            return _end_ok(sig, data, o)
        members, lo, hi = elems[k]
        r = 0
        while True:
            if r >= lo and completes(k + 1, o + r):
                return True
            if r == hi or o + r >= n or data[o + r] not in members:
                return False
            r += 1

    out = {}
    for s in range(n):
        if not _start_ok(sig, data, s):
            continue
        reach = _reach(elems[:first_elem], data, s)
        good = sorted(o for o in reach if completes(first_elem, o))
        if good:
            out[s] = (good[0], min(reach))
    return out


def owner_list(sigs, data, anchors, flags=0):
    """(pos, ids, end) in the order of the contract, and per entry (owner offset, first reachable offset)"""
    _, a_part, a_off, a_len = anchors
    found = []
    for i, sig in enumerate(sigs, 1):
        ends = ends_recursive(sig, data)
        own = owners(sig, data, int(a_part[i]))
        assert set(ends) == set(own), f"signature {i}: the two models disagree on which starts occur"
        pick = min if flags & SHORTEST else max
        found += [(own[s][0] + int(a_off[i]), -int(a_len[i]), -i, s, pick(ends[s]), own[s]) for s in ends]
    found.sort(key=lambda f: f[:4])
    col = lambda k, sign=1: np.array([sign * f[k] for f in found], dtype=np.int32)  # noqa: E731
    return (col(3), col(2, -1), col(4)), [f[5] for f in found]


def same(got, want, what):
    got, want = [np.asarray(a, dtype=np.int64) for a in got], [np.asarray(a, dtype=np.int64) for a in want]
    assert got[0].size == want[0].size, f"{what}: {got[0].size} entries, want {want[0].size}"
    bad = np.flatnonzero(np.any([g != w for g, w in zip(got, want)], axis=0)) if want[0].size else np.zeros(0, int)
    if bad.size:
        k = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} entries differ, first at {k}: got (pos, id, end) {[int(g[k]) for g in got]} want {[int(w[k]) for w in want]}")


def check_models(sigs, data, anchors, what, flags=0, lines=None):
    """the three models against each other on one input -> the list"""
    want, _ = owner_list(sigs, data, anchors, flags)
    for i, sig in enumerate(sigs, 1):
        one = ends_recursive(sig, data)
        assert ends_by_sets(sig, data) == one, f"{what}: signature {i}: sets of offsets against the recursion"
        if lines is not None:
            line = lines[i - 1]
            assert ends_re(line.encode("latin-1") if isinstance(line, str) else line, data) == one, f"{what}: signature {i}: re against the recursion"
    return want


# ---------------------------------------------------------------- the case table

SEP = b"|" * 70                                   # wider than any slack: nothing reaches across it
_PARTS64 = "".join(chr(97 + k % 26) + "[0-9]" for k in range(32))
_INST64 = bytes(b for k in range(32) for b in (97 + k % 26, 48 + k % 10))

# (name, the lines of the text form, input, maxAnchorLen, flags)
CASES = [
    ("one-literal-part", ["abc", "MZ\\x00\\x00PE", "a\\.c"], b"abc abd MZ\0\0PE abc a.c", 0, 0),
    ("class-k", ["AKIA[0-9A-Z]{4}"], b"AKIA0A1B AKIA0a1B AKIA012 AKIAZZZZZ", 0, 0),
    ("class-lo-hi-cut-three-ways", ["k=[0-9]{2,5}"], b"k=12x k=1234567 k=1 k=123", 0, 0),
    ("lo-0-with-an-empty-run", ["ab[0-9]{0,3}cd", "x\\d?y"], b"abcd ab12cd ab1234cd xy x1y x12y", 0, 0),
    ("two-class-parts-share-bytes", ["x[ab]{0,2}[bc]{0,2}y"], b"xabbcy xy xaay xbby xbbby xabcy xcay xbbbby", 0, 0),
    ("end-lazy-dead-end", ["a.?[`-o].?[c][dD]"], b"abccd", 0, SHORTEST),
    ("largest-end-needs-a-shorter-early-run", ["k[ab]{1,3}b[c]{0,3}"], b"kabbc kabc kabbbcccc", 0, 0),
    ("owner-both-complete", ["a.{0,2}KK.{0,2}z"], b"aKKK.z", 0, 0),
    ("owner-nearer-dead", ["a.{0,2}KK[zZ]"], b"aKKKz", 0, 0),
    ("owner-nearer-only-to-forbidden-ends", ["a.{0,2}KK.{1,2}(?![0-9])"], b"aKKK12;", 0, 0),
    ("not-before", ["(?<![0-9])[0-9]{3}-x"], b"123-x 9123-x a123-x", 0, 0),
    ("not-after-at-the-input-end", ["tok=[a-f]{2,4}(?![a-f])"], b"tok=abcdef tok=abc", 0, 0),
    ("slack-63", ["ab.{0,63}yz", "A[0-9]{0,31}B[0-9]{0,32}C"],
     SEP.join(b"ab" + b"." * d + b"yz" for d in (0, 63, 64)) + SEP + b"A" + b"1" * 31 + b"B" + b"2" * 32 + b"C" + SEP + b"ABC" + SEP + b"A" + b"1" * 32 + b"BC", 0, 0),
    ("64-parts", [_PARTS64], _INST64 + b" " + _INST64[:-1] + b"x " + _INST64, 0, 0),
    ("identical-signatures", ["id[0-9]{1,2};", "id[0-9]{1,2};"], b"id1; id22; id333;", 0, 0),
    ("a-shared-anchor", ["key=[0-9]{1,3};", "key=[a-f]{2}", "[A-Z]{2}key="], b"key=12; key=ab XYkey=7; key=1234;", 0, 0),
    ("anchor-prefix-chain", ["ab[0-9]{1,2}", "abcd[0-9]{1,2}", "abc[x-z]"], b"abcd12 ab1 abcx abcd ab12", 0, 0),
    ("literal-with-a-newline", ["ab\\ncdef[0-9]{1,2}"], b"ab\ncdef12 abcdef1 ab\ncdef", 0, 0),
    ("negated-set", ['q="[^"\\\\]{1,8}"'], b'q="abc" q="" q="a\nb" q="123456789" q="a\\b"', 0, 0),
    ("full-class", ["MZ.{2,4}PE"], b"MZ..PE MZ.PE MZ\n\n\n\nPE MZ.....PE", 0, 0),
    ("anchor-cut", ["abcdef[0-9]", "[0-9]abcxyz"], b"abcdef1 1abcxyz abcde1", 3, 0),
    ("shortest-and-largest", ["t[a-c]{1,4}[c-e]{0,3}"], b"tabccde tc", 0, SHORTEST),
]
# worked out by hand: name -> (ids, starts, ends)
WANT = {
    "end-lazy-dead-end": ([1], [0], [5]),
    "owner-both-complete": ([1], [0], [6]),
    "owner-nearer-dead": ([1], [0], [5]),
    "owner-nearer-only-to-forbidden-ends": ([1], [0], [6]),
    "not-before": ([1, 1], [0, 14], [5, 19]),
    "not-after-at-the-input-end": ([1], [11], [18]),
    "class-lo-hi-cut-three-ways": ([1, 1, 1], [0, 6, 20], [4, 13, 25]),
    "identical-signatures": ([2, 1, 2, 1], [0, 0, 5, 5], [4, 4, 10, 10]),
    "largest-end-needs-a-shorter-early-run": ([1, 1, 1], [0, 6, 11], [5, 10, 19]),
}


def case_sigs(case):
    return parse_lines(case[1])


def test_the_models_agree_on_every_case():
    for name, lines, data, cut, flags in CASES:
        sigs = parse_lines(lines)
        assert all(check_limits(s) is None for s in sigs), name
        for line in lines:
            re.compile(line.encode("latin-1"), re.S)
        anchors, _ = model_anchors(sigs, cut)
        want = check_models(sigs, data, anchors, name, flags, lines)
        if name in WANT:
            ids, pos, end = WANT[name]
            same(want, (pos, ids, end), f"{name}: the models against the list worked out by hand")
        assert want[0].size > 0, name
    # the cases hold what they are meant to
    by = {c[0]: c for c in CASES}
    assert owners(case_sigs(by["owner-both-complete"])[0], b"aKKK.z", 2) == {0: (1, 1)}
    assert owners(case_sigs(by["owner-nearer-dead"])[0], b"aKKKz", 2) == {0: (2, 1)}, "the owner is not the first offset the head reaches"
    assert owners(case_sigs(by["owner-nearer-only-to-forbidden-ends"])[0], b"aKKK12;", 2) == {0: (2, 1)}
    assert len(fuse(case_sigs(by["64-parts"])[0])) == 64 and sum(hi - lo for _, lo, hi in case_sigs(by["slack-63"])[0][0]) == 63
    assert len(ends_recursive(case_sigs(by["slack-63"])[0], by["slack-63"][2])) == 2, "distances 0 and 63, not 64"
    assert choose_anchor(case_sigs(by["literal-with-a-newline"])[0]) == (0, 3, 4)
    assert ends_recursive(case_sigs(by["shortest-and-largest"])[0], b"tabccde tc") == {0: {2, 3, 4, 5, 6, 7}, 8: {10}}
    assert choose_anchor(parse_line(b"[0-9]{3}[a-f]{2}")) is None and choose_anchor(parse_line(b"\\n[0-9]")) is None
    for line in REFUSED_LINES:
        try:
            parse_line(line)
        except ValueError:
            continue
        raise AssertionError(f"{line!r} must be refused")


# lines the text form refuses (each on its own)
REFUSED_LINES = [b"a*", b"a+", b"a|b", b"(ab)", b"^ab", b"ab$", b"a{2,}", b"a{,2}", b"a{3,2}", b"{2}a", b"?a", b"a{2}{3}", b"a{2}?", b"a??", b"a[bc",
                 b"a[]", b"a[^]", b"a[z-a]", b"a\\q", b"a\\xZ1", b"a\\x4", b"a{65536}", b"a{1,65536}", b"", b"a]", b"a}", b"a)", b"a{ 2}", b"a{2 }",
                 b"a{}", b"a{x}", b"a\\", b"a[\\d-z]", b"a[a-\\d]", b"a(?![0-9])b", b"a(?<![0-9])", b"(?<!a)b", b"a(?!b)", b"(?<![0-9])", b"a\\01",
                 b"a(?=[0-9])", b"a[^\\x00-\\xff]", b"a\\-b"]


# ---------------------------------------------------------------- the seeded random case (tests/test_clsig_*.py)

_POOL = [_DIGIT, frozenset(range(97, 103)) | _DIGIT, frozenset(range(65, 91)), _WORD, _ALL, _ALL - frozenset(b'"\n'), frozenset(b"ab"), frozenset(b"bc")]


def random_signatures(seed, count=200):
    """token rules: a literal of 3 .. 10 bytes from a 6-letter alphabet (so anchors repeat and prefix each other) at the front, in the middle or
    at the end, one to three class runs with a slack of at most 63 in all, boundaries on half of them"""
    rng = np.random.default_rng(seed)
    sigs = []
    for _ in range(count):
        slack, elems = 0, []
        runs = int(rng.integers(1, 4))
        place = int(rng.integers(0, runs + 1))
        for k in range(runs + 1):
            if k == place:
                elems += [(frozenset([int(b)]), 1, 1) for b in rng.choice(list(b"kKeyx="), size=int(rng.integers(3, 11)))]
                continue
            lo = int(rng.integers(0, 6))
            width = min(int(rng.integers(0, 12)), MAX_SLACK - slack)
            slack += width
            elems.append((_POOL[int(rng.integers(0, len(_POOL)))], lo, max(1, lo + width)))
            if rng.integers(0, 3) == 0:
                elems.append((frozenset([int(rng.choice(list(b";-:")))]), 1, 1))
        nb = _POOL[int(rng.integers(0, 4))] if rng.integers(0, 2) else None
        na = _POOL[int(rng.integers(0, 4))] if rng.integers(0, 2) else None
        sigs.append((elems, nb, na))
    return sigs


def embed(sigs, data, seed, per_sig=3):
    """`data` (uint8, modified in place) with per_sig instances of every signature at random places with random run lengths"""
    rng = np.random.default_rng(seed + 1)
    n = data.size
    for elems, _, _ in sigs:
        for _ in range(per_sig):
            body = []
            for members, lo, hi in elems:
                pool = np.array(sorted(members), dtype=np.uint8)
                body.append(pool[rng.integers(0, pool.size, int(rng.integers(lo, hi + 1)))])
            body = np.concatenate(body)
            at = int(rng.integers(0, n - body.size + 1))
            data[at:at + body.size] = body
    return data


def random_case(seed=20261023, count=200, n=1 << 16):
    sigs = random_signatures(seed, count)
    data = embed(sigs, np.random.default_rng(seed + 2).integers(0, 256, n, dtype=np.uint8), seed)
    return sigs, data


def fast_list(sigs, data, anchors, flags=0):
    """the list of the random case: the models above restricted to the starts that a numpy search for the anchor bytes leaves (an occurrence has
    its anchor part somewhere within the span behind its start), so that 200 signatures over 64 KiB take seconds -> (list, figures)"""
    raw = bytes(data)
    _, a_part, a_off, a_len = anchors
    found, late, multi = [], 0, {}
    for i, sig in enumerate(sigs, 1):
        parts = fuse(sig)
        anchor = parts[int(a_part[i])][1][int(a_off[i]):int(a_off[i]) + int(a_len[i])]
        head_hi = sum(hi for _, _, hi in sig[0][:parts[int(a_part[i])][2]]) + int(a_off[i])
        starts = set()
        for m in re.finditer(b"(?=" + re.escape(anchor) + b")", raw, re.S):
            starts |= set(range(max(0, m.start() - head_hi), m.start() + 1))
        for s in sorted(starts):
            lo_cut = s
            hi_cut = min(len(raw), s + sum(hi for _, _, hi in sig[0]) + 1)
            piece = raw[max(0, lo_cut - 1):hi_cut + 1]
            shift = max(0, lo_cut - 1)
            ends = ends_recursive(sig, piece).get(s - shift)
            if hi_cut + 1 < len(raw) and ends:                      # the cut is no input end: an end there needs its boundary test on the real byte
                ends = {e for e in ends if e + shift < hi_cut + 1 or _end_ok(sig, raw, e + shift)}
            if not ends:
                continue
            own = owners(sig, piece, int(a_part[i])).get(s - shift)
            if own is None:
                continue
            x, first = own[0] + shift, own[1] + shift
            late += x != first
            multi[(i, x)] = multi.get((i, x), 0) + 1
            pick = min if flags & SHORTEST else max
            found.append((x + int(a_off[i]), -int(a_len[i]), -i, s, pick(ends) + shift))
    found.sort(key=lambda f: f[:4])
    col = lambda k, sign=1: np.array([sign * f[k] for f in found], dtype=np.int32)  # noqa: E731
    figures = {"entries": len(found), "late_owner": int(late), "multi_start": sum(1 for c in multi.values() if c > 1)}
    return (col(3), col(2, -1), col(4)), figures
