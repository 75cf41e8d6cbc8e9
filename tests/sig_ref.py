"""References for the signature calls (PFACX_sig*: masked byte signatures with wildcards) that share no code with the library.

parse_line          one line of the text form -> (values, masks) uint8, by the rules of include/pfac_ext.h; ValueError for a line it refuses
choose_anchor       the documented choice rule: the longest run of mask-0xFF bytes other than 0x0A, the leftmost of equal ones, cut
sig_brute           the definition: per signature a numpy masked compare at every start
sig_re              Python's re in bytes mode: a wildcard byte is `.` under DOTALL, any other mask a class of the bytes it admits (16 members for
                    a half byte), the whole inside a lookahead so that overlapping occurrences are found
Both return (pos, ids) int32 in the order of the contract: anchor position start + anchor_off[id] ascending, at one anchor position the longer
anchor first, within one anchor ids descending -- NOT sorted by start.  anchor_off / anchor_len are indexed by id (entry 0 unused): the tests pass
what the library's own PFACX_sigGetAnchors returned.  Test infrastructure only."""

import re

import numpy as np

DEFAULT_ANCHOR = 32


def parse_line(line):
    """b'4D 5a ?? 5? ?3' -> (values, masks); the line without its '\\n' (a '\\r' at its end is dropped)"""
    line = bytes(line)
    if line.endswith(b"\r"):
        line = line[:-1]
    values, masks = [], []
    j = 0
    while j < len(line):
        if line[j:j + 1] in (b" ", b"\t"):
            j += 1
            continue
        pair = line[j:j + 2]
        if len(pair) < 2 or any(c not in b"0123456789abcdefABCDEF?" for c in pair):
            raise ValueError(f"refused at byte {j}")
        hi, lo = chr(pair[0]), chr(pair[1])
        values.append((0 if hi == "?" else int(hi, 16) << 4) | (0 if lo == "?" else int(lo, 16)))
        masks.append((0 if hi == "?" else 0xF0) | (0 if lo == "?" else 0x0F))
        j += 2
    if not values:
        raise ValueError("an empty line")
    return np.array(values, dtype=np.uint8), np.array(masks, dtype=np.uint8)


def parse_lines(lines):
    return [parse_line(line.encode() if isinstance(line, str) else line) for line in lines]


def text_of(lines):
    return b"".join((line.encode() if isinstance(line, str) else bytes(line)) + b"\n" for line in lines)


def csr_of(sigs):
    """[(values, masks)] -> (values, masks, offsets) as PFACX_sigOpen takes them"""
    off = np.zeros(len(sigs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(v) for v, _ in sigs])
    cat = lambda k: np.concatenate([np.asarray(s[k], dtype=np.uint8) for s in sigs]) if sigs else np.zeros(0, np.uint8)  # noqa: E731
    return cat(0), cat(1), off


def choose_anchor(values, masks, max_len=0):
    """(offset, length) of the anchor, None for a signature without a candidate byte"""
    cut = max_len or DEFAULT_ANCHOR
    best, at, i, n = 0, 0, 0, len(values)
    while i < n:
        if masks[i] != 0xFF or values[i] == 0x0A:
            i += 1
            continue
        j = i
        while j < n and masks[j] == 0xFF and values[j] != 0x0A:
            j += 1
        if j - i > best:
            best, at = j - i, i
        i = j
    return (at, min(best, cut)) if best else None


def model_anchors(sigs, max_len=0):
    """what PFACX_sigGetAnchors must return, by the documented rule: (anchor_id, anchor_off, anchor_len) indexed by id, and the distinct anchors"""
    ids, offs, lens, seen, anchors = [0], [0], [0], {}, []
    for v, m in sigs:
        at, length = choose_anchor(v, m, max_len)
        key = bytes(np.asarray(v, dtype=np.uint8)[at:at + length] & np.asarray(m, dtype=np.uint8)[at:at + length])
        if key not in seen:
            anchors.append(key)
            seen[key] = len(anchors)
        ids.append(seen[key])
        offs.append(at)
        lens.append(length)
    return (np.array(ids, np.int32), np.array(offs, np.int32), np.array(lens, np.int32)), anchors


def _ordered(found, anchor_off, anchor_len):
    """found: [(id, start)] -> (pos, ids) in the order of the contract"""
    found = sorted(found, key=lambda f: (f[1] + int(anchor_off[f[0]]), -int(anchor_len[f[0]]), -f[0]))
    return np.array([f[1] for f in found], dtype=np.int32), np.array([f[0] for f in found], dtype=np.int32)


def starts_of(values, masks, data):
    """every start at which one signature occurs: a masked compare of all candidate starts, byte by byte of the signature"""
    data = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.asarray(data, dtype=np.uint8)
    v, m = np.asarray(values, dtype=np.uint8) & np.asarray(masks, dtype=np.uint8), np.asarray(masks, dtype=np.uint8)
    length, n = len(v), data.size
    if length > n:
        return np.zeros(0, dtype=np.int64)
    at = np.arange(n - length + 1, dtype=np.int64)
    for k in range(length):
        if m[k] and at.size:
            at = at[((data[at + k] ^ v[k]) & m[k]) == 0]
    return at


def sig_brute(sigs, data, anchor_off, anchor_len):
    found = []
    for i, (v, m) in enumerate(sigs):
        found.extend((i + 1, int(s)) for s in starts_of(v, m, data))
    return _ordered(found, anchor_off, anchor_len)


def regex_of(values, masks):
    parts = []
    for v, m in zip(np.asarray(values, dtype=np.uint8).tolist(), np.asarray(masks, dtype=np.uint8).tolist()):
        if m == 0xFF:
            parts.append(b"\\x%02x" % (v & m))
        elif m == 0:
            parts.append(b".")
        else:
            members = [b for b in range(256) if ((b ^ v) & m) == 0]
            assert m not in (0xF0, 0x0F) or len(members) == 16
            parts.append(b"[" + b"".join(b"\\x%02x" % b for b in members) + b"]")
    return re.compile(b"(?=" + b"".join(parts) + b")", re.S)


def sig_re(sigs, data, anchor_off, anchor_len):
    raw = bytes(data)
    found = []
    for i, (v, m) in enumerate(sigs):
        found.extend((i + 1, match.start()) for match in regex_of(v, m).finditer(raw))
    return _ordered(found, anchor_off, anchor_len)


def same(got, want, what):
    (gp, gi), (wp, wi) = got, want
    gp, gi, wp, wi = (np.asarray(a, dtype=np.int64) for a in (gp, gi, wp, wi))
    assert gp.size == wp.size, f"{what}: {gp.size} entries, want {wp.size}"
    bad = np.flatnonzero((gp != wp) | (gi != wi))
    if bad.size:
        k = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} entries differ, first at {k}: got ({gi[k]}, {gp[k]}) want ({wi[k]}, {wp[k]})")


def check_models(sigs, data, anchor_off, anchor_len, what):
    """the model against re on one test input -> the model's list"""
    want = sig_brute(sigs, data, anchor_off, anchor_len)
    same(sig_re(sigs, data, anchor_off, anchor_len), want, f"{what}: re against the masked compare")
    return want


# ---------------------------------------------------------------- the compare edges

EDGE_LENGTHS = [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 64]


def edge_signature(length, kind="exact"):
    """a signature of `length` bytes that starts with its own letter and goes on with bytes no other edge signature has; kind: exact, or with a
    wildcard at `first`, at `last`, or at every byte `but-anchor` (then the anchor is byte 0 alone... or the middle byte for kind `middle`)"""
    k = EDGE_LENGTHS.index(length)
    values = np.array([0x41 + k] + [0x80 + ((7 * i + 13 * k) % 0x70) for i in range(1, length)], dtype=np.uint8)
    masks = np.full(length, 0xFF, dtype=np.uint8)
    if kind == "first" and length > 1:
        masks[0] = 0
    elif kind == "last" and length > 1:
        masks[-1] = 0
    elif kind == "but-anchor":
        masks[1:] = 0
    elif kind == "middle":
        masks[:] = 0
        masks[length // 2] = 0xFF
    elif kind == "halves" and length > 1:
        masks[0], masks[-1] = 0xF0, 0x0F
    return values, masks


def edge_input(lengths=EDGE_LENGTHS):
    """every exact edge signature as it is, then with only its last byte and only its first byte changed; the pieces have many lengths, so the
    occurrences start at every residue mod 4; the buffer ends with an occurrence, behind one cut short by n"""
    pieces = []
    for k, length in enumerate(lengths):
        v = bytes(edge_signature(length)[0])
        pieces += [v, v[:-1] + bytes([v[-1] ^ 0x01]), bytes([v[0] ^ 0x10]) + v[1:], b"-" * (k % 3)]
    longest = bytes(edge_signature(lengths[-1])[0])
    return b" ".join(pieces) + b" " + longest[:-1] + b" " + bytes(edge_signature(33)[0])


# ---------------------------------------------------------------- the seeded random case (tests/test_sig_gpu.py, tools/sig_sweep.py)


def random_signatures(seed, count=200, min_len=16, max_len=200, max_wild=0.20):
    """`count` signatures of min_len .. max_len bytes with 0 .. max_wild wildcard bytes (one in four of them a half byte), never the first byte"""
    rng = np.random.default_rng(seed)
    sigs = []
    for _ in range(count):
        length = int(rng.integers(min_len, max_len + 1))
        values = rng.integers(0, 256, length, dtype=np.uint8)
        masks = np.full(length, 0xFF, dtype=np.uint8)
        wild = rng.choice(np.arange(1, length), size=int(rng.uniform(0, max_wild) * length), replace=False)
        for at in wild:
            masks[at] = (0xF0, 0x0F)[int(rng.integers(0, 2))] if rng.integers(0, 4) == 0 else 0x00
        sigs.append((values, masks))
    return sigs


def embed(sigs, data, seed, per_sig=3, near_misses=1):
    """`data` (uint8, modified in place) with per_sig occurrences of every signature at random places, wildcards filled with random bytes, and
    near misses: the same with one masked bit flipped"""
    rng = np.random.default_rng(seed + 1)
    n = data.size
    for v, m in sigs:
        length = len(v)
        if length > n:
            continue
        for k in range(per_sig + near_misses):
            at = int(rng.integers(0, n - length + 1))
            body = (v & m) | (rng.integers(0, 256, length, dtype=np.uint8) & ~m)
            if k >= per_sig:
                where = int(rng.choice(np.flatnonzero(m)))
                body[where] ^= np.uint8(int(m[where]) & -int(m[where]))            # the lowest masked bit
            data[at:at + length] = body
    return data


def random_case(seed=20261021, count=200, n=1 << 16):
    sigs = random_signatures(seed, count)
    data = embed(sigs, np.random.default_rng(seed + 2).integers(0, 256, n, dtype=np.uint8), seed)
    return sigs, data


# ---------------------------------------------------------------- the case table (tools/sig_host_san.cpp has the same table)

# (name, the lines of the text form, input)
CASES = [
    ("mz-pe", ["4D 5A ?? ?? 50 45 00 00"], b"MZ\x90\x00PE\x00\x00 MZxyPE\x00\x01 MZPE\x00\x00 xMZ\n\nPE\x00\x00"),
    ("call-pop-ret", ["E8 ?? ?? ?? ?? 5? C3"], b"\xe8\x01\x02\x03\x04\x5b\xc3 \xe8\xe8\xe8\xe8\xe8\x5f\xc3\xc3 \xe8\x00\x00\x00\x00\x6b\xc3 \xe8\x00\x00\x00\x00\x50\xc2"),
    ("text-rule", ["69 64 3D ?? ?? ?? ?? 3B"], b"id=1234; id=12345; id=;;;;; xid=\n\r\t ;id=123;"),
    ("both-halves", ["4? ?1 41", "?1 4? 41"], b"AAA OQA QOA Oa A\x11A\x41\x41 \x41\x4fA"),
    ("anchor-in-the-middle", ["?? ?? 61 62 63 ?? ??"], b"abc..xabc..xxabc..xxxabcxxabcxxabc.abcx"),
    ("newline-outside-the-anchor", ["0A 61 62 0A", "61 62 0A 0A 63"], b"\nab\n ab\n\nc \nab \nab\n\nc xab\n"),
    ("only-newline-neighbours", ["0A 0A 41 0A"], b"\n\nA\n \n\nA \nA\n\n\nA\n"),
    ("an-anchor-is-a-prefix-of-another", ["61 62 ?? 64", "61 62 63 ??", "?? 61 62 63", "61 62 63"], b"abcd abxd abc xabc abcabcd"),
    ("identical-signatures", ["61 ?? 63", "61 ?? 63"], b"abc axc"),
    ("one-anchor-at-several-offsets", ["?? ?? 61 62", "61 62 ??", "?? 61 62"], b"xxabyab"),
    ("single-bytes", ["61", "62", "61"], b"abab"),
    ("equal-runs-the-leftmost-wins", ["61 62 ?? 63 64", "?? 63 64 ?? 61 62"], b"abxcd cdxab xcdxab abcd"),
    ("a-half-byte-splits-a-run", ["61 62 6? 64 65 66"], b"abcdef abxdef abkdef abCdef"),
    ("compare-edges", None, edge_input()),          # the lines: edge_lines()
]
# what the definition gives, worked out by hand: name -> (ids, starts)
WANT = {
    "identical-signatures": ([2, 1, 2, 1], [0, 0, 4, 4]),
    "one-anchor-at-several-offsets": ([3, 2, 1, 3, 1], [1, 2, 0, 4, 3]),       # anchor positions 2, 2, 2, 5, 5: not sorted by start
    "mz-pe": ([1, 1], [0, 26]),                                                # the second one with both newlines under its wildcards
}


def hex_line(values, masks):
    out = []
    for v, m in zip(np.asarray(values).tolist(), np.asarray(masks).tolist()):
        text = "%02X" % (v & m)
        out.append(("?" if not m & 0xF0 else text[0]) + ("?" if not m & 0x0F else text[1]))
    return " ".join(out)


def edge_lines():
    """per edge length: exact, a wildcard first byte, a wildcard last byte, every byte but the anchor, the anchor in the middle, half bytes at
    both ends"""
    return [hex_line(*edge_signature(length, kind)) for length in EDGE_LENGTHS for kind in ("exact", "first", "last", "but-anchor", "middle", "halves")]


def case_lines(case):
    return edge_lines() if case[1] is None else case[1]


def test_the_models_agree_on_every_case():
    for case in CASES:
        name, data = case[0], case[2]
        sigs = parse_lines(case_lines(case))
        (_, off, length), _ = model_anchors(sigs)
        brute = check_models(sigs, data, off, length, name)
        if name in WANT:
            ids, pos = WANT[name]
            same(brute, (pos, ids), f"{name}: the masked compare against the list worked out by hand")
        assert brute[0].size > 0, name
    # the edges hold what they are meant to: each exact signature occurs exactly where it stands unchanged (33: twice), at every residue mod 4
    exact = [edge_signature(length) for length in EDGE_LENGTHS]
    (_, off, length), _ = model_anchors(exact)
    pos, ids = sig_brute(exact, edge_input(), off, length)
    assert np.bincount(ids, minlength=len(exact) + 1).tolist() == [0] + [1] * 9 + [2, 1]
    assert int(pos[-1]) + 33 == len(edge_input()), "the buffer ends with an occurrence"
    assert set(int(p) & 3 for p in pos) == {0, 1, 2, 3}, "occurrences at every residue mod 4"
    assert choose_anchor(*parse_line(b"0A")) is None and choose_anchor(*parse_line(b"?? 4?")) is None
    assert choose_anchor(*parse_line(b"61 62 ?? 63 64")) == (0, 2) and choose_anchor(*parse_line(b"61 ?? 63 64 0A 65 66 67")) == (5, 3)
    assert choose_anchor(*parse_line(b"61 62 63 64"), 3) == (0, 3)
