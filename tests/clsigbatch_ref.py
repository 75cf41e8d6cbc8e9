"""What the two batch files of the class-signature calls share (tests/test_clsigbatch_host.py, tests/test_clsigbatch_gpu.py): the batch list as
the contract states it -- the models of tests/clsig_ref.py run on each segment's bytes ALONE, shifted by the segment's offset, concatenated in
segment order --, the clamp a device call applies to hostile offsets, the table of window-edge cases with the lists worked out by hand, and the
seeded cuts of the random case.  Nothing here knows how the library finds a pair's segment.  Test infrastructure only."""

import numpy as np

from tests import clsig_ref as ref

SHORTEST = ref.SHORTEST


def clamp_offsets(offsets, size):
    """what a device form makes of its offsets: each clamped to [0, size], then raised to the largest entry in front of it"""
    o = np.clip(np.asarray(offsets, dtype=np.int64), 0, size) if len(offsets) else np.zeros(0, np.int64)
    return np.maximum.accumulate(o)


def offsets_of(segments):
    return np.concatenate([[0], np.cumsum([len(s) for s in segments])]).astype(np.int64)


def batch_model(sigs, data, offsets, anchors, flags=0, lines=None, fast=False):
    """-> ((pos, ids, end), seg_first): per segment the plain list of its bytes alone (every model against the others, or fast_list for the
    random case), o_k added; bytes in front of offsets[0] or behind offsets[-1] belong to no segment"""
    raw = bytes(np.asarray(data, dtype=np.uint8).tobytes()) if not isinstance(data, (bytes, bytearray)) else bytes(data)
    cols, first, total = [[], [], []], [], 0
    for k in range(len(offsets) - 1):
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        first.append(total)
        if hi <= lo:
            continue
        piece = raw[lo:hi]
        if fast:
            want, _ = ref.fast_list(sigs, np.frombuffer(piece, dtype=np.uint8), anchors, flags)
        else:
            want = ref.check_models(sigs, piece, anchors, f"segment {k}", flags, lines)
        cols[0] += [int(p) + lo for p in want[0]]
        cols[1] += [int(i) for i in want[1]]
        cols[2] += [int(e) + lo for e in want[2]]
        total += int(want[0].size)
    first.append(total)
    return tuple(np.array(c, dtype=np.int32) for c in cols), np.array(first, dtype=np.uint64)


def triples(lists):
    pos, ids, end = lists
    return sorted(zip((int(i) for i in ids), (int(p) for p in pos), (int(e) for e in end)))


# ---------------------------------------------------------------- window edges
# (name, lines, max anchor length, the segments, {flags: [(id, start, end)] worked out by hand, sorted} or None)
# Starts and ends count from the first byte of the first segment.

FULL = "[\\x00-\\xff]"
_AK1, _AK2 = b"..AKIA0123", b"456789ABCDEF.."

EDGE_CASES = [
    # an embedding that completes only across a boundary is not listed; the same bytes in one segment are
    ("crossing", ["AKIA[0-9A-Z]{16}"], 0, [_AK1, _AK2, _AK1 + _AK2], {0: [(1, 26, 46)], SHORTEST: [(1, 26, 46)]}),
    # flat: k=12345 ends at 7.  The batch: the run is cut at 4.  With the lookahead the flat call has the end 7 alone; the edge makes 4 valid
    ("a-crossing-embedding-hides-a-shorter-one", ["k=[0-9]{2,5}", "k=[0-9]{2,5}(?![0-9])", "k=[0-9]{1,5}"], 0, [b"k=12", b"345 k=678"],
     {0: [(1, 0, 4), (1, 8, 13), (2, 0, 4), (2, 8, 13), (3, 0, 4), (3, 8, 13)], SHORTEST: [(1, 0, 4), (1, 8, 12), (2, 0, 4), (2, 8, 13), (3, 0, 3), (3, 8, 11)]}),
    # a token at a segment's first and last byte whose neighbours in the other segments are in notBefore / notAfter is listed; inside one segment
    # the same bytes forbid it
    ("boundary-classes-do-not-see-the-neighbour", ["(?<![0-9])tok[a-f]{2}(?![a-f])"], 0, [b"..5", b"tokab", b"c..", b"5tokab", b"tokabc", b".5tokabc"],
     {0: [(1, 3, 8)], SHORTEST: [(1, 3, 8)]}),
    # a full notBefore class: only at o_k; a full notAfter class: only where the segment ends
    ("full-boundary-classes", ["(?<!" + FULL + ")GET /", "END(?!" + FULL + ")", "(?<!" + FULL + ")[a-z]{0,2}=1(?!" + FULL + ")"], 0,
     [b"GET /a GET /b", b"xGET /cEND", b"GET /END.", b"END", b"a=1", b"abc=1", b"=1", b"b=1."],
     {0: [(1, 0, 5), (1, 23, 28), (2, 20, 23), (2, 32, 35), (3, 35, 38), (3, 43, 45)]}),
    # a class run is cut by o_{k+1} going forwards and by o_k going backwards
    ("class-runs-are-cut-at-both-edges", ["wxyz[a-z]{2,9}", "[a-z]{0,5}WXYZ", "wxyz[a-z]{4,9}"], 0, [b"wxyzabc", b"defgh", b"abc", b"deWXYZ"],
     {0: [(1, 0, 7), (2, 15, 21), (2, 16, 21), (2, 17, 21)]}),
    # the longest anchor at p crosses the boundary while its prefix anchor fits
    ("the-longest-anchor-crosses-and-its-prefix-fits", ["abcdef[0-9]", "abc[x-z]?", "abcd"], 0, [b"..abc", b"def1", b".abcd", b"ef1"],
     {0: [(2, 2, 5), (2, 10, 13), (3, 10, 14)]}),
    # the anchor part at x == o_k exactly, and one byte in front of it (the anchor `cdef` lies 3 bytes into its literal part)
    ("the-anchor-part-at-the-segment-start-and-in-front-of-it", ["[Q]?Rabc", "ab\\ncdef[0-9]{1,2}"], 0,
     [b"..Q", b"Rabc", b"QRabc", b"xa", b"b\ncdef1", b"ab\ncdef12", b"ab\n", b"cdef1"],
     {0: [(1, 3, 7), (1, 7, 12), (1, 8, 12), (2, 21, 30)]}),
    # segment lengths 0, 1, the anchor's length, the anchor's length - 1
    ("segment-lengths-around-the-anchor", ["abc", "a[0-9]?", "[0-9]?abc"], 0, [b"", b"a", b"abc", b"ab", b"c", b"", b"", b"abc", b"1", b"abc", b"a1", b""], None),
]


def edge_batch(case, lead=0):
    """the case's bytes and offsets behind a first segment of `lead` filler bytes (every segment start moves by it) -> (data, offsets, lead)"""
    segments = [b"~" * lead] + list(case[3])
    return np.frombuffer(b"".join(segments), dtype=np.uint8), offsets_of(segments)


def edge_want(case, flags, lead=0):
    by_hand = case[4].get(flags) if case[4] else None
    return None if by_hand is None else [(i, s + lead, e + lead) for i, s, e in by_hand]


# ---------------------------------------------------------------- offsets that are no offsets (n: the size of the buffer, at least 12)

HOSTILE = [
    ("decreasing", lambda n: [0, n // 2, n // 3, n]),
    ("above-size", lambda n: [0, n // 2, n + 5, n]),
    ("first-above-zero", lambda n: [3, n // 2, n]),
    ("last-below-size", lambda n: [0, n // 2, n - 4]),
    ("far-above-size", lambda n: [0, 2 ** 63, n]),
]

# ---------------------------------------------------------------- block edges: one pair per byte

RUN_LINES = ["a[a]{0,1}a[b-z]?", "a[0-9]{1,3}b"]                   # tests/test_clsig_gpu.py: every 'a' is a pair; the second one never holds


def run_want(offsets):
    """the list of RUN_LINES over a buffer of 'a's by the rule itself: signature 1 at every start with a second 'a' inside its segment, the end
    one further where a third one is"""
    pos, end, first = [], [], []
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        first.append(len(pos))
        for s in range(int(lo), int(hi) - 1):
            pos.append(s)
            end.append(min(s + 3, int(hi)))
    first.append(len(pos))
    return (np.array(pos, np.int32), np.ones(len(pos), np.int32), np.array(end, np.int32)), np.array(first, np.uint64)


# ---------------------------------------------------------------- the seeded random case

RANDOM_SEED, DELIMITERS = 20261103, 4          # chosen with the models alone: 1 131 segments, 299 crossings lost, 12 entries freed by an edge


def random_cuts(data, seed=RANDOM_SEED, delimiters=DELIMITERS):
    """offsets that cut `data` IN FRONT of every byte of a seeded delimiter class (what PFACX_split* gives with PFACX_SPLIT_BEFORE): records of
    some 60 bytes on average, many of them shorter than a token, some that start right behind one"""
    cls = np.random.default_rng(seed).choice(256, size=delimiters, replace=False)
    cuts = np.flatnonzero(np.isin(data, cls))
    return np.concatenate([[0], cuts[cuts > 0], [data.size]]).astype(np.int64)


def random_batch():
    """-> (sigs, data, offsets)"""
    sigs, data = ref.random_case()
    return sigs, data, random_cuts(data)


def crossing_figures(flat, batch):
    """(entries of the flat list whose (id, start) the batch list lacks, entries of the batch list whose (id, start) the flat list lacks)"""
    f = set(zip(flat[1].tolist(), flat[0].tolist()))
    b = set(zip(batch[1].tolist(), batch[0].tolist()))
    return len(f - b), len(b - f)
