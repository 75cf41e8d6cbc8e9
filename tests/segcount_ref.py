"""References for the batch count calls (PFACX_countBatch*) that share no code with the library or with each other.

segcounts_py           per segment, the all-match list of the segment's bytes ALONE by brute force (tests/allmatch_ref.py: every position, every pattern
                       length, a dict lookup) through np.unique(..., return_counts=True); longest: the first pair of each position alone
segcounts_from_result  numpy: a per-segment longest vector (the concatenation of the longest-match vectors of the segments, what PFACX_matchBatch*
                       returns) pushed up the prefix table level by level, one np.unique over segment * (F + 1) + id keys
batch_result           that per-segment vector from the longest vector of the WHOLE buffer: every pattern at a position is on the chain of the longest
                       one there, so a segment's longest pattern at a position is the first chain member that ends inside the segment
All lists are (segFirst uint64[numSegments + 1], ids int32, counts uint32): the entries with a non-zero count in ascending (segment, id) order.
Also the case table both test files share and the generator of fixed-width sets.  Test infrastructure only."""

import numpy as np

from tests import allmatch_ref as am
from tests import count_ref
from tests.count_ref import NESTED, fold


def segcounts_py(pats, data, offsets=None, nocase=False, longest=False):
    """offsets: numSegments + 1 ascending byte offsets into data (None: one segment); segment k is data[offsets[k]:offsets[k + 1]]"""
    data = bytes(data)
    offsets = [0, len(data)] if offsets is None else [int(o) for o in offsets]
    if nocase:
        pats, data = [fold(p) for p in pats], fold(data)
    first, ids, counts = [0], [], []
    for k in range(len(offsets) - 1):
        pos, found = am.brute_all(pats, np.frombuffer(data[offsets[k]:offsets[k + 1]], dtype=np.uint8))
        if longest and pos.size:                                # the list is longest first within a position
            lead = np.ones(pos.size, dtype=bool)
            lead[1:] = pos[1:] != pos[:-1]
            found = found[lead]
        u, c = np.unique(found, return_counts=True)
        ids.extend(int(i) for i in u)
        counts.extend(int(x) for x in c)
        first.append(len(ids))
    return np.array(first, dtype=np.uint64), np.array(ids, dtype=np.int32), np.array(counts, dtype=np.uint32)


def segcounts_from_result(seg_result, offsets, prefix_table, longest=False):
    """seg_result: the per-segment longest vector over the whole buffer; prefix_table: (prefixPattern[F + 1], chainLen[F + 1]) by id"""
    prefix = np.asarray(prefix_table[0], dtype=np.int64)
    r = np.asarray(seg_result)
    offsets = np.asarray(offsets, dtype=np.int64)
    segs = offsets.size - 1
    at = np.flatnonzero(r > 0)
    seg = np.searchsorted(offsets, at, side="right") - 1        # the last segment that starts at or in front of the position
    seg = np.clip(seg, 0, segs - 1)
    cur = r[at].astype(np.int64)
    keys = []
    while cur.size:
        keys.append(seg * prefix.size + cur)
        if longest:
            break
        cur = prefix[cur]
        alive = cur > 0
        cur, seg = cur[alive], seg[alive]
    u, c = np.unique(np.concatenate(keys) if keys else np.zeros(0, dtype=np.int64), return_counts=True)
    first = np.zeros(segs + 1, dtype=np.uint64)
    first[1:] = np.cumsum(np.bincount(u // prefix.size, minlength=segs))
    return first, (u % prefix.size).astype(np.int32), c.astype(np.uint32)


def batch_result(result, offsets, pats, prefix):
    """the per-segment longest vector from the longest vector of the whole buffer (offsets ascending, first 0, last the size)"""
    lens = np.array([0] + [len(p) for p in pats], dtype=np.int64)
    prefix = np.asarray(prefix, dtype=np.int64)
    r = np.asarray(result).astype(np.int64)
    offsets = np.asarray(offsets, dtype=np.int64)
    at = np.flatnonzero(r > 0)
    end = offsets[np.searchsorted(offsets, at, side="right")]   # the end of the segment the position lies in
    cur = r[at]
    while True:
        over = (cur > 0) & (at + lens[cur] > end)
        if not over.any():
            break
        cur[over] = prefix[cur[over]]
    out = np.zeros(r.size, dtype=np.int32)
    out[at] = cur
    return out


def brute_seg_result(pats, data, offsets, nocase=False):
    """the per-segment longest vector by brute force: tests/spans_ref.brute_result on each segment's bytes alone"""
    from tests.spans_ref import brute_result
    data = bytes(data)
    parts = [brute_result(pats, data[int(offsets[k]):int(offsets[k + 1])], nocase) for k in range(len(offsets) - 1)]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)


def same(got, want, what):
    """got / want: (segFirst, ids, counts)"""
    for g, w, name in zip(got, want, ("segFirst", "ids", "counts")):
        g, w = np.asarray(g).astype(np.int64), np.asarray(w).astype(np.int64)
        assert g.shape == w.shape, f"{what}: {name}: {g.size} entries, want {w.size}"
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            raise AssertionError(f"{what}: {name}: {bad.size} mismatches; first at {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}")


def pairs_of(lst, k):
    """[(id, count), ...] of segment k of a list"""
    first, ids, counts = lst
    lo, hi = int(first[k]), int(first[k + 1])
    return list(zip(ids[lo:hi].tolist(), counts[lo:hi].tolist()))


def segmentations(n):
    """(name, offsets) of the cuts every case is run under: every byte a segment, one segment, empty segments at the front, middle and end"""
    return [("every-byte", list(range(n + 1))), ("one-segment", [0, n]), ("empty-front-middle-end", [0, 0, n // 2, n // 2, n, n])]


EXTRA = [
    ("nested-a-cut-at-10", NESTED, b"a" * 20, [0, 10, 20]),
    ("needle-across-a-cut", [b"needle", b"nee", b"dle"], b"a needle", [0, 5, 8]),
    ("prefix-fits-where-the-longest-does-not", [b"ab", b"abcd", b"cd"], b"abcdabcd", [0, 3, 6, 8]),
    ("nocase-cut", [b"Error", b"ERR", b"or"], b"eRRoR ErrOR", [0, 4, 11]),
]
# (name, patterns, input, offsets): the cases of the count calls under every segmentation, then cases of their own
CASES = [(f"{name}/{cut}", pats, data, offsets) for name, pats, data in count_ref.CASES for cut, offsets in segmentations(len(data))] + EXTRA


def is_nocase(name):
    return name.startswith("nocase")


def fixed_set(count, chain=False):
    """`count` distinct patterns of seven bytes, pattern id i = b"p%05x;" % i: no pattern is a prefix of another (maxChain 1).  chain: id 1 is
    b"p" instead, a proper prefix of every other pattern (maxChain 2)"""
    pats = [b"p%05x;" % i for i in range(1, count + 1)]
    if chain:
        pats[0] = b"p"
    return pats


def test_the_two_segment_references_agree_on_every_case():
    for name, pats, data, offsets in CASES:
        nocase = is_nocase(name)
        folded = [fold(p) for p in pats] if nocase else pats
        prefix, chain, _ = am.prefix_table(folded)
        seg_result = brute_seg_result(pats, data, offsets, nocase)
        whole = brute_seg_result(pats, data, [0, len(data)], nocase)
        assert np.array_equal(batch_result(whole, offsets, folded, prefix), seg_result), name
        for longest in (False, True):
            a = segcounts_py(pats, data, offsets, nocase, longest)
            same(segcounts_from_result(seg_result, offsets, (prefix, chain), longest), a, f"{name}/longest {longest}")
            assert np.all(a[2] > 0) and int(a[0][-1]) == a[1].size
            # the rows summed are the counts of each segment alone
            for k in range(len(offsets) - 1):
                want = count_ref.counts_py(pats, data[offsets[k]:offsets[k + 1]], nocase, longest)
                got = np.zeros(len(pats) + 1, dtype=np.uint64)
                for i, c in pairs_of(a, k):
                    got[i] = c
                count_ref.same(got, want, f"{name}/segment {k}")
    nested = segcounts_py(NESTED, b"a" * 20, [0, 10, 20])
    assert pairs_of(nested, 0) == pairs_of(nested, 1) == [(k, 11 - k) for k in range(1, 9)]
    assert pairs_of(segcounts_py(NESTED, b"a" * 20, [0, 10, 20], longest=True), 1) == [(k, 1) for k in range(1, 8)] + [(8, 3)]
    cut = segcounts_py([b"needle", b"nee", b"dle"], b"a needle", [0, 5, 8])
    assert pairs_of(cut, 0) == [(2, 1)] and pairs_of(cut, 1) == [(3, 1)], "needle across the cut counts nowhere, nee in front of it does"
    assert pairs_of(segcounts_py([b"needle", b"nee", b"dle"], b"a needle", [0, 8]), 0) == [(1, 1), (2, 1), (3, 1)]
    fits = segcounts_py([b"ab", b"abcd", b"cd"], b"abcdabcd", [0, 3, 6, 8])
    assert [pairs_of(fits, k) for k in range(3)] == [[(1, 1)], [(1, 1)], [(3, 1)]]
    dup = segcounts_py([b"ab", b"cd", b"ab"], b"ab.cd.abcd", [0, 3, 10])
    assert pairs_of(dup, 0) == [(3, 1)] and pairs_of(dup, 1) == [(2, 2), (3, 1)], "duplicate lines count under the highest id"
    assert segcounts_py([b"ab"], b"", [0, 0])[0].tolist() == [0, 0]
