"""Reference for the groups calls (PFACX_groups*) that shares no code with the library: the brute-force all-match list of each segment ALONE
(tests/allmatch_ref.py: brute_all), duplicate lines resolved to the highest id with ORed masks, then the filter of the definition.

groups_ref      (pos, ids, segFirst, segGroups) of a batch; all_matches=False keeps the first enabled pair of each position
longest_filter  the tempting shortcut -- the LONGEST pairs, those of a pattern that is not enabled dropped -- which loses an enabled proper prefix
CASES, WANT     the case table shared by the host test, the GPU test and tools/groups_host_san.cpp (which holds a copy)
Masks are Python ints or uint64.  Test infrastructure only."""

import numpy as np

from tests import allmatch_ref as am
from tests.spans_ref import fold

ALL_BITS = (1 << 64) - 1


def resolve_masks(pats, masks):
    """M[id] by REPORTED id: the OR over every line that names the pattern; 0 for the ids never reported (and entry 0)"""
    d = am.pattern_ids(pats)
    m = [0] * (len(pats) + 1)
    for i, p in enumerate(pats, 1):
        m[d[bytes(p)]] |= int(masks[i])
    return m


def segment_lists(pats, data, offsets=None, nocase=False):
    """[(pos, ids)] -- the all-match list of each segment alone, positions relative to the buffer -- and the folded patterns"""
    folded = [fold(p) for p in pats] if nocase else [bytes(p) for p in pats]
    raw = bytes(np.ascontiguousarray(data, dtype=np.uint8)) if not isinstance(data, (bytes, bytearray)) else bytes(data)
    hay = fold(raw) if nocase else raw
    off = [0, len(hay)] if offsets is None else [int(o) for o in offsets]
    out = []
    for k in range(len(off) - 1):
        pos, ids = am.brute_all(folded, np.frombuffer(hay[off[k]:off[k + 1]], dtype=np.uint8))
        out.append((pos.astype(np.int64) + off[k], ids.astype(np.int64)))
    return out, folded


def filter_lists(lists, m, seg_masks=None, all_matches=False):
    """the definition over the segments' all-match lists and the resolved masks m"""
    pos_out, ids_out, first, groups = [], [], [0], []
    for k, (pos, ids) in enumerate(lists):
        sm = ALL_BITS if seg_masks is None else int(seg_masks[k])
        hit = 0
        last = None
        count = 0
        for p, i in zip(pos.tolist(), ids.tolist()):
            both = m[i] & sm
            if both == 0:
                continue
            hit |= both
            if all_matches or p != last:
                pos_out.append(p)
                ids_out.append(i)
                count += 1
            last = p
        first.append(first[-1] + count)
        groups.append(hit)
    return (np.array(pos_out, dtype=np.int32), np.array(ids_out, dtype=np.int32), np.array(first, dtype=np.uint64),
            np.array(groups, dtype=np.uint64))


def groups_ref(pats, masks, data, offsets=None, seg_masks=None, all_matches=False, nocase=False):
    lists, folded = segment_lists(pats, data, offsets, nocase)
    return filter_lists(lists, resolve_masks(folded, masks), seg_masks, all_matches)


def longest_filter(pats, masks, data, offsets=None, seg_masks=None, nocase=False):
    """(pos, ids) of the shortcut: the longest pair of each position, kept only where that pattern is enabled"""
    lists, folded = segment_lists(pats, data, offsets, nocase)
    m = resolve_masks(folded, masks)
    pos_out, ids_out = [], []
    for k, (pos, ids) in enumerate(lists):
        sm = ALL_BITS if seg_masks is None else int(seg_masks[k])
        last = None
        for p, i in zip(pos.tolist(), ids.tolist()):
            if p != last and m[i] & sm:
                pos_out.append(p)
                ids_out.append(i)
            last = p
    return np.array(pos_out, dtype=np.int32), np.array(ids_out, dtype=np.int32)


def bounds_of(seg_first_pairs, count):
    """the first pair of each segment as the pairs form reads a caller's array: clamped to [0, count], raised to the largest entry in front"""
    return np.maximum.accumulate(np.clip(np.asarray(seg_first_pairs, dtype=np.int64), 0, count))


def groups_from_pairs(pair_pos, pair_ids, seg_first_pairs, num_segments, prefix, m, seg_masks=None, all_matches=False):
    """The definition over a LONGEST pair list, numpy level by level (big inputs, and the contract of the pairs form): pair i lies in the segment
    whose bounds hold it (none: it gives nothing), an id outside [1, F] gives nothing, a position is copied.  prefix: prefixPattern by id; m: the
    resolved masks by id"""
    pair_pos, pair_ids = np.asarray(pair_pos, dtype=np.int64), np.asarray(pair_ids, dtype=np.int64)
    prefix, mm = np.asarray(prefix, dtype=np.int64), np.array([int(x) for x in m], dtype=np.uint64)
    count, f = pair_ids.size, mm.size - 1
    if seg_first_pairs is None:
        seg = np.zeros(count, dtype=np.int64)
    else:
        seg = np.searchsorted(bounds_of(seg_first_pairs, count), np.arange(count), side="right") - 1
    sm = np.full(num_segments, ALL_BITS, dtype=np.uint64) if seg_masks is None else np.array([int(x) for x in seg_masks], dtype=np.uint64)
    keep = (seg >= 0) & (seg < num_segments) & (pair_ids >= 1) & (pair_ids <= f)
    index, q, s = np.flatnonzero(keep), pair_ids[keep], seg[keep]
    found = np.zeros(index.size, dtype=bool)
    groups = np.zeros(num_segments, dtype=np.uint64)
    out_index, out_q, out_level, level = [], [], [], 0
    while index.size:
        both = mm[q] & sm[s]
        ok = both != 0
        np.bitwise_or.at(groups, s[ok], both[ok])
        emit = ok if all_matches else ok & ~found
        found = found | ok
        out_index.append(index[emit])
        out_q.append(q[emit])
        out_level.append(np.full(int(emit.sum()), level))
        q = prefix[q]
        go = q > 0
        index, q, s, found = index[go], q[go], s[go], found[go]
        level += 1
    if out_index:
        i, qq, lv = np.concatenate(out_index), np.concatenate(out_q), np.concatenate(out_level)
        order = np.lexsort((lv, i))
        i, qq = i[order], qq[order]
    else:
        i = qq = np.zeros(0, dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(np.bincount(seg[i], minlength=num_segments)[:num_segments])]).astype(np.uint64)
    return pair_pos[i].astype(np.int32), qq.astype(np.int32), first, groups


def clip_to_segments(result, offsets, prefix, lengths):
    """the longest-match vector of a whole buffer -> that of its segments one by one: in front of a border the longest pattern that still fits"""
    out = np.array(result, dtype=np.int32)
    longest = int(max(lengths))
    for c in [int(o) for o in offsets[1:-1]]:
        for p in range(max(0, c - longest + 1), c):
            q = int(out[p])
            while q and p + int(lengths[q]) > c:
                q = int(prefix[q])
            out[p] = q
    return out


def same(got, want, what):
    """exact equality of two (pos, ids, segFirst, segGroups) results; a None in `got` is not compared"""
    for name, g, w in zip(("pos", "ids", "segFirst", "segGroups"), got, want):
        if g is None:
            continue
        g, w = np.asarray(g).astype(np.uint64 if name.startswith("seg") else np.int64), np.asarray(w).astype(np.uint64 if name.startswith("seg") else np.int64)
        assert g.size == w.size, f"{what}: {name} has {g.size} entries, want {w.size}"
        bad = np.flatnonzero(g != w)
        if bad.size:
            k = int(bad[0])
            raise AssertionError(f"{what}: {name} differs in {bad.size} entries, first at {k}: got {int(g[k]):#x} want {int(w[k]):#x}")


NESTED = [b"a" * k for k in range(1, 9)]                       # a, aa, ..., a x 8
B31, B32, B63 = 1 << 31, 1 << 32, 1 << 63
# (name, patterns, masks by id (entry 0 unused), input, offsets or None, segment masks or None, caseless)
CASES = [
    ("foo-foobar-masks-1-2-3-0", [b"foo", b"foobar"], [0, 1, 2], b"foobar foo" * 4, [0, 10, 20, 30, 40], [1, 2, 3, 0], False),
    ("chain-of-three-middle-enabled", [b"ab", b"abc", b"abcd"], [0, 1, 2, 4], b"abcd abc ab", [0, 11], [2], False),
    ("duplicate-lines-bits-0-and-63", [b"ab", b"cd", b"ab"], [0, 1, 2, B63], b"ab cd ab", [0, 3, 6, 8], [1, B63, B63], False),
    ("a-pattern-with-mask-0", [b"x", b"xy"], [0, 0, 5], b"xy x", None, None, False),
    ("bit-31-against-bit-32", [b"p", b"q"], [0, B31, B32], b"pq pq", [0, 3, 5], [B32, B31], False),
    ("a-match-across-a-border", [b"abcd", b"ab"], [0, 1, 1], b"xabcdx", [0, 3, 6], [1, 1], False),
    ("empty-segments", [b"a"], [0, 1], b"aa", [0, 0, 1, 1, 1, 1, 2, 2], None, False),
    ("one-byte-segments", [b"a", b"b", b"ab"], [0, 1, 2, 4], b"abab", [0, 1, 2, 3, 4], [3, 3, 1, 2], False),
    ("nested-a-longer-than-the-input", NESTED, [0] + [1 << k for k in range(8)], b"a" * 12, [0, 12], None, False),
    ("nested-a-every-other-group", NESTED, [0] + [1 << k for k in range(8)], b"a" * 12, [0, 5, 12], [0xAA, 0x55], False),
    ("the-whole-buffer-is-one-segment", [b"foo", b"foobar"], [0, 1, 2], b"foobar foo", None, [1], False),
    ("caseless", [b"Foo", b"FOOBAR"], [0, 1, 2], b"fooBAR FOO", None, [1], True),
]
# what the definition gives, worked out by hand: name -> ((ids, positions, segFirst) with flags 0, with ALL, segGroups)
WANT = {
    "foo-foobar-masks-1-2-3-0": (([1, 1, 2, 2, 1], [0, 7, 10, 20, 27], [0, 2, 3, 5, 5]),
                                 ([1, 1, 2, 2, 1, 1], [0, 7, 10, 20, 20, 27], [0, 2, 3, 6, 6]), [1, 2, 3, 0]),
    "chain-of-three-middle-enabled": (([2, 2], [0, 5], [0, 2]),) * 2 + ([2],),
    "duplicate-lines-bits-0-and-63": (([3, 3], [0, 6], [0, 1, 1, 2]),) * 2 + ([1, 0, B63],),
    "a-pattern-with-mask-0": (([2], [0], [0, 1]),) * 2 + ([5],),
    "bit-31-against-bit-32": (([2, 1], [1, 3], [0, 1, 2]),) * 2 + ([B32, B31],),
    "a-match-across-a-border": (([2], [1], [0, 1, 1]),) * 2 + ([1, 0],),
    "empty-segments": (([1, 1], [0, 1], [0, 0, 1, 1, 1, 1, 2, 2]),) * 2 + ([0, 1, 0, 0, 0, 1, 0],),
    "one-byte-segments": (([1, 2, 1, 2], [0, 1, 2, 3], [0, 1, 2, 3, 4]),) * 2 + ([1, 2, 1, 2],),
    "the-whole-buffer-is-one-segment": (([1, 1], [0, 7], [0, 2]),) * 2 + ([1],),
    "caseless": (([1, 1], [0, 7], [0, 2]),) * 2 + ([1],),
}


def test_the_reference_agrees_with_the_lists_worked_out_by_hand():
    for name, pats, masks, data, offsets, seg_masks, nocase in CASES:
        for all_matches in (False, True):
            got = groups_ref(pats, masks, data, offsets, seg_masks, all_matches, nocase)
            assert got[2][-1] == got[0].size and got[2].size == (2 if offsets is None else len(offsets))
            if name in WANT:
                ids, pos, first = WANT[name][1 if all_matches else 0]
                same(got, (pos, ids, first, WANT[name][2]), f"{name}/all {all_matches}")
            # the level-by-level form over the longest pairs of the segments gives the same
            lists, folded = segment_lists(pats, data, offsets, nocase)
            longest = [(p[np.r_[True, p[1:] != p[:-1]]], i[np.r_[True, p[1:] != p[:-1]]]) if p.size else (p, i) for p, i in lists]
            bounds = np.concatenate([[0], np.cumsum([p.size for p, _ in longest])])
            by_pairs = groups_from_pairs(np.concatenate([p for p, _ in longest]), np.concatenate([i for _, i in longest]), bounds, len(lists),
                                         am.prefix_table(folded)[0], resolve_masks(folded, masks), seg_masks, all_matches)
            same(by_pairs, got, f"{name}/all {all_matches}: from the longest pairs")
    # ALL is longer than the input: 12 bytes of a under a, aa, ..., a x 8
    assert groups_ref(*CASES[8][1:4], CASES[8][4], None, True)[0].size == sum(min(8, 12 - p) for p in range(12)) > 12
    # the shortcut loses foo where foobar, of another group, is the longest
    name, pats, masks, data, offsets, seg_masks, nocase = CASES[0]
    assert longest_filter(pats, masks, data, offsets, seg_masks)[0].tolist() == [7, 10, 20, 27]
