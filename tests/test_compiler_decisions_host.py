"""Every decision of the pattern compiler on both sides of its threshold, without a GPU: the sets of tests/compiler_sets.py (each asserts which
side it is on) through the numpy models of the prefilter (tests/filter_model.py) and of the chained table (tests/chain_model.py) against the
oracle, and the structures that the one-sided rule -- a miss proves the result is 0 -- depends on, rebuilt from the pattern list: skip tags and
tail entries exist only for hashes that exactly one ladder node carries, and a tail entry describes the last bytes of the one pattern below its
node.  (pattern_compiler.cpp: buildFilter; tables.cpp: buildChainedHashTable.)"""
import numpy as np
import pytest

from pfac_amd import api
from tests import compiler_sets as cs
from tests.chain_model import ChainWalker
from tests.filter_model import (SKIP_TAGS_MAX, TAIL_MAX_BYTES, TAIL_MIN_BYTES, ladder_hash, ladder_nodes, prefilter_model,
                                reduce_filter_model, skip_tag_paths, tail_entries, tail_hash)


@pytest.mark.parametrize("name", cs.NAMES)
def test_prefilter_of_the_set_has_no_false_negatives(name):
    """The set lies where its builder says (compiler_sets asserts it), and every position at which the oracle reports a pattern passes the
    prefilter as the veto kernels, the other full-result kernels and the compacted-output kernel evaluate it."""
    cs.get(name)
    h = cs.host_handle(name)
    whole, want_whole = cs.stream(name)
    cut = whole[:-2]                                    # the last pattern is cut off by the end of the input
    want_cut = cs.oracle_match(name, cut)
    assert not np.array_equal(want_cut, want_whole[:-2])
    for data, want in ((whole, want_whole), (cut, want_cut)):
        hit = want != 0
        assert hit.sum() > 500
        for veto in (True, False):
            level1, cand, walk = prefilter_model(h, data, veto=veto)
            for what, passed in (("level 1", level1), ("candidates", cand), ("walked", walk)):
                assert np.all(passed[hit]), (name, veto, what, int(np.flatnonzero(hit & ~passed)[0]))
        level1, walk = reduce_filter_model(h, data)
        assert np.all(level1[hit]) and np.all(walk[hit]), name


def _decision(info):
    return {"tags": info.filterSkipTags, "lds": info.filterTailEntries > 0, "global": info.filterTailGlobalEntries > 0, "last": info.filterLadderLast,
            "extend": info.ladderExtend, "thin": info.ladderThin > 1, "bits": info.filterLog2Bits, "ladderBits": info.filterLog2BitsLadder,
            "final3Bits": info.filterLog2BitsFinal3, "short": bool(info.filterHasShort)}


# the fields in which the two sets of a pair differ; every other field of _decision is the same for both ("ladderBits" follows the number of
# nodes and "bits" the number of 3-grams: left out where the sets differ in size)
@pytest.mark.parametrize("a,b,differ,free", [
    ("tags8", "tags9", (), ("bits",)),                              # 8 and 9 tagged-looking paths: eight tags either way
    ("tags1", "tag_ends", ("tags", "lds"), ()),
    ("tags1", "tag_branch", ("tags",), ()),
    ("rest5", "rest6", ("lds",), ()),
    ("rest255", "rest256", ("lds",), ()),
    ("lds5000", "glob8000", ("lds", "global"), ("ladderBits", "bits")),
    ("lds5000", "lds5000_short", ("lds", "global", "short"), ()),
    ("deep_kept", "deep_refused", ("last", "global"), ("ladderBits", "bits")),
    ("extend0", "thin2", ("thin",), ("ladderBits", "bits")),
    ("final3_8", "final3_9", ("final3Bits",), ()),
])
def test_the_two_sets_of_a_pair_differ_in_the_decision_the_pair_is_about(a, b, differ, free):
    da, db = _decision(cs.host_handle(a).info()), _decision(cs.host_handle(b).info())
    for field in da:
        if field in differ:
            assert da[field] != db[field], (a, b, field, da[field])
        elif field not in free:
            assert da[field] == db[field], (a, b, field, da[field], db[field])


@pytest.mark.parametrize("name", cs.NAMES)
def test_skip_tags_and_tail_entries_belong_to_exactly_one_ladder_node(name):
    """The ladder rebuilt from the pattern list with the set's thin threshold, extra level, depth and salt has the node counts the library
    reports.  Every skip tag is the hash of a depth-6 node with one path of G nodes down to depth 20 that no other node shares, and there are
    min(such paths, 8) of them.  Every tail entry, of either form, belongs to a hash that exactly one node carries: a thin stop with one pattern
    below it whose rest has 6 .. 255 bytes; the entry compares the LAST min(rest, 16) & ~3 bytes of that pattern, from the depth it says, and
    holds their hash; the device-memory form has no entry for a depth beyond 255 (the set glob_far)."""
    sset = cs.get(name)
    h = cs.host_handle(name)
    info = h.info()
    nodes = ladder_nodes(sset.patterns, info.ladderThin, info.ladderExtend, info.filterLadderLast, info.filterLadderSalt)
    assert sum(nd.stop for nd in nodes) == info.ladderStops and sum(not nd.stop for nd in nodes) == info.ladderGoOns
    by_hash = {}
    for nd in nodes:
        by_hash.setdefault(nd.hash, []).append(nd)

    tags = h.table(api.PFACX_TABLE_FILTER_SKIP).tolist()
    eligible = skip_tag_paths(nodes)
    assert len(tags) == info.filterSkipTags == min(len(eligible), SKIP_TAGS_MAX), (len(tags), len(eligible))
    assert len(set(tags)) == len(tags) and set(tags) <= set(eligible)
    if sset.tagged and info.filterSkipTags:                         # the stream's near misses of tagged prefixes do meet a tag
        data, _ = cs.stream(name)
        text = data.tobytes()
        met = [t for t in sset.tagged if ladder_hash(t[:6], info.filterLadderSalt) in tags and text.count(t[:6]) >= 18]
        assert met, name

    entries = tail_entries(h)
    assert len(entries) == info.filterTailEntries + info.filterTailGlobalEntries
    assert not (info.filterTailEntries and info.filterTailGlobalEntries), "a set has one form or the other"
    for tag, want, nbytes, start, mask in entries:
        assert len(by_hash.get(tag, ())) == 1, (name, hex(tag), len(by_hash.get(tag, ())))
        nd = by_hash[tag][0]
        assert nd.thin_stop and len(nd.below) == 1, (name, nd.prefix)
        p = nd.below[0]
        rest = len(p) - nd.depth
        assert TAIL_MIN_BYTES <= rest <= 255, (name, p, rest)
        assert 4 <= nbytes <= TAIL_MAX_BYTES and nbytes % 4 == 0 and nbytes == min(rest, TAIL_MAX_BYTES) & ~3, (name, p, nbytes)
        assert start == len(p) - nbytes and start >= nd.depth, (name, p, start, nbytes)
        assert tail_hash(tag, p[start:]) & mask == want, (name, p)
    # the device-memory form keeps `start` in eight bits: a pattern whose last 16 bytes begin at depth 256 has no entry, its neighbour at 255 has
    owners = {by_hash[tag][0].below[0] for tag, *_ in entries}
    for p in sset.extra.get("near", []):
        assert len(p) - TAIL_MAX_BYTES == 255 and p in owners, (name, len(p))
    for p in sset.extra.get("far", []):
        assert len(p) - TAIL_MAX_BYTES == 256 and p not in owners, (name, len(p))
    # nothing that could have an entry is refused for another reason than its table being full: the thin stops of a small set all have theirs
    if len(sset.patterns) <= 100 and info.filterTailEntries:
        could = [nd for nd in nodes if nd.thin_stop and len(nd.below) == 1 and len(by_hash[nd.hash]) == 1
                 and TAIL_MIN_BYTES <= len(nd.below[0]) - nd.depth <= 255]
        assert len(entries) >= len(could) - 4, (name, len(entries), len(could))      # (an entry that finds both its slots taken is left out)


def _walk(name, streams):
    walker = ChainWalker(cs.host_handle(name))
    for data in streams:
        want = cs.oracle_match(name, data)
        for long_jump in (False, True):
            walker.walk_all(data, want, long_jump, what=(name, long_jump))
    return walker


def _joined(pats, miss=True):
    """every pattern complete and (miss) with its last byte wrong, a filler byte between them; behind them as much filler as the longest pattern
    of any set has bytes (the walker leaves out the positions from which a walk could reach the end)"""
    parts = []
    for p in pats:
        parts += [p, b"0"] + ([p[:-1] + b"#", b"0"] if miss else [])
    return np.frombuffer(b"".join(parts) + b"0" * 720, dtype=np.uint8)


def test_chained_walk_meets_every_slot_shape_of_the_chains_set():
    """The Python walker over the chained table of the set built for it, with both jump tables, equals the oracle at every position of a 20 KB
    stream and of a stream of every pattern and its near miss; on the way it has met chains of every length 0 .. 23, long slots, a final state
    in mid-chain, the jump-table fallback of a pattern whose prefix lost its slot, and the buckets of the states with fan-out 9 and 130."""
    sset = cs.get("chains")
    extra = sset.extra
    data, _ = cs.stream("chains", 20 * 1024 + 77)
    walker = _walk("chains", [data, _joined(sset.patterns)])
    assert walker.chain_lengths >= set(range(24)), sorted(walker.chain_lengths)
    assert walker.long_slots > 0 and walker.mid_finals > 0 and walker.fell_back > 0
    assert walker.info.chainJumpLog2 == extra["J"]
    # the colliding pair: one slot, so at least one of the two prefixes is not in it -- and its pattern is found through the initial state's bucket
    a, b = extra["pair"]
    assert walker.jump_slot(int.from_bytes(a, "little")) == walker.jump_slot(int.from_bytes(b, "little"))
    slot = walker.slots[walker.jump_slot(int.from_bytes(a, "little"))]
    owner = bytes([int(slot[0]) & 0xFF]) + int(slot[2]).to_bytes(4, "little")[:3]
    lost = [p for p in sset.patterns if p[:4] in (a, b) and p[:4] != owner]
    assert lost and not (int(slot[0]) & (1 << 14))
    one = ChainWalker(cs.host_handle("chains"))
    stream = _joined(lost, miss=False)
    want = cs.oracle_match("chains", stream)
    assert np.count_nonzero(want) >= len(lost)
    _, fell_back = one.walk_all(stream, want)
    assert walker.info.maxPatternLen <= 720 and fell_back >= len(stream) - 720          # every walk of this stream, the lost patterns' among them
    # bucket sizes: a fan-out of 9 takes 16 slots, one of 130 takes 256 (tables.cpp: needBucket)
    for word, size in ((extra["fan9"], 16), (extra["fan130"], 256)):
        one = ChainWalker(cs.host_handle("chains"))
        stream = _joined([p for p in sset.patterns if p.startswith(word)])
        one.walk_all(stream, cs.oracle_match("chains", stream))
        assert size in one.bucket_sizes, (word, sorted(one.bucket_sizes))


@pytest.mark.parametrize("name", ["rest255", "tags9", "final3_9"])
def test_chained_walk_of_other_sets_equals_oracle(name):
    data, _ = cs.stream(name, 20 * 1024 + 77)
    walker = _walk(name, [data])
    if name == "rest255":
        assert walker.long_slots > 0 and 23 in walker.chain_lengths
