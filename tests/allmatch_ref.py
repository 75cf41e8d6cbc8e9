"""Reference all-match lists for tests/test_match_all_host.py and test_match_all_gpu.py, computed without the library's trie.

The all-match list (include/pfac_ext.h) is every (position, pattern id) pair such that the pattern occurs at the position, in
ascending position, longest pattern first within a position.  Duplicate lines are one pattern, reported under the highest ID.
  brute_all        every position, every distinct pattern length, a dict lookup (inputs of a few KiB)
  expand_longest   the oracle's longest result per position, each match followed by the shorter patterns that are prefixes of it
"""
import numpy as np


def pattern_ids(pats):
    """{pattern bytes: reported id} -- file order, the highest id of duplicate lines."""
    d = {}
    for i, p in enumerate(pats, 1):
        d[bytes(p)] = i
    return d


def prefix_table(pats):
    """(prefixPattern[F + 1], chainLen[F + 1], maxMatchesPerPosition) as PFACX_TABLE_PREFIX_PATTERN / PFACX_getInfo define them."""
    d = pattern_ids(pats)
    f = len(pats)
    prefix = np.zeros(f + 1, dtype=np.int32)
    chain = np.zeros(f + 1, dtype=np.int64)
    reported = sorted(d.values(), key=lambda i: len(pats[i - 1]))       # shorter first: a prefix's chain is known before it is needed
    for i in reported:
        p = bytes(pats[i - 1])
        for ln in range(len(p) - 1, 0, -1):
            q = d.get(p[:ln])
            if q is not None:
                prefix[i] = q
                break
        chain[i] = 1 + (chain[prefix[i]] if prefix[i] else 0)
    most = int(chain.max()) if f else 1
    return prefix, chain, max(1, most)


def brute_all(pats, data):
    """(pos, ids) int32 arrays of the all-match list by brute force."""
    d = pattern_ids(pats)
    lengths = sorted({len(p) for p in d}, reverse=True)
    raw = bytes(np.ascontiguousarray(data, dtype=np.uint8))
    n = len(raw)
    pos, ids = [], []
    for p in range(n):
        for ln in lengths:
            if p + ln <= n:
                i = d.get(raw[p:p + ln])
                if i is not None:
                    pos.append(p)
                    ids.append(i)
    return np.array(pos, dtype=np.int32), np.array(ids, dtype=np.int32)


NESTED_TOKEN_PATTERNS = [b"a", b"ab", b"abc"]       # ids 1, 2, 3: the chain of "abc" is 3, 2, 1


def nested_tokens(count):
    """`count` tokens "abc", "ab", "a", cycling in this order, each followed by the filler byte "x": one longest pair per token (no other
    byte starts a pattern), chains of 3, 2 and 1 alternating.  -> (data, pos, ids, start, pair_first): the input, the all-match list of
    NESTED_TOKEN_PATTERNS over it by construction, the byte each token starts at, and the list offset of each longest pair's first
    entry (count + 1 entries, the last one the length of the list)."""
    k = np.arange(count, dtype=np.int64)
    kind = k % 3
    toklen, chain = 4 - kind, 3 - kind
    ends = np.cumsum(toklen)
    start = ends - toklen
    pair_first = np.concatenate([[0], np.cumsum(chain)]).astype(np.int64)
    data = np.frombuffer(b"abcxabxax" * (count // 3 + 1), dtype=np.uint8)[:int(ends[-1]) if count else 0].copy()
    within = np.arange(pair_first[-1], dtype=np.int64) - np.repeat(pair_first[:-1], chain)
    pos = np.repeat(start, chain).astype(np.int32)
    ids = (np.repeat(chain, chain) - within).astype(np.int32)
    return data, pos, ids, start, pair_first


def expand_longest(pats, longest):
    """(pos, ids) of the all-match list from the longest-match result vector (oracle): at a position whose longest pattern is L,
    every shorter pattern that is a prefix of L's bytes also occurs there."""
    d = pattern_ids(pats)
    lengths = sorted({len(p) for p in d}, reverse=True)
    longest = np.asarray(longest)
    where = np.nonzero(longest > 0)[0]
    cache = {}
    pos, ids = [], []
    for p in where:
        top = int(longest[p])
        chain = cache.get(top)
        if chain is None:
            b = bytes(pats[top - 1])
            chain = [top] + [d[b[:ln]] for ln in lengths if ln < len(b) and b[:ln] in d]
            cache[top] = chain
        pos.extend([int(p)] * len(chain))
        ids.extend(chain)
    return np.array(pos, dtype=np.int32), np.array(ids, dtype=np.int32)
