"""Pattern sets on both sides of every decision the pattern compiler takes (pattern_compiler.cpp: buildFilter; tables.cpp; the dense fast table
of pfac_api.cpp) and the streams that go with them (tests/test_compiler_decisions_host.py, test_compiler_decisions_gpu.py): test
infrastructure only, in the style of tests/scale_sets.py.  Every builder is a pure function of its name, cached for the process, and asserts
its own precondition from PFACX_getInfo of a host-only handle: a change of the compiler that moves a threshold turns the fixture red instead
of quietly testing one side twice.  Counts are asserted only where the code fixes them (min(groups, kSkipTagsMax) skip tags).

  tags1 tags7 tags8 tags9   g groups of a random 24-byte prefix + three random 10-byte tails: g skip tags, at most 8
  tag_ends tag_branch       one such group + a pattern that ends on the tagged path / that branches off it between depths 6 and 20: no tag
  rest4 .. rest256          50 random patterns of 6 + r bytes: the ladder stops at depth 6 and r bytes are the rest.  r < kTailMinBytes: no
                            tail entry; 6 .. 255: entries; 256 (more than the 255 bytes the compiler follows): none
  lds5000 glob8000          random 30-byte patterns: the tail table in LDS (entries that find both slots taken are dropped) / in device memory
  lds5000_short             lds5000 + `q` and `zz`: the 2-byte bitmap takes the LDS the table had
  glob_far                  glob8000 + patterns of 271 / 272 bytes that are alone from depth 22 on: the depth of the bytes a device-memory entry
                            compares fits its eight bits (255) / does not (256: no entry)
  deep_kept deep_refused    400 / 600 groups of 64 patterns that share 24 bytes and go on over a two-letter alphabet: the ladder behind depth 20
                            fits the bitmap (filterLadderLast 60) / does not (20); more than 8 tagged-looking paths
  extend0 thin2             34 000 / 50 000 random patterns of 12..24 bytes over 16 letters: no extra level behind thin nodes / ladderThin > 1
  tiny                      10 random 30-byte patterns: every bitmap at its smallest size
  final3_8 final3_9         8 / 9 three-byte patterns: filterLog2BitsFinal3 at 10 / above
  short_shrink              20 000 of the 16-letter patterns + `q`: the 2-byte bitmap makes the budget loop shrink the ladder's cap
  salted                    1000 random 30-byte patterns for which the compiler picks a non-zero ladder salt
  shared_hash               ten such patterns + two whose ladder nodes at depth 6 have one hash: neither may have a tail entry
  chains                    the `longset` recipe of tests/test_kernel_variants.py without its one-byte pattern + prefixes of patterns at depths 7, 8, 23, 24, two patterns whose
                            first four bytes collide in the jump table, a state with fan-out 9 and one with fan-out 130
  fast_under fast_over fast_chains   6000 / 7950 three-byte patterns over 20 letters (under / over 8192 states, none inside a chain) and 330 patterns of 20 bytes
                            over two letters (most states inside chains): the dense fast table exists for the first only
"""
import atexit
import functools
import os
import shutil
import tempfile

import numpy as np

from pfac_amd import api
from pfac_amd import workloads as wl
from tests.chain_model import jump_hash
from tests.filter_model import LADDER_LAST, SKIP_TAGS_MAX, TAIL_MAX_BYTES, TAIL_MIN_BYTES

CHUNK = 2048                                 # input bytes of a chunk of the filter kernel
STREAM_BYTES = 2048 * 150 + 333              # what tests/test_kernel_variants.py: test_long_slots_in_every_kernel uses with the filter kernel forced
DENSE_BYTES = (33 << 20) + 1237              # above the 32 MiB below which PFACX_KERNEL_AUTO takes the tiled kernel alone, and odd
TAIL_MAX_REST, TAIL_GLOBAL_MAX_FROM, LADDER_DEEP_LAST = 255, 255, 60      # the longest rest the compiler follows; the deepest `from` of a device-memory entry; kLadderDeepLast
DENSE_FAST_MAX_STATES = 8192                 # pfac_context.h: kDenseFastMaxStates
LOW = np.arange(97, 123, dtype=np.uint8)
LOW16 = np.frombuffer(b"abcdefghijklmnop", dtype=np.uint8)



@functools.lru_cache(maxsize=None)
def _dir():
    """where the pattern files go: made when the first set is built (importing this module for longset_patterns alone makes nothing)"""
    path = tempfile.mkdtemp(prefix="pfac_compiler_")
    atexit.register(shutil.rmtree, path, ignore_errors=True)
    return path


class CompilerSet:
    """patterns: in file order (ids 1..); tagged: the 24-byte prefixes that look like skip-tag paths; veto: the form of the tail table the set
    was built to get (scanStats()["veto"] behind a PFACX_WALKER_VETO launch: 0 none, 1 LDS, 2 device memory); spares_walks: near misses of
    the set's patterns are what the veto launch must walk less of than the window launch"""

    def __init__(self, name, patterns, tagged=(), veto=1, spares_walks=False, extra=None):
        self.name, self.patterns, self.tagged, self.veto, self.spares_walks = name, patterns, tuple(tagged), veto, spares_walks
        self.extra = extra or {}
        self.pattern_file = wl.write_pattern_file(os.path.join(_dir(), name + ".pat"), patterns)

    @property
    def small(self):
        return len(self.patterns) <= 5000


def _words(rng, count, length, alpha=LOW):
    out = set()
    while len(out) < count:
        ln = length if isinstance(length, int) else int(rng.integers(length[0], length[1] + 1))
        out.add(alpha[rng.integers(0, alpha.size, ln)].tobytes())
    return sorted(out)


def _info(patterns, table=None):
    """PFACX_getInfo of a host-only handle with the patterns read (table: built first -- the chained table exists on request only)"""
    h = api.PFAC.createHostOnly()
    try:
        h.setPerfMode(api.PFAC_SPACE_DRIVEN)
        h.readPatternFromMemory(b"".join(p + b"\n" for p in patterns))
        if table is not None:
            h.table(table)
        return h.info()
    finally:
        h.destroy()


# --------------------------------------------------------------------------------------------------------------------------- skip tags

def _tag_groups(groups, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    prefixes = [LOW[rng.integers(0, 26, 24)].tobytes() for _ in range(groups)]
    pats = [p + LOW[rng.integers(0, 26, 10)].tobytes() for p in prefixes for _ in range(3)]
    return prefixes, pats, rng


def _tags(name):
    groups = {"tags1": 1, "tags7": 7, "tags8": 8, "tags9": 9, "tag_ends": 1, "tag_branch": 1}[name]
    prefixes, pats, rng = _tag_groups(groups, 600 + groups)
    want = min(groups, SKIP_TAGS_MAX)
    if name == "tag_ends":
        pats, want = pats + [prefixes[0][:10]], 0
    if name == "tag_branch":
        pats, want = pats + [prefixes[0][:13] + b"#" + LOW[rng.integers(0, 26, 20)].tobytes()], 0
    info = _info(pats)
    assert info.filterSkipTags == want, (name, info.filterSkipTags)
    # (the pattern that ends at depth 10 is a stop with four patterns below it: the ladder of tag_ends never gets to a node that knows a rest)
    assert (info.filterTailEntries > 0) == (name != "tag_ends") and info.filterTailGlobalEntries == 0
    return CompilerSet(name, pats, tagged=prefixes, veto=int(name != "tag_ends"), spares_walks=name != "tag_ends")


# -------------------------------------------------------------------------------------------------------------------------- tail table

def _rest(name):
    r = int(name[4:])
    pats = _words(np.random.Generator(np.random.PCG64(700 + r)), 50, 6 + r)
    assert len({p[:4] for p in pats}) == 50            # every pattern is alone from depth 4 on: one more level, then the stop at depth 6
    info = _info(pats)
    has = TAIL_MIN_BYTES <= r <= TAIL_MAX_REST
    assert (info.filterTailEntries > 0) == has and info.filterTailGlobalEntries == 0, (name, info.filterTailEntries, info.filterTailGlobalEntries)
    return CompilerSet(name, pats, veto=1 if has else 0, spares_walks=has)


def _lds(name):
    count = 8000 if name == "glob8000" else 5000
    pats = _words(np.random.Generator(np.random.PCG64(9)), count, 30)
    if name == "lds5000_short":
        pats = pats + [b"q", b"zz"]
    info = _info(pats)
    if name == "lds5000":
        assert 0 < info.filterTailEntries < count and info.filterTailGlobalEntries == 0, (info.filterTailEntries, info.filterTailGlobalEntries)
        assert info.filterLog2Bits == 18           # the level-1 bitmap at its largest
    else:
        assert info.filterTailEntries == 0 and info.filterTailGlobalEntries > 0, (info.filterTailEntries, info.filterTailGlobalEntries)
    assert info.filterHasShort == (name == "lds5000_short")
    return CompilerSet(name, pats, veto=1 if name == "lds5000" else 2, spares_walks=True)


def _glob_far(name):
    """glob8000 + two groups of four patterns that share 20 bytes and branch there: each is alone from depth 22 on and stops, one level on, at
    depth 24 with a rest of 247 / 248 bytes.  A device-memory entry keeps the depth of the first compared byte -- the pattern's length less 16 --
    in eight bits: the patterns of 271 bytes (depth 255) have an entry, those of 272 (256) must have none."""
    rng = np.random.Generator(np.random.PCG64(10))
    groups = {}
    for which, length in (("near", TAIL_GLOBAL_MAX_FROM + TAIL_MAX_BYTES), ("far", TAIL_GLOBAL_MAX_FROM + TAIL_MAX_BYTES + 1)):
        stem = LOW[rng.integers(0, 26, 20)].tobytes()
        groups[which] = [stem + bytes([97 + 3 * k]) + LOW[rng.integers(0, 26, length - 21)].tobytes() for k in range(4)]
        assert all(len(p) == length and length - 24 <= TAIL_MAX_REST for p in groups[which])
    pats = _words(np.random.Generator(np.random.PCG64(9)), 8000, 30) + groups["near"] + groups["far"]
    info = _info(pats)
    assert info.filterTailEntries == 0 and info.filterTailGlobalEntries > 0 and info.filterLadderLast == LADDER_DEEP_LAST
    return CompilerSet(name, pats, veto=2, spares_walks=True, extra=groups)


# ------------------------------------------------------------------------------------------------------------------------ ladder shape

def _family(groups):
    rng = np.random.Generator(np.random.PCG64(5))
    ab = np.frombuffer(b"ab", dtype=np.uint8)
    prefixes, pats = [], set()
    for _ in range(groups):
        pre = LOW[rng.integers(0, 26, 24)].tobytes()
        prefixes.append(pre)
        for _ in range(64):
            pats.add(pre + ab[rng.integers(0, 2, 36)].tobytes())
    return prefixes, sorted(pats)


def _deep(name):
    prefixes, pats = _family(400 if name == "deep_kept" else 600)
    info = _info(pats)
    assert info.ladderThin == 1 and info.ladderExtend == 1 and info.filterSkipTags == SKIP_TAGS_MAX
    if name == "deep_kept":
        assert info.filterLadderLast == LADDER_DEEP_LAST and info.filterTailGlobalEntries > 0 and info.filterTailEntries == 0
        assert info.filterLog2BitsLadder == 19     # the ladder bitmap at its cap (no 2-byte bitmap in the LDS)
    else:                                           # nothing behind depth 20: the stops there have many patterns below them, none knows a rest
        assert info.filterLadderLast == LADDER_LAST and info.filterTailGlobalEntries == 0 and info.filterTailEntries == 0
    return CompilerSet(name, pats, tagged=prefixes, veto=2 if name == "deep_kept" else 0, spares_walks=name == "deep_kept")


@functools.lru_cache(maxsize=None)
def _letters16(count):
    """the recipe of tests/test_host_api.py: test_prefix_ladder_of_a_very_large_pattern_set, shrunk: patterns of 12..24 bytes over 16 letters"""
    rng = np.random.default_rng(11)
    out = set()
    while len(out) < count:
        out.add(LOW16[rng.integers(0, 16, size=int(rng.integers(12, 25)))].tobytes())
    return sorted(out)


def _thin(name):
    pats = _letters16(34000 if name == "extend0" else 50000)
    info = _info(pats)
    assert info.filterLadderLast == LADDER_LAST and info.ladderExtend == 0, (info.filterLadderLast, info.ladderExtend)
    assert (info.ladderThin == 1) if name == "extend0" else (1 < info.ladderThin < (1 << 30)), info.ladderThin
    assert info.filterTailGlobalEntries > 0 and info.filterTailEntries == 0
    # spares_walks stays off for these sets and for short_shrink: the stream's candidates are mostly those of 34 000+ patterns' prefixes, and the
    # VETO = 2 kernel asks the table only for a batch with at least kTailAskMin stopped candidates (scan_filter.hip).  The model, which asks
    # for every stop, spares 1 - 4 % of the walks; how many batches reach the gate depends on how the chunks fall to the waves (a handful on
    # extend0 and short_shrink, none on thin2): the veto launch is asserted to walk no more than the window launch, not less.
    return CompilerSet(name, pats, veto=2)


# --------------------------------------------------------------------------------------------------------------------- bitmap sizes, salt

def _tiny(name):
    pats = _words(np.random.Generator(np.random.PCG64(13)), 10, 30)
    info = _info(pats)
    assert (info.filterLog2Bits, info.filterLog2BitsLadder, info.filterLog2BitsFinal3) == (13, 13, 10)
    assert info.filterTailEntries > 0
    return CompilerSet(name, pats, veto=1, spares_walks=True)


def _final3(name):
    count = int(name[7:])
    rng = np.random.Generator(np.random.PCG64(33))
    pats = _words(rng, count, 3) + _words(rng, 6, 12)
    info = _info(pats)
    assert (info.filterLog2BitsFinal3 == 10) if count == 8 else (info.filterLog2BitsFinal3 > 10), info.filterLog2BitsFinal3
    return CompilerSet(name, pats, veto=1 if info.filterTailEntries else 0)


def _short_shrink(name):
    base = _letters16(20000)
    plain, short = _info(base), _info(base + [b"q"])
    assert plain.filterLog2BitsLadder == 19 and not plain.filterHasShort
    assert short.filterHasShort and short.filterLog2BitsLadder == 18, short.filterLog2BitsLadder      # 32 + 64 + 1 + 8 KiB is over the budget: the ladder gives way
    assert short.filterLog2Bits == 18 and short.filterTailGlobalEntries > 0
    return CompilerSet(name, base + [b"q"], veto=2)


def _salted(name):
    pats = _words(np.random.Generator(np.random.PCG64(1)), 1000, 30)      # seed 1: the first seed tried whose set gets a salt (seed 2 does too)
    info = _info(pats)
    assert info.filterLadderSalt != 0 and info.filterTailEntries > 0
    return CompilerSet(name, pats, veto=1, spares_walks=True)


def _shared_hash(name):
    """two patterns whose depth-6 ladder nodes have ONE hash whatever the salt (it is XORed into both): first four bytes whose depth-4 hashes
    agree in their upper 16 bits, then two bytes that make up for the rest"""
    from tests.filter_model import LAD_MUL0, ladder_hash
    by_top, pair = {}, None
    for a in range(26 ** 4):
        w = bytes([97 + a // 17576, 97 + a // 676 % 26, 97 + a // 26 % 26, 97 + a % 26])
        h = (int.from_bytes(w, "little") * LAD_MUL0) & 0xFFFFFFFF
        for other, h2 in by_top.get(h >> 16, ()):
            d = h ^ h2
            lo, hi = d & 0xFF, d >> 8
            x = next((c for c in range(97, 123) if 97 <= c ^ lo <= 122), None)         # two letters that differ by lo, two that differ by hi
            y = next((c for c in range(97, 123) if 97 <= c ^ hi <= 122), None)
            if pair is None and x is not None and y is not None:
                pair = (w + bytes([x, y]), other + bytes([x ^ lo, y ^ hi]))
        if pair:
            break
        by_top.setdefault(h >> 16, []).append((w, h))
    rng = np.random.Generator(np.random.PCG64(77))
    twins = [q + LOW[rng.integers(0, 26, 12)].tobytes() for q in pair]
    assert ladder_hash(pair[0], 0) == ladder_hash(pair[1], 0) and ladder_hash(pair[0], 12345) == ladder_hash(pair[1], 12345)
    pats = sorted(_words(rng, 10, 30) + twins)
    info = _info(pats)
    assert 0 < info.filterTailEntries <= 10 and info.filterTailGlobalEntries == 0, info.filterTailEntries      # none for the twins
    return CompilerSet(name, pats, veto=1, spares_walks=True, extra={"twins": twins})


# ------------------------------------------------------------------------------------------------------------------------ chained table

def longset_patterns():
    """Patterns whose tries are long single-successor runs cut in every way a slot can be cut: lengths 9 .. 64 in steps of one
    (chains of every length 0 .. 23 behind a branch), one 300-byte and one 700-byte pattern (several long slots in a row; deeper
    than the 128 bytes staged behind a chunk), patterns that are prefixes of patterns at depths 8, 9, 24, 25 (a final state with
    successors ends a slot early), a shared 24-byte prefix with 40 tails (BASELINE config 5's shape) and a few short ones.
    -> (sorted patterns, prefix, tails, p300, p700)"""
    rng = np.random.Generator(np.random.PCG64(55))
    low = np.arange(97, 123, dtype=np.uint8)
    def word(n):
        return low[rng.integers(0, low.size, n)].tobytes()
    pats = set()
    for n in range(9, 65):
        pats.add(word(n))
    p300, p700 = word(300), word(700)
    pats.update([p300, p700, p300[:8], p300[:9], p300[:24], p300[:25], p700[:100], p700[:101] + b"X"])
    prefix = word(24)
    tails = [word(int(rng.integers(8, 41))) for _ in range(40)]
    pats.update(prefix + t for t in tails)
    pats.update([b"zq", b"q", b"zqzqzq"])
    pats = sorted(pats)
    return pats, prefix, tails, p300, p700


def _chains(name):
    pats, prefix, tails, p300, p700 = longset_patterns()
    rng = np.random.Generator(np.random.PCG64(56))
    def word(n):
        return LOW[rng.integers(0, 26, n)].tobytes()
    # (without the one-byte pattern `q`: its 65536 3-grams fill the level-1 bitmap of so small a set, every chunk then counts as pattern-dense and goes
    # to the tiled kernel -- no walker of the filter kernel would ever run)
    pats = [p for p in pats if p != b"q"] + [p700[:7], p700[:8], p700[:23], p700[:24]]
    # behind a branch: a chain of every length 0 .. 23 that ends in a leaf, and one of every length that ends in a branch again
    stem = word(6)
    for k in range(24):
        pats.append(stem + bytes([65 + k]) + word(k))                      # 'A' + k: the edge byte, then k chain bytes
        fork = stem + bytes([33 + k]) + word(k)                             # '!' + k
        pats += [fork + b"x" + word(3), fork + b"y" + word(3)]
    fan9, fan130 = word(5), word(5)
    pats += [fan9 + bytes([48 + k]) + word(4) for k in range(9)]
    pats += [fan130 + bytes([126 + k]) + word(4) for k in range(130)]
    # two 4-byte prefixes in one slot of the jump table (two more prefixes in a table of eight slots per prefix do not change its size: checked below)
    J = _info(pats + [word(16), word(16)], api.PFACX_TABLE_CHAIN).chainJumpLog2
    seen, pair = {}, None
    taken = {p[:4] for p in pats if len(p) >= 4}
    while pair is None:
        w = word(4)
        if w in taken:
            continue
        slot = jump_hash(int.from_bytes(w, "little"), J)
        if slot in seen and seen[slot] != w:
            pair = (seen[slot], w)
        seen[slot] = w
    pats += [pair[0] + word(12), pair[1] + word(12)]
    assert len(set(pats)) == len(pats)
    assert _info(pats, api.PFACX_TABLE_CHAIN).chainJumpLog2 == J
    info = _info(pats)
    assert info.filterTailEntries > 0
    return CompilerSet(name, pats, tagged=[prefix], veto=1, spares_walks=True,
                       extra={"J": J, "pair": pair, "fan9": fan9, "fan130": fan130, "stem": stem, "p300": p300, "p700": p700})


# ----------------------------------------------------------------------------------------------------------------------- dense fast table

def chain_states(patterns):
    """(states of the trie as PFACX_getInfo counts them: numOfStates, the unused state 0 included; internal states with exactly one successor)"""
    children = {b"": set()}
    for p in patterns:
        for d in range(len(p)):
            children.setdefault(p[:d], set()).add(p[d])
    whole = set(patterns)
    internal = [q for q in children if q not in whole]                       # (a final state with successors is numbered among the final ones)
    inside = sum(1 for q in internal if len(children[q]) == 1 and q != b"")
    return len(whole) + len(internal) + 1, inside


def _fast(name):
    if name == "fast_chains":
        pats = _words(np.random.Generator(np.random.PCG64(21)), 330, 20, np.frombuffer(b"ab", dtype=np.uint8))
    else:                                                                    # 6000 / 7950 of the 8000 three-letter words over 20 letters
        rng = np.random.Generator(np.random.PCG64(9))
        every = [bytes([a, b, c]) for a in LOW[:20] for b in LOW[:20] for c in LOW[:20]]
        pats = sorted(every[i] for i in rng.permutation(len(every))[:6000 if name == "fast_under" else 7950])
    states, inside = chain_states(pats)
    info = _info(pats)
    assert info.numOfStates == states, (info.numOfStates, states)
    fast = states <= DENSE_FAST_MAX_STATES and inside * 4 < states
    assert fast == (name == "fast_under"), (states, inside)
    if name == "fast_over":
        assert states > DENSE_FAST_MAX_STATES and inside * 4 < states
    if name == "fast_chains":
        assert states <= DENSE_FAST_MAX_STATES and inside * 4 >= states
    return CompilerSet(name, pats, veto=1 if info.filterTailEntries else 0, extra={"fast": fast, "states": states})


_BUILDERS = {}
for _names, _fn in ((("tags1", "tags7", "tags8", "tags9", "tag_ends", "tag_branch"), _tags),
                    (("rest4", "rest5", "rest6", "rest7", "rest17", "rest255", "rest256"), _rest),
                    (("lds5000", "glob8000", "lds5000_short"), _lds), (("glob_far",), _glob_far), (("deep_kept", "deep_refused"), _deep), (("extend0", "thin2"), _thin),
                    (("tiny",), _tiny), (("final3_8", "final3_9"), _final3), (("short_shrink",), _short_shrink), (("salted",), _salted),
                    (("shared_hash",), _shared_hash), (("chains",), _chains), (("fast_under", "fast_over", "fast_chains"), _fast)):
    for _n in _names:
        _BUILDERS[_n] = _fn
NAMES = tuple(_BUILDERS)
FAST_NAMES = ("fast_under", "fast_over", "fast_chains")


@functools.lru_cache(maxsize=None)
def get(name):
    return _BUILDERS[name](name)


@functools.lru_cache(maxsize=None)
def host_handle(name):
    """a host-only handle in hashed mode with the set read: the compiled tables for the models (never destroyed: cached for the process)"""
    h = api.PFAC.createHostOnly()
    h.setPerfMode(api.PFAC_SPACE_DRIVEN)
    h.readPatternFromFile(get(name).pattern_file)
    return h


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle import binding as ob
    return ob.Oracle(get(name).pattern_file, dense=False, hashed=True)


def oracle_match(name, data):
    """the hashed oracle's result vector (the dense table of the larger sets would be hundreds of MB; tests/test_oracle_golden.py pins both forms)"""
    return _oracle(name).match(np.ascontiguousarray(data), hashed=True, omp=True)


# ------------------------------------------------------------------------------------------------------------------------------ streams

def _put(data, at, p):
    data[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def stream(name, n=STREAM_BYTES):
    """(data, oracle result): filler that matches nothing ('0'..'5'; every set is made of other bytes) with complete patterns, near misses (the last
    1..4 bytes wrong), patterns truncated at a random length; for a tagged set a near miss with one wrong byte at each offset 6..23 of a tagged
    prefix; patterns that start 0..99 bytes in front of a 2 KiB chunk boundary; one pattern that ends exactly at the last byte, with a pattern that lacks its last byte
    right in front of it.  (stream(name)[0][:-2] cuts the last pattern off by the end of the input: both test files run that too.)"""
    cs = get(name)
    rng = np.random.Generator(np.random.PCG64(4242))
    data = (rng.integers(0, 6, n, dtype=np.uint8) + 48).astype(np.uint8)
    pool = [p for p in cs.patterns if len(p) >= 3]
    shorts = [p for p in cs.patterns if len(p) < 3]
    longest = max(len(p) for p in pool)
    room = n - 2 * longest - 64
    gap = 40 if n <= (1 << 20) else 400
    at, k = 7, 0
    planted = 0
    while at < room:
        p = pool[int(rng.integers(0, len(pool)))]
        kind = k % 4
        if kind == 1:
            cut = min(int(rng.integers(1, 5)), len(p) - 1)
            p = p[:-cut] + b"#" * cut                                       # near miss: right up to the last 1..4 bytes
        elif kind == 2:
            p = p[:int(rng.integers(1, len(p)))]                            # truncated: the input goes on with filler
        else:
            planted += 1
        _put(data, at, p)
        at += len(p) + int(rng.integers(1, 2 * gap))
        k += 1
        if shorts and k % 9 == 0:
            _put(data, at - 1 - len(shorts[k % len(shorts)]), shorts[k % len(shorts)])
    if n >= STREAM_BYTES:
        whole = [p for p in pool if len(p) >= 8] or pool
        for j in range(100):                                                # the veto's bytes lie partly outside what is staged
            p = whole[(j * 7919) % len(whole)]
            _put(data, CHUNK * (10 + j) - j, p)
        # (the compiler hands its eight tags out from the end of the sorted order: the last prefixes first)
        tagged = [p for t in sorted(cs.tagged, reverse=True)[:40] for p in [q for q in cs.patterns if q.startswith(t)][:2 if len(cs.tagged) <= 3 else 1]]
        spot = CHUNK * 120 + 5
        for p in tagged:
            for off in range(6, 24):
                _put(data, spot, p[:off] + b"#" + p[off + 1:])
                spot += len(p) + 3
            _put(data, spot, p)
            spot += len(p) + 3
        assert spot < CHUNK * 149
        spot = CHUNK * 112 + 9
        for p in cs.extra.get("near", []) + cs.extra.get("far", []):          # (glob_far) complete, and with the last byte wrong
            _put(data, spot, p)
            _put(data, spot + len(p) + 2, p[:-1] + b"#")
            spot += 2 * len(p) + 5
        assert spot < CHUNK * 120
    last = pool[(len(pool) * 2) // 3]
    cut = pool[len(pool) // 3]
    if len(cut) >= 3:
        _put(data, n - len(last) - (len(cut) - 1), cut[:-1])
    _put(data, n - len(last), last)
    want = oracle_match(name, data)
    assert want[n - len(last)] > 0 and np.count_nonzero(want) >= planted // 2, (name, int(np.count_nonzero(want)), planted)
    data.setflags(write=False)
    want.setflags(write=False)
    return data, want


@functools.lru_cache(maxsize=1)
def dense_stream(name, n=DENSE_BYTES):
    """(data, oracle result) of a fast_* set: n bytes of the set's own alphabet at random -- every 3-gram of it is the start of a pattern or nearly
    so --, whole patterns every 40 bytes in the last MiB, one ending with the input"""
    cs = get(name)
    rng = np.random.Generator(np.random.PCG64(99))
    alpha = np.frombuffer(bytes(sorted({b for p in cs.patterns for b in p})), dtype=np.uint8)
    data = alpha[rng.integers(0, alpha.size, n)]
    for k, at in enumerate(range(n - (1 << 20), n - 64, 40)):
        _put(data, at, cs.patterns[k % len(cs.patterns)])
    _put(data, n - len(cs.patterns[5]), cs.patterns[5])
    want = oracle_match(name, data)
    assert want[n - len(cs.patterns[5])] > 0
    data.setflags(write=False)
    want.setflags(write=False)
    return data, want
