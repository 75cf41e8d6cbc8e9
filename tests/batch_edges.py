"""Cases for the edges of the batch fix-up kernels (pfac_amd/csrc/scan_batch.hip; tests/test_batch_edges_host.py, test_batch_edges_gpu.py):
test infrastructure only, no GPU code.  Every builder is seeded, a pure function of its arguments and cached for the process.

A case is a Case(name, set, data, offsets, nocase, want): `set` names the pattern list in SETS (pattern id = index + 1), `want` is the expected
per-segment vector where it is known BY CONSTRUCTION (the two large tables and the pair tables) and None elsewhere.  reference(case) is the
expected result: tests.segcount_ref.brute_seg_result (bytes.find per segment: no code of the library, none of the oracle) -- or `want`, which
tests/test_batch_edges_host.py checks against the brute force on whole segments.

Pattern sets
  arun      `a` x k for k = 1..70: maxWalk 69 > 64; over a run of `a` every position matches and every zone position crosses its end
  nested    the prefixes of lengths PREFIX_LENS of one 200-byte string P whose first byte occurs nowhere else in it: short slots, both halves of
            an extension unit (chain bytes 8..15 and 16..23), chains of several slots
  longzone  arun + nested: maxWalk 199, a zone of three and more strides of a 64-lane group
  drop      `GET /admin`, `min.php`, `qq`: a straddling pattern with nothing shorter inside
  grid      a 70-byte string and its 3-byte prefix

Tables (what each pins is listed in DESIGN.md 5a "edges under test")
  width-L (0..6), width-6-long-zone, trip-N (1..17), empties, long-slots, nocase          full_tables()
  grid-pass                                                                              grid_pass(cus)
  pairs-N (N in PAIR_COUNTS), one-block-all-dropped, all-dropped, none-dropped, many-blocks, pair-on-offset, no-pairs       pair_tables()
"""
import atexit
import collections
import functools
import os
import shutil
import tempfile

import numpy as np

from pfac_amd import api
from pfac_amd import workloads as wl
from tests.segcount_ref import brute_seg_result

BLOCK = api.PFACX_BATCH_BLOCK                    # scan_batch.hip: kBatchBlock
SEGS_PER_TRIP = api.PFACX_BATCH_SEGS_PER_TRIP    # kSegsPerTrip
MAX_GROUP_LOG2 = api.PFACX_BATCH_MAX_GROUP_LOG2  # the cap of groupLog2
GRID_PER_CU = 16                                 # PFACX_batchFixup: gridCap(c, 16)
SCAN_BLOCKS = 1024                               # PFACX_batchReduceFixup launches pfac_array_scan with one block of 1024 lanes: more blocks of pairs take a second trip

Case = collections.namedtuple("Case", "name set data offsets nocase want")

_DIR = tempfile.mkdtemp(prefix="pfac_batch_edges_")
atexit.register(shutil.rmtree, _DIR, ignore_errors=True)


# ---------------------------------------------------------------------------------------------------------------- coverage model
# The two functions below decide only WHICH CASE REACHES WHICH CODE (the host test asserts that every table sits where its name says);
# they never decide an expected result.  They mirror, in PFACX_batchFixup (scan_batch.hip):
#     const size_t mean = size / numSegments, want = mean < b.maxWalk ? (mean ? mean : 1) : b.maxWalk;
#     while (groupLog2 < 6 && (size_t(1) << groupLog2) < want) groupLog2++;
# and, in pfac_batch_fixup, `groups = (gridDim.x * kBatchBlock) >> groupLog2` with the stride `groups * kSegsPerTrip` at the full grid of
# gridCap(c, 16) = 16 blocks per compute unit.

def group_log2(size, num_segments, max_pattern_len):
    max_walk = max_pattern_len - 1
    mean = size // num_segments
    want = max(mean, 1) if mean < max_walk else max_walk
    log2 = 0
    while log2 < MAX_GROUP_LOG2 and (1 << log2) < want:
        log2 += 1
    return log2


def segments_per_pass(cus, log2):
    return ((cus * GRID_PER_CU * BLOCK) >> log2) * SEGS_PER_TRIP


def case_group_log2(case):
    return group_log2(int(case.data.size), len(case.offsets) - 1, max(len(p) for p in SETS[case.set]))


# ------------------------------------------------------------------------------------------------------------------- pattern sets

ARUN = [b"a" * k for k in range(1, 71)]
PREFIX_LENS = (2, 3, 8, 9, 10, 16, 17, 18, 24, 25, 26, 33, 64, 65, 100, 200)
_rng = np.random.Generator(np.random.PCG64(5101))
P = b"Z" + bytes(_rng.integers(ord("b"), ord("p") + 1, 199, dtype=np.uint8))          # `Z` (folded: `z`) occurs nowhere else in it
G70 = b"G" + bytes(_rng.integers(ord("b"), ord("p") + 1, 69, dtype=np.uint8))
del _rng
NESTED = [P[:k] for k in PREFIX_LENS]
NESTED_MIXED = [p.lower() if i % 2 else p.upper() for i, p in enumerate(NESTED)]      # the same set under PFACX_READ_NOCASE
DROP = [b"GET /admin", b"min.php", b"qq"]
SETS = {"arun": ARUN, "nested": NESTED, "nested-mixed": NESTED_MIXED, "longzone": ARUN + NESTED, "drop": DROP, "grid": [G70, G70[:3]]}
MAX_WALK = {name: max(len(p) for p in pats) - 1 for name, pats in SETS.items()}
FILLER = b"#0123"                                # starts no pattern of any set and is no byte of P or G70


@functools.lru_cache(maxsize=None)
def pattern_file(name):
    return wl.write_pattern_file(os.path.join(_DIR, f"batch_edges_{name}.pat"), SETS[name])


def longest_prefix_id(j):
    """the id (in `nested`) of the longest prefix pattern of P that is no longer than j bytes; 0: none"""
    fit = [i + 1 for i, k in enumerate(PREFIX_LENS) if k <= j]
    return fit[-1] if fit else 0


def _filler(n, k=0):
    return bytes(FILLER[(k + i) % len(FILLER)] for i in range(n))


def _case(name, set_name, segments, nocase=False, want=None, data=None):
    lens = [len(s) for s in segments]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    if data is None:
        data = np.frombuffer(b"".join(segments), dtype=np.uint8).copy()
    data.setflags(write=False)
    assert int(offsets[-1]) == data.size
    return Case(name, set_name, data, offsets, nocase, want)


def segment_lengths(case):
    return np.diff(case.offsets.astype(np.int64))


# --------------------------------------------------------------------------------------------------------------- 1: group widths

_MEANS = {0: (0, 1), 1: (2, 2), 2: (3, 4), 3: (5, 8), 4: (9, 16), 5: (17, 32), 6: (33, 64)}     # the means that give groupLog2 == L at maxWalk 69


def width_specials(log2):
    """the segment lengths every width table holds: empty, 1 byte, shorter than the group, maxWalk - 1, maxWalk, maxWalk + 1, about 3 x maxWalk"""
    w = MAX_WALK["arun"]
    return [0, 1, max((1 << log2) - 1, 0), w - 1, w, w + 1, 3 * w]


@functools.lru_cache(maxsize=None)
def width_case(log2):
    """a run of `a` (a `b` at the head of every fifth segment of two bytes and more) cut so that the mean segment gives groupLog2 == log2:
    the special lengths spread among as many segments of the mean's range as that takes (at least 40)"""
    lo, hi = _MEANS[log2]
    special = width_specials(log2)
    fill, size, k = [], sum(special), 0
    while len(fill) < 40 or group_log2(size, len(fill) + len(special), 70) != log2:
        fill.append(lo + k % (hi - lo + 1))
        size += fill[-1]
        k += 1
        assert k < 2000
    step = len(fill) // len(special)
    lens = []
    for i, n in enumerate(fill):
        lens.append(n)
        if i % step == step - 1 and i // step < len(special):
            lens.append(special[i // step])
    assert sorted(lens) == sorted(fill + special)
    segs = [(b"b" + b"a" * (n - 1)) if n >= 2 and i % 5 == 4 else b"a" * n for i, n in enumerate(lens)]
    return _case(f"width-{log2}", "arun", segs)


def _cuts(js, filler_len, continued):
    """[segments], [(position of P's first byte, j)]: for every j an occurrence of P cut by a segment end after j bytes.  continued: the next
    segment begins with the rest of P, so the scan over the concatenation reports the whole of P and the fix-up has to walk again; otherwise
    the next segment begins with filler, which is not P's next byte.  j == len(P): P ends exactly at the segment end and is kept."""
    segs, marks, at, rest = [], [], 0, b""
    for k, j in enumerate(js):
        head = rest + _filler(filler_len(k), k)
        segs.append(head + P[:j])
        marks.append((at + len(head), j))
        at += len(segs[-1])
        rest = P[j:] if continued else b""
    segs.append(rest + _filler(9))                # the last segment ends in filler: nothing walks at the end of the input
    return segs, marks


@functools.lru_cache(maxsize=None)
def width6_long_zone():
    """longzone set (maxWalk 199), every segment longer than 3 x 64 bytes: runs of `a` and cuts of P.  A group of 64 lanes strides three and
    four times through each zone"""
    cut, _ = _cuts((2, 9, 17, 33, 65, 100, 199, 200), lambda k: 200 + k, True)
    cut[-1] += _filler(200)
    return _case("width-6-long-zone", "longzone", [b"a" * 200, b"a" * 230] + cut + [b"a" * 257, b"a" * 193])


# ---------------------------------------------------------------------------------------------------------- 2, 3: trips, empties

@functools.lru_cache(maxsize=None)
def trip_case(n):
    """n segments of 5..9 bytes of a run of `a`: one trip and its tail lanes (n < 8), exactly one (8), one and a tail, two, two and one"""
    return _case(f"trip-{n}", "arun", [b"a" * (5 + (3 * i + n) % 5) for i in range(n)])


@functools.lru_cache(maxsize=None)
def empties():
    """empty segments first and last, a run of nine (a whole trip and one more), one between two segments that both need a fix-up"""
    lens = [0, 0, 7] + [0] * 9 + [12, 0, 12, 5, 0, 0]
    return _case("empties", "arun", [b"a" * n for n in lens])


# ---------------------------------------------------------------------------------------------------------------- 4, 7: long slots

@functools.lru_cache(maxsize=None)
def long_slots_marks():
    a, ma = _cuts(range(len(P) + 1), lambda k: 1 + k % 7, True)
    b, mb = _cuts(range(len(P) + 1), lambda k: 1 + k % 7, False)
    shift = sum(len(s) for s in a)
    return a + b, ma + [(p + shift, j) for p, j in mb]


@functools.lru_cache(maxsize=None)
def long_slots():
    """P cut after j bytes for EVERY j in 0..200, once with the rest of P at the head of the next segment and once with filler there"""
    return _case("long-slots", "nested", long_slots_marks()[0])


NOCASE_CUTS = tuple(sorted(set(PREFIX_LENS) | {k - 1 for k in PREFIX_LENS} | {k + 1 for k in PREFIX_LENS if k < 200} | {0, 5, 6, 12, 13, 14, 20, 21, 22, 28, 30, 40, 48, 56, 72, 80, 120, 150, 180}))


@functools.lru_cache(maxsize=None)
def nocase_case():
    """50 cuts of P, the rest at the head of the next segment, every letter of the input in a random case: for a PFACX_READ_NOCASE handle"""
    assert len(NOCASE_CUTS) == 50
    segs, _ = _cuts(NOCASE_CUTS, lambda k: 1 + k % 7, True)
    data = np.frombuffer(b"".join(segs), dtype=np.uint8).copy()
    rng = np.random.Generator(np.random.PCG64(5102))
    letter = (data >= ord("a")) & (data <= ord("z")) | (data >= ord("A")) & (data <= ord("Z"))
    data[letter & (rng.random(data.size) < 0.5)] ^= 0x20
    return _case("nocase", "nested-mixed", segs, nocase=True, data=data)


def full_tables():
    """every table of the full result but grid-pass"""
    return ([width_case(k) for k in range(MAX_GROUP_LOG2 + 1)] + [width6_long_zone()] + [trip_case(n) for n in range(1, 18)]
            + [empties(), long_slots(), nocase_case()])


# ------------------------------------------------------------------------------------------------------------------ 5: grid pass

@functools.lru_cache(maxsize=2)
def grid_pass(cus):
    """segments_per_pass(cus, 6) + 9 segments of 70 bytes: the grid of pfac_batch_fixup takes a second pass of one whole trip and one segment.
    Segment k ends in the first c(k) bytes of G70 and segment k + 1 begins with the rest: the scan reports G70 at 70 (k + 1) - c(k), the
    fix-up its 3-byte prefix (c >= 3) or nothing.  c runs 69, 68, ..., 0 and again; the last segment cuts nothing.  want: by construction"""
    nseg = segments_per_pass(cus, MAX_GROUP_LOG2) + 9
    g = np.frombuffer(G70, dtype=np.uint8)
    c = ((69 - np.arange(nseg)) % 70).astype(np.int16)
    c[-1] = 0
    before = np.concatenate([[0], c[:-1]]).astype(np.int16)
    x = np.arange(70, dtype=np.int16)[None, :]
    rows = np.full((nseg, 70), ord("#"), dtype=np.uint8)
    tail = x >= 70 - c[:, None]
    rows[tail] = g[np.clip(x - (70 - c[:, None]), 0, 69)][tail]
    head = (before[:, None] > 0) & (x < 70 - before[:, None])
    assert not (head & tail).any()
    rows[head] = g[np.clip(x + before[:, None], 0, 69)][head]
    data = rows.reshape(-1)
    want = np.zeros(data.size, dtype=np.int32)
    k = np.flatnonzero(c >= 3)
    want[k * 70 + 70 - c[k].astype(np.int64)] = 2
    offsets = (np.arange(nseg + 1, dtype=np.uint64) * np.uint64(70))
    data.setflags(write=False)
    want.setflags(write=False)
    return Case("grid-pass", "grid", data, offsets, False, want)


# ----------------------------------------------------------------------------------------------------------------- 6: pair tables

KEEP, GONE = b"qq.", (b"GET /", b"admin.")
PAIR_COUNTS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513)
MANY_PAIRS = 270_000                             # 1055 blocks of 256 pairs
MANY_DROPS = (5, 1025 * BLOCK + 17)


def claimed_drops(count):
    """pair indices that drop in pairs-<count>: the first lane, either side of the first wave's end and of the first block's end, the last pair"""
    return sorted({i for i in (0, 63, 64, 255, 256, count - 1) if i < count})


def _pair_case(name, count, drops, cut_every=3, empty_before=()):
    """`count` units, each ONE pair of the scan over the concatenation, in position order: a kept one is `qq.` (id 3), a dropped one is
    `GET /` | `admin.` with a segment end at the bar (id 1 over the concatenation, nothing inside either segment).  A segment ends behind every
    cut_every-th kept unit; empty_before: unit indices that get an empty segment in front (the unit then starts its segment)"""
    drops, empty_before = set(drops), set(empty_before)
    segs, cur, kept_at, at = [], b"", [], 0
    for i in range(count):
        if i in empty_before:
            segs += [cur, b""]
            cur = b""
        if i in drops:
            segs.append(cur + GONE[0])
            cur = GONE[1]
            at += len(GONE[0]) + len(GONE[1])
        else:
            kept_at.append(at)
            cur += KEEP
            at += len(KEEP)
            if i % cut_every == 0:
                segs.append(cur)
                cur = b""
    segs.append(cur)
    want = np.zeros(at, dtype=np.int32)
    want[np.asarray(kept_at, dtype=np.int64)] = 3
    want.setflags(write=False)
    return _case(name, "drop", segs, want=want)


@functools.lru_cache(maxsize=None)
def pair_case(name):
    if name.startswith("pairs-"):
        count = int(name[6:])
        return _pair_case(name, count, claimed_drops(count))
    if name == "one-block-all-dropped":
        return _pair_case(name, 3 * BLOCK, range(BLOCK, 2 * BLOCK))
    if name == "all-dropped":
        return _pair_case(name, 300, range(300))
    if name == "none-dropped":
        return _pair_case(name, 300, ())
    if name == "many-blocks":
        return _pair_case(name, MANY_PAIRS, MANY_DROPS)
    if name == "pair-on-offset":
        return _pair_case(name, 40, (), cut_every=1, empty_before=(0, 5, 6, 20, 39))
    if name == "no-pairs":
        segs = [_filler(n, n) for n in range(20)]
        return _case(name, "drop", segs, want=np.zeros(sum(range(20)), dtype=np.int32))
    raise KeyError(name)


PAIR_TABLES = tuple(f"pairs-{n}" for n in PAIR_COUNTS) + ("one-block-all-dropped", "all-dropped", "none-dropped", "many-blocks", "pair-on-offset", "no-pairs")
CLAIMED = {**{f"pairs-{n}": (n, claimed_drops(n)) for n in PAIR_COUNTS},
           "one-block-all-dropped": (3 * BLOCK, list(range(BLOCK, 2 * BLOCK))), "all-dropped": (300, list(range(300))), "none-dropped": (300, []),
           "many-blocks": (MANY_PAIRS, list(MANY_DROPS)), "pair-on-offset": (40, []), "no-pairs": (0, [])}


def pair_tables():
    return [pair_case(name) for name in PAIR_TABLES]


# --------------------------------------------------------------------------------------------------------------------- reference

_REFERENCE = {}


def reference(case):
    """the expected per-segment vector: the case's own (by construction) or the brute force, computed once"""
    if case.want is not None:
        return case.want
    if case.name not in _REFERENCE:
        want = brute_seg_result(SETS[case.set], case.data.tobytes(), case.offsets, case.nocase)
        want.setflags(write=False)
        _REFERENCE[case.name] = want
    return _REFERENCE[case.name]


def sample_segments(case, count=200, seed=1, always=()):
    """indices of `count` segments (or all): the first and last eighteen, `always`, the rest drawn at random"""
    nseg = len(case.offsets) - 1
    if nseg <= count:
        return np.arange(nseg)
    rng = np.random.Generator(np.random.PCG64(seed))
    fixed = set(range(18)) | set(range(nseg - 18, nseg)) | {int(k) for k in always}
    drawn = rng.choice(nseg, size=count, replace=False)
    return np.array(sorted(fixed | {int(k) for k in drawn[:max(0, count - len(fixed))]}), dtype=np.int64)


def brute_on_segments(case, segments):
    """[(segment index, brute-force vector of that segment alone)]"""
    pats, data = SETS[case.set], case.data
    out = []
    for k in segments:
        s, e = int(case.offsets[k]), int(case.offsets[k + 1])
        out.append((int(k), brute_seg_result(pats, data[s:e].tobytes(), [0, e - s], case.nocase)))
    return out


def segment_of(case, position):
    return int(np.searchsorted(case.offsets.astype(np.int64), position, side="right")) - 1
