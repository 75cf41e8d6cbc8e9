"""Cases for the four ordering launches of a compacted-output call (pfac_amd/csrc/scan_order.inc; tests/test_order_edges_host.py,
test_order_edges_gpu.py): test infrastructure only.  The ordering needs the pairs and the claimed input size n, not n bytes of input, so
PFACX_orderPairsProbe (include/pfac_module.h) reaches every bin width with a few thousand pairs.

A case is (n, positions, input order): `positions` a sorted array of distinct values below n, the ids a fixed mix of the position (ids_of), the
list handed to the probe positions[perm] with its ids.  The expected output is `positions` with their ids: numpy only.

  plan(n)                    the model of PairOrder::plan: shift, bins, padded (counters: whole blocks of kOrderBlockBins), words and per (the bitmap
                             of a crowded bin: 2^(shift - 5) words, `per` consecutive words per thread of the rank pass)
  capacity_fresh(n, pairs)   the pairs the scratch holds after plan(n, pairs) on a handle whose ordering scratch is empty
  grid_for(cus, items)       scan_passes.h: gridFor
  sizes(shift)               the first, a middle (ragged last bin) and the last n of a shift; for shift 6 the small sizes too
  cases(grid)                every case, by group; `grid` = the blocks of the count, scatter and rank launches on a handle whose scratch holds
                             8 * CUs * 256 pairs or more (the shared handle of the GPU test: grid_for(cus, anything that large) = 8 * CUs)

Totals (asserted by tests/test_order_edges_host.py): 184 cases -- 58 "size", 87 "bins", 5 "crowded", 12 "pairs", 20 "waves", 2 "fresh" --, the
largest 2 * grid * 256 + 77 pairs (1 048 653 at 256 CUs; the cap is 2 Mi), 3.9 M pairs in all at 256 CUs, 0.6 M of them outside "pairs" and "crowded".

Groups:
  size      per shift 6..15 and per n of sizes(shift): up to 2000 random positions with 0 and n - 1 among them, in random order; per shift the only
            pair of the input on position 0 and on position n - 1 (at the first and the last n of the shift)
  bins      per shift, at mid_n(shift) (49 670 bins: 48 whole blocks of counters and a ragged 49th): the occupancies(shift) in the named_bins(n),
            rotated through len(occupancies) cases so that every occupancy meets every named bin; 1500 background pairs in the other bins (the front
            sums of the offsets pass are sums of non-zero counters); ascending, descending and random input in turn
  crowded   1, grid - 1, grid, grid + 1, 2 grid + 3 bins of 65 pairs at shift 7: the rank pass takes one block per crowded bin, round after round
  pairs     0 .. 2 grid 256 + 77 pairs spread evenly at shift 7: the grid-stride loops of the count, scatter and rank pass take a second and third pass
  waves     per shift: "striped" -- every aligned run of 64 list entries (a wave of the count and scatter pass) lies in 64 different bins -- and
            "clumped" -- every aligned run of 64 lies in one bin, the clumps shuffled
  fresh     for a handle of its own: more crowded bins than capacity_fresh() gives blocks; a plain one beside it
"""
import functools
import os
import re
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constant(name):
    src = open(os.path.join(ROOT, "pfac_amd", "csrc", "scan_order.inc")).read()
    m = re.search(r"constexpr\s+unsigned\s+" + name + r"\s*=\s*(\d+)\s*;", src)
    assert m, name
    return int(m.group(1))


kOrderMaxBinsLog2 = _constant("kOrderMaxBinsLog2")
kOrderMinShift = _constant("kOrderMinShift")
kOrderMaxShift = _constant("kOrderMaxShift")
kOrderBlockBins = _constant("kOrderBlockBins")
kOrderCrowded = _constant("kOrderCrowded")
# the values the cases below were designed for
assert (kOrderMaxBinsLog2, kOrderMinShift, kOrderMaxShift, kOrderBlockBins, kOrderCrowded) == (16, 6, 15, 1024, 64)

SHIFTS = tuple(range(kOrderMinShift, kOrderMaxShift + 1))
MAX_PAIRS = 2 << 20                              # no case has more
POISON = 64                                      # ints on either side of the arrays handed to the probe
NOMINAL_CUS = 256                                # the host test builds the list for this many compute units (and for another count)


# ------------------------------------------------------------------------------------------------------------------------ the model

def _round256(b):
    return (b + 255) // 256 * 256


def plan(n):
    """PairOrder::plan(n): {shift, bins, padded, words, per}"""
    assert 0 < n < 1 << 31
    log2n = 1
    while log2n < 32 and (n - 1) >> log2n:
        log2n += 1
    shift = log2n - kOrderMaxBinsLog2 if log2n > kOrderMaxBinsLog2 + kOrderMinShift else kOrderMinShift
    assert shift <= kOrderMaxShift
    bins = ((n - 1) >> shift) + 1
    padded = (bins + kOrderBlockBins - 1) // kOrderBlockBins * kOrderBlockBins
    words = 1 << (shift - 5)
    return {"shift": shift, "bins": bins, "padded": padded, "words": words, "per": words // 256 if words > 256 else 1}


def fixed_bytes(n):
    """the counters, cursors and the list of crowded bins in front of the two pair arrays"""
    p = plan(n)
    return _round256(p["padded"] * 4 + 16) + p["padded"] * 4 + _round256(p["bins"] * 4)


def reserve_bytes(n, pairs):
    """what reduceScratch reserves for plan(n, pairs) when the scratch is smaller: need + need / 2 (DeviceBuffer::reserve allocates exactly that)"""
    need = fixed_bytes(n) + 2 * _round256(pairs * 4)
    return need + need // 2


def capacity_of(n, scratch_bytes):
    """OrderArgs::capacity of plan(n, ...) over a scratch of scratch_bytes"""
    per_array = (scratch_bytes - fixed_bytes(n)) // 2 // 256 * 256
    return min(per_array // 4, 0xFFFFFFFF)


def capacity_fresh(n, pairs):
    return capacity_of(n, reserve_bytes(n, pairs))


def grid_for(cus, items):
    """scan_passes.h: gridFor -- blocks of 256 threads for `items` items, one at least, eight per compute unit at most"""
    cap = (cus if cus > 0 else 256) * 8
    return max(1, min(cap, (items + 255) // 256))


def front_is_eight_deep(block):
    """orderOffsetsPhase: block `block` sums the counters in front of its own; does thread 0 take the loop with eight loads in flight?"""
    first_quad = block * (kOrderBlockBins // 4)
    return first_quad > 7 * 256


def first_eight_deep_block():
    return next(b for b in range(64) if front_is_eight_deep(b))


# ------------------------------------------------------------------------------------------------------------------------ sizes

def first_n(shift):
    return 1 if shift == kOrderMinShift else (1 << (15 + shift)) + 1


def last_n(shift):
    return min(1 << (16 + shift), (1 << 31) - 1)


def mid_n(shift):
    """between the two: 48 whole blocks of counters, 518 bins of a 49th, the last bin 29 positions short (shift 6: 41 positions wide)"""
    return (1 << (15 + shift)) + (1 << (14 + shift)) + (517 << shift) + ((1 << shift) - 29 if shift > 6 else 41)


SMALL_SIZES = (1, 2, 63, 64, 65, 64 * 1024, 64 * 1024 + 1, 64 * 8192 + 1)


def sizes(shift):
    if shift == kOrderMinShift:
        return SMALL_SIZES + (mid_n(shift), last_n(shift) - 1, last_n(shift))
    return (first_n(shift), mid_n(shift), last_n(shift))


# ------------------------------------------------------------------------------------------------------------------------ cases

def ids_of(pos):
    """a position written with another pair's id is seen"""
    p = np.asarray(pos, dtype=np.uint64)
    return (1 + ((p * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(1000003)).astype(np.int32)


ORDERS = ("ascending", "descending", "random", "striped", "clumped")


class Case:
    def __init__(self, group, name, n, pos, order, tags=()):
        self.group, self.name, self.n, self.order, self.tags = group, name, int(n), order, tuple(tags)
        self.pos = np.asarray(pos, dtype=np.int64)
        self.shift = plan(self.n)["shift"]
        assert order in ORDERS

    def __repr__(self):
        return f"{self.group}/{self.name}/{self.order}"

    @property
    def count(self):
        return int(self.pos.size)

    def rng(self):
        return np.random.Generator(np.random.PCG64(zlib.crc32(repr(self).encode())))

    def perm(self):
        """the input order: list entry k is pair perm()[k] of the sorted list"""
        c = self.count
        if self.order == "ascending":
            return np.arange(c)
        if self.order == "descending":
            return np.arange(c)[::-1].copy()
        if self.order == "random":
            return self.rng().permutation(c)
        bins = self.pos >> self.shift
        starts = np.flatnonzero(np.r_[True, bins[1:] != bins[:-1]])
        rank = np.arange(c) - np.repeat(starts, np.diff(np.r_[starts, c]))      # of a pair among the pairs of its bin
        if self.order == "striped":                                               # the first pair of every bin, then the second of every bin, ...
            return np.lexsort((bins, rank))
        # "clumped": every bin holds a multiple of 64 pairs, so every aligned 64 of the sorted list are one bin's: shuffled, and the clumps shuffled
        assert c > 0 and np.all(np.diff(np.r_[starts, c]) % 64 == 0)
        r = self.rng()
        return np.concatenate([r.permutation(64) + 64 * k for k in r.permutation(c // 64)])

    def histogram(self):
        return np.bincount(self.pos >> self.shift, minlength=plan(self.n)["bins"])


def _rng(*key):
    return np.random.Generator(np.random.PCG64(zlib.crc32(repr(key).encode())))


def bin_width(n, b):
    s = plan(n)["shift"]
    return min(1 << s, n - (b << s))


def occupancies(shift):
    """what a named bin holds, as (label, number of pairs or a builder of offsets); a bin narrower than the number (the ragged last bin) is full"""
    w = 1 << shift
    if shift == 6:                               # 64 pairs are the full bin and min(2^s, 4096); 65 do not exist
        return [("0", 0), ("1", 1), ("2", 2), ("63", 63), ("64=full", 64), ("first+last", "ends")]
    occ = [("0", 0), ("1", 1), ("2", 2), ("63", 63), ("64", 64), ("65", 65), ("min(2^s,4096)", min(w, 4096))]
    occ.append(("full", w) if shift <= 12 else ("33+33+every 97th", "ends97"))
    occ.append(("first+last", "ends"))
    return occ


def occupancy_offsets(n, b, what, rng):
    """the offsets inside bin b of an input of n bytes for occupancy `what`"""
    w = bin_width(n, b)
    if what == "ends":
        return np.unique(np.array([0, w - 1]))
    if what == "ends97":
        return np.unique(np.r_[np.arange(min(33, w)), np.arange(max(0, w - 33), w), np.arange(0, w, 97)])
    k = min(int(what), w)
    return np.sort(rng.choice(w, k, replace=False))


def named_bins(n):
    p = plan(n)
    deep = first_eight_deep_block() * kOrderBlockBins
    whole = p["bins"] // kOrderBlockBins * kOrderBlockBins
    return {"bin 0": 0, "bin 1": 1, "bin 1023": kOrderBlockBins - 1, "bin 1024": kOrderBlockBins, "bin 1025": kOrderBlockBins + 1,
            "bin 8191": deep - 1, "bin 8192": deep, "bin 8193": deep + 1, "last bin": p["bins"] - 1, "last bin of the last whole block": whole - 1}


def bins_layout(shift, r):
    """case r of the "bins" group: {label of a named bin: (bin, label of its occupancy, what)}"""
    n = mid_n(shift)
    occ = occupancies(shift)
    return {label: (b,) + occ[(j + r) % len(occ)] for j, (label, b) in enumerate(named_bins(n).items())}


def _bins_case(shift, r):
    n = mid_n(shift)
    rng = _rng("bins", shift, r)
    layout = bins_layout(shift, r)
    taken = {b for b, _, _ in layout.values()}
    parts = [(b << shift) + occupancy_offsets(n, b, what, rng) for b, _, what in layout.values()]
    back = rng.choice(n, 1500, replace=False)
    parts.append(back[~np.isin(back >> shift, list(taken))])
    return Case("bins", f"shift {shift}/rotation {r}", n, np.unique(np.concatenate(parts)), ORDERS[r % 3])


def _sample(n, count, rng):
    """`count` distinct positions below n (all of them when n is smaller), 0 and n - 1 among them"""
    if n <= count:
        return np.arange(n)
    pos = rng.choice(n, count, replace=False) if n < 1 << 24 else np.unique(rng.integers(0, n, count))
    return np.unique(np.r_[pos, 0, n - 1])


def _spread(n, count):
    return (np.arange(count, dtype=np.int64) * n) // max(count, 1)


CROWDED_N = (1 << 22) + (1 << 21) + 5            # shift 7, 49 153 bins
CROWDED_LABELS = ("1", "grid-1", "grid", "grid+1", "2*grid+3")
PAIRS_LABELS = ("0", "1", "63", "64", "65", "255", "256", "257", "grid*256-1", "grid*256", "grid*256+1", "2*grid*256+77")
FRESH_CROWDED_BINS = 300                         # of 65 pairs, on a handle of its own: capacity_fresh() gives fewer blocks than that


def crowded_counts(grid):
    return (1, grid - 1, grid, grid + 1, 2 * grid + 3)


def pair_counts(grid):
    return (0, 1, 63, 64, 65, 255, 256, 257, grid * 256 - 1, grid * 256, grid * 256 + 1, 2 * grid * 256 + 77)


def _crowded_case(group, label, bins_crowded):
    n = CROWDED_N
    p = plan(n)
    rng = _rng("crowded", label)
    step = max(1, (p["bins"] - 1) // bins_crowded)
    assert step * (bins_crowded - 1) < p["bins"] - 1           # the ragged last bin stays out of it
    parts = [(b * step << 7) + np.sort(rng.choice(128, kOrderCrowded + 1, replace=False)) for b in range(bins_crowded)]
    back = rng.choice(n, 1500, replace=False)
    parts.append(back[(back >> 7) % step != 0] if step > 1 else back[(back >> 7) >= bins_crowded])
    return Case(group, f"{label} crowded bins", n, np.unique(np.concatenate(parts)), "random", tags=(("crowded bins", bins_crowded),))


@functools.lru_cache(maxsize=None)
def cases(grid=NOMINAL_CUS * 8):
    """every case, in the order of the groups; grid: see the module's docstring"""
    out = []
    for s in SHIFTS:
        for n in sizes(s):
            out.append(Case("size", f"shift {s}/n {n}", n, _sample(n, 2000, _rng("size", n)), "random"))
        out.append(Case("size", f"shift {s}/the only pair on position 0", first_n(s) if s > 6 else mid_n(s), [0], "ascending"))
        out.append(Case("size", f"shift {s}/the only pair on position n - 1", last_n(s), [last_n(s) - 1], "ascending"))
    for s in SHIFTS:
        for r in range(len(occupancies(s))):
            out.append(_bins_case(s, r))
    for label, k in zip(CROWDED_LABELS, crowded_counts(grid)):
        out.append(_crowded_case("crowded", label, k))
    for label, k in zip(PAIRS_LABELS, pair_counts(grid)):
        out.append(Case("pairs", f"{label} pairs", CROWDED_N, _spread(CROWDED_N, k), "random", tags=(("pairs", k),)))
    for s in SHIFTS:
        n = mid_n(s)
        rng = _rng("waves", s)
        # 128 bins (two whole waves per level) of 3 pairs each, every 331st bin
        striped = np.concatenate([(b * 331 << s) + np.sort(rng.choice(1 << s, 3, replace=False)) for b in range(128)])
        out.append(Case("waves", f"shift {s}/64 bins per wave", n, np.sort(striped), "striped"))
        # 40 bins of 64 pairs (shift 6: full bins) or 128 (two clumps; crowded), every 1021st bin
        per_bin = 64 if s == 6 else 128
        clumped = np.concatenate([(b * 1021 << s) + np.sort(rng.choice(1 << s, per_bin, replace=False)) for b in range(40)])
        out.append(Case("waves", f"shift {s}/one bin per wave", n, np.sort(clumped), "clumped"))
    out.append(_crowded_case("fresh", "fresh handle, 300", FRESH_CROWDED_BINS))
    out.append(Case("fresh", "fresh handle, plain", CROWDED_N, _sample(CROWDED_N, 2000, _rng("fresh")), "random"))
    names = [repr(c) for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def group(name, grid=NOMINAL_CUS * 8, shift=None):
    return [c for c in cases(grid) if c.group == name and (shift is None or c.shift == shift)]


def shift_id(shift):
    """the id of a shift in the GPU test's parametrisation: the bitmap's words per thread ride along where there are several"""
    per = plan(mid_n(shift))["per"]
    return f"shift{shift}" + (f"-per{per}" if per > 1 else "")


# ------------------------------------------------------------------------------------------------------------------------ the real scans

PATTERNS = [b"h", b"ab", b"abc", b"mnop"]
FILLER = b"0123456789"                           # starts no pattern
REAL_SIZES = ((1 << 22) - 1, 1 << 22, (1 << 22) + 1, (1 << 23) + 1)
REAL_BIG = (1 << 24) + 1                         # a test of its own


def real_plants(n):
    """{what: (bin, pairs)} of real_input(n): the occupancies its plants give these bins under plan(n)'s shift"""
    p = plan(n)
    s, w = p["shift"], 1 << p["shift"]
    at = {"64": (3000, 64), "65": (3001, 65), "full": (5000, w), "bin 1023": (1023, 1), "bin 1024": (1024, 1), "bin 0": (0, 1), "last bin": (p["bins"] - 1, 1)}
    if s == 6:                                   # a bin of 64 positions: 64 pairs fill it and 65 do not exist -- 63 beside the full one
        at["64"], at["65"] = (3000, 63), (3001, 64)
    return at


@functools.lru_cache(maxsize=4)
def real_input(n):
    """n bytes of filler with the plants of real_plants(n) and a sprinkle of every pattern elsewhere"""
    p = plan(n)
    s, w = p["shift"], 1 << p["shift"]
    data = np.resize(np.frombuffer(FILLER, dtype=np.uint8), n).copy()
    rng = _rng("real", n)
    for at in rng.choice(n - 8, n // 1000, replace=False):     # background: the front sums are sums of non-zero counters
        b = int(at) >> s
        if b in (0, 1022, 1023, 1024, 2999, 3000, 3001, 4999, 5000, p["bins"] - 2, p["bins"] - 1):
            continue
        pat = PATTERNS[int(at) % 4]
        data[at:at + len(pat)] = np.frombuffer(pat, dtype=np.uint8)
    h = ord("h")
    plants = real_plants(n)
    for what in ("64", "65"):
        b, k = plants[what]
        if s == 6:
            data[(b << s):(b << s) + k] = h                     # 63: all but the bin's last position; 64: the whole bin
        else:
            data[(b << s):(b << s) + 128:2] = h                 # 64 pairs on the even offsets of the bin's first 128 positions
            if k == 65:
                data[(b << s) + 1] = h
    b = plants["full"][0]
    data[b << s:(b + 1) << s] = h
    data[0:3] = np.frombuffer(b"abc", dtype=np.uint8)           # a match on position 0
    data[(1024 << s) - 1:(1024 << s) + 1] = np.frombuffer(b"ab", dtype=np.uint8)     # on the last position of bin 1023, its end in bin 1024
    data[(1024 << s) + 1:(1024 << s) + 5] = np.frombuffer(b"mnop", dtype=np.uint8)
    data[n - 1] = h                                             # a match on position n - 1: the last bin
    return data


def hygiene_input():
    """300 KB with planted patterns for the real calls of the counter-hygiene sequence"""
    n = 300_000
    data = np.resize(np.frombuffer(FILLER, dtype=np.uint8), n).copy()
    rng = _rng("hygiene")
    for at in rng.choice(n - 8, 4000, replace=False):
        pat = PATTERNS[int(at) % 4]
        data[at:at + len(pat)] = np.frombuffer(pat, dtype=np.uint8)
    data[70_000:70_300] = ord("h")                              # crowded bins
    data[n - 1] = ord("h")
    return data


def capacity_edge():
    """n with capacity_fresh(n, 65536) == n: n bytes of `h` under the pattern `h` are n pairs, as many as the scratch of a first call holds (reduceScan
    plans a call of this size for 65536 pairs); n + 1 are one more"""
    n = 65536
    for _ in range(64):
        m = capacity_fresh(n, 65536)
        if m == n:
            return n
        n = m
    raise AssertionError("no fixed point")
