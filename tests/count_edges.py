"""The cases of tests/test_count_edges_host.py and tests/test_count_edges_gpu.py: PFACX_countPairsFromDevice where pfac_count_hist
(scan_count.hip) takes another path -- at the edges of a lane's quad of ids, of a wave's 256 elements, of a block's trip of 1024, of a slot
of the tagged cache and of one pass of the grid.  No test functions and nothing of the library: the reference (histogram: np.bincount of
the ids inside [1, F]), a plain Python transcription of pfac_count_hist<true> and <false> (hist_model) whose `mutate` switches on one named
off-by-one at a time and whose `order` is the order in which lanes and waves reach the LDS atomics -- the claim of a cache slot is a race on
the device --, and builders of cases

    (name, ids, shift, F)               the list starts `shift` ints behind a 16-byte boundary; F: 5 (direct), 16383 (direct, the last
                                        LDS word), 16384 and 16385 (the tagged cache)

each with `.claims`, the edges it says it reaches, which claim_holds() re-derives from the list alone for the grid the case was built for:
element j = shift + i of the aligned ints is k = j % 4 of lane (j / 4) % 64 of wave (j / 256) % 4 of trip j / 1024 / grid of block
j / 1024 % grid.  Never through the model.

    A  shift 0 .. 3 x counts 1 .. 9 and 1020 .. 1029; lists that are one run; a run from the partial first quad into the partial last one;
       junk in the first and in the last element: the two conditions of loadQuad's 16-byte load
    B  every (start k, end k') of a run that ends in its lane, the next, two lanes on and lane 63; a run that fills a wave, 257 from a wave's
       first element, 256 from its second; runs over a wave and over a trip boundary; the last run of a wave; a run cut by junk; runs of mixed
       junk; alternating ids: heads, any, above, nextLane, first, next and run.  At shift 0 and 3
    C  pass = 2 C 1024 ids on C compute units: pass - 1, pass, pass + 1, 3 pass + 5; pass - 2 at shift 3 (one thread opens the second trip);
       1024 k at shift 0 (a block without a quad) and 1024 k - 2 at shift 3 (a block for the alignment's quad), k = 2 C - 1; an id once in
       every trip of a block; one run: every wave adds 256
    D  F = 16384 and 16385, ids by their slot (id * 0x9E3779B1) >> 19: two and four ids of a slot, every id once and three times, slots 0
       and 8191, id F among junk, a slot claimed in a block's first trip and hit by another id in its second
    E  F = 16383 and 16384, the same lists: id F as one run, id F and F + 1 alternating, F - 1, F, F + 1 in runs

OUT OF SCOPE, deliberately: the grid-stride loops of pfac_count_store and pfac_count_chain (they need F + 1 > 2048 C patterns, over
524 288 on 256 compute units: no set of the project is that large); the 64-bit total of a pair list (PFACX_countPairsFromDevice passes no
h_total: the total stays covered through PFACX_countFromDevice in tests/test_count_gpu.py); PFACX_countNonzeroFromDevice (test_nonzero_counts
has its block and scan-step edges).

Test infrastructure only."""
import functools

import numpy as np

THREADS = 256                           # scan_count.hip: kCountThreads
PER = 4                                 # kCountPer: consecutive ids per lane
TRIP = THREADS * PER                    # kCountTrip: ids a block takes per trip
WAVE = 64 * PER                         # elements of a wave
LDS_WORDS = 16384                       # kCountLdsWords == kCountDirect (pfac_amd/api.py: PFACX_COUNT_LDS_DIRECT)
CACHE_LOG2 = 13                         # kCountCacheLog2
SLOTS = 1 << CACHE_LOG2
MULTIPLIER = 0x9E3779B1                 # slot = (id * MULTIPLIER) >> (32 - kCountCacheLog2)
BLOCKS_PER_CU = 2                       # PFACX_countPairs: gridCap(c, 2)
M32, M64 = 0xFFFFFFFF, (1 << 64) - 1
INT_MAX, INT_MIN = (1 << 31) - 1, -(1 << 31)
OUTSIDE = 1                             # what lies in front of and behind a list, in the model and on the device: a VALID id, so that a read
                                        # outside the list is counted

FIVE = 5                                # the five-pattern set of test_id_lists_at_every_alignment_and_length
SETS = (FIVE, 16383, 16384, 16385)

# name -> what it changes.  equivalent_mutants() lists the ones no list can tell from the kernel
MUTANTS = {
    "quad_lt": "loadQuad: j + 4 < end for <= end",
    "quad_le_plus_1": "loadQuad: j + 4 <= end + 1",
    "quad_gt": "loadQuad: j > shift for >= shift",
    "quad_ge_minus_1": "loadQuad: j + 1 >= shift",
    "lane0_not_forced": "head[0] = v[0] != prev in lane 0 too (__shfl_up gives lane 0 its own last id)",
    "next_drops_first": "next = nextLane * 4, without firstThere",
    "above_includes_own": "above = any & (~0 << lane): the own lane's heads are among the lanes above",
    "last_run_63": "the last run of a wave ends at 63 * 4",
    "raw_compare": "heads from the ids as loaded, the filter behind the comparison",
    "filter_le": "the filter: v - 1 <= numIds",
    "no_second_trip": "the trip loop of a block runs once",
    "loser_dropped": "an id whose slot is another's is not added to hist",
    "owner_not_accepted": "only owner == 0 adds to the slot: the winner's later runs go to hist",
    "flush_unchecked": "the flush of the cache adds hist[id] without id - 1 < numIds",
    "filter_le_flush_unchecked": "filter_le and flush_unchecked together",
}


def equivalent_mutants():
    """name -> (why no list can tell it from the kernel, the neighbour that a list does tell).
    quad_lt, quad_gt: the condition only chooses between one 16-byte load and four loads with bounds of the SAME four ints; a whole quad
    that takes the second form has the same ids (it costs time, not counts).  What goes wrong is a 16-byte load of a quad that is NOT whole:
    one int more on either side, quad_le_plus_1 and quad_ge_minus_1, which count the int outside the list.
    raw_compare: junk compared raw makes more heads, but every run of junk is skipped whatever its length, and a valid id differs from its
    neighbours raw iff it differs folded.  The fold in front of the comparison saves atomics, never a count.
    owner_not_accepted: the winner's second run goes to hist with a global atomic and its first waits in the slot for the flush: each run is
    added once, in one place or the other.
    flush_unchecked: a tag is an id that loadQuad let through, so the check never decides -- unless the filter is wrong as well
    (filter_le_flush_unchecked writes hist[F + 1]).
    filter_le in CACHE mode alone is caught by the flush's check and changes no count; in DIRECT mode id F + 1 is added to the word behind
    the cleared ones (at F + 1 == 16384: behind the array), which the model reports as a stray write: it is NOT in this table"""
    return {"quad_lt": ("a whole quad loaded int by int holds the same ids", "quad_le_plus_1"),
            "quad_gt": ("only quad 0 at shift 0 changes form, and it holds the same ids", "quad_ge_minus_1"),
            "raw_compare": ("runs of junk are skipped whatever their number and length", "filter_le"),
            "owner_not_accepted": ("every run is added once: to the slot or to hist", "loser_dropped"),
            "flush_unchecked": ("a tag has passed the filter of loadQuad", "filter_le_flush_unchecked")}


# ---------------------------------------------------------------------------------------------------------------- the reference

def histogram(ids, f):
    """uint64[F + 1]: np.bincount over the ids inside [1, F]; entry 0 is 0"""
    ids = np.asarray(ids, dtype=np.int64)
    return np.bincount(ids[(ids >= 1) & (ids <= f)], minlength=f + 1).astype(np.uint64)


def slot_of(i):
    return ((int(i) * MULTIPLIER) & M32) >> (32 - CACHE_LOG2)


@functools.lru_cache(maxsize=None)
def slots(f):
    """slot -> the ids of [1, f] that hash to it, ascending"""
    ids = np.arange(1, f + 1, dtype=np.uint64)
    s = ((ids * np.uint64(MULTIPLIER)) & np.uint64(M32)) >> np.uint64(32 - CACHE_LOG2)
    out = {}
    for i, k in zip(ids.tolist(), s.tolist()):
        out.setdefault(k, []).append(i)
    return out


def check_slots():
    """what family D relies on, for ids 1 .. 16384"""
    by = slots(16384)
    assert set(by) == set(range(SLOTS)) and {len(v) for v in by.values()} == {1, 2, 3, 4}, "every slot has between 1 and 4 ids"
    assert by[0] == [4181, 10946, 15127] and by[SLOTS - 1] == [6765]
    assert all(slot_of(i) == s for s in (0, 1, SLOTS - 1) for i in by[s])
    return by


# ---------------------------------------------------------------------------------------------------------------- the model

def launch_grid(count, compute_units):
    """PFACX_countPairs: trips = (count + 2 * kCountPer + kCountTrip - 1) / kCountTrip, at most gridCap(c, 2) blocks"""
    return min((count + 2 * PER + TRIP - 1) // TRIP, BLOCKS_PER_CU * compute_units)


def hist_model(ids, shift, f, grid, order="ascending", mutate=None):
    """pfac_count_hist<F + 1 <= kCountDirect> over `grid` blocks, line by line -> (hist as uint64[F + 1], stray): stray lists every add that
    lands outside the cleared LDS words or outside hist[1, F] -- the kernel has none.  order: "ascending" or "descending", the order of the
    lanes of a wave and of the waves of a block at an atomic (within a lane k runs 3 .. 0, as in the kernel).  Every read outside the list
    reads OUTSIDE"""
    assert mutate is None or mutate in MUTANTS
    assert order in ("ascending", "descending")
    ids = [int(x) & M32 for x in np.asarray(ids).tolist()]
    count = len(ids)
    direct = f + 1 <= LDS_WORDS
    used = f + 1 if direct else LDS_WORDS
    end = shift + count
    quads = (shift + count + PER - 1) // PER
    hist, stray = {}, []
    le = mutate in ("filter_le", "filter_le_flush_unchecked")
    unchecked = mutate in ("flush_unchecked", "filter_le_flush_unchecked")

    def aligned(x):
        return ids[x - shift] if shift <= x < end else OUTSIDE

    def fold(v):
        d = (v - 1) & M32
        return v if (d <= f if le else d < f) else 0

    def to_hist(i, c):
        if 1 <= i <= f:
            hist[i] = (hist.get(i, 0) + c) & M32
        else:
            stray.append(("hist", i))

    def load_quad(q):
        j = q * PER
        lo = j + 1 >= shift if mutate == "quad_ge_minus_1" else j > shift if mutate == "quad_gt" else j >= shift
        hi = j + PER < end if mutate == "quad_lt" else j + PER <= end + 1 if mutate == "quad_le_plus_1" else j + PER <= end
        if lo and hi:
            return [aligned(j + k) for k in range(PER)]
        return [aligned(j + k) if shift <= j + k < end else 0 for k in range(PER)]

    lanes = list(range(64)) if order == "ascending" else list(range(63, -1, -1))
    waves = list(range(THREADS // 64)) if order == "ascending" else list(range(THREADS // 64 - 1, -1, -1))
    for block in range(grid):
        lds, tag, cnt = {}, {}, {}
        q0 = block * THREADS
        while q0 < quads:
            for wave in waves:
                raw = [load_quad(q0 + wave * 64 + l) if q0 + wave * 64 + l < quads else [0] * PER for l in range(64)]
                v = raw if mutate == "raw_compare" else [[fold(x) for x in four] for four in raw]
                head, anyone = [], 0
                for l in range(64):
                    prev = v[l - 1][PER - 1] if l else v[0][PER - 1]                      # __shfl_up: lane 0 keeps its own
                    h = [(l == 0 and mutate != "lane0_not_forced") or v[l][0] != prev] + [v[l][k] != v[l][k - 1] for k in range(1, PER)]
                    head.append(h)
                    if any(h):
                        anyone |= 1 << l
                first = [0 if h[0] else 1 if h[1] else 2 if h[2] else 3 for h in head]
                adds = [[] for _ in range(PER)]                                            # by k: (lane, id, run)
                for l in range(64):
                    if mutate == "above_includes_own":
                        above = anyone & (M64 << l) & M64
                    else:
                        above = 0 if l == 63 else anyone & (M64 << (l + 1)) & M64
                    next_lane = (above & -above).bit_length() - 1 if above else 0
                    there = 0 if mutate == "next_drops_first" else first[next_lane]
                    nxt = next_lane * PER + there if above else (63 if mutate == "last_run_63" else 64) * PER
                    for k in range(PER - 1, -1, -1):
                        if not head[l][k]:
                            continue
                        e = l * PER + k
                        run, nxt = (nxt - e) & M32, e
                        i = fold(v[l][k]) if mutate == "raw_compare" else v[l][k]
                        if i:
                            adds[k].append((l, i, run))
                for k in range(PER - 1, -1, -1):
                    for l, i, run in (adds[k] if order == "ascending" else adds[k][::-1]):
                        if direct:
                            if i < used:
                                lds[i] = (lds.get(i, 0) + run) & M32
                            else:
                                stray.append(("lds", i))
                            continue
                        s = slot_of(i)
                        owner = tag.get(s, 0)
                        if owner == 0:
                            tag[s] = i
                        if owner == 0 or (owner == i and mutate != "owner_not_accepted"):
                            cnt[s] = (cnt.get(s, 0) + run) & M32
                        elif mutate != "loser_dropped":
                            to_hist(i, run)
            q0 += grid * THREADS
            if mutate == "no_second_trip":
                break
        if direct:
            for i in sorted(lds):
                if lds[i]:
                    to_hist(i, lds[i])
        else:
            for s in sorted(tag):
                if cnt.get(s, 0) and (unchecked or 1 <= tag[s] <= f):
                    to_hist(tag[s], cnt[s])
    out = np.zeros(f + 1, dtype=np.uint64)
    for i, c in hist.items():
        out[i] = c
    return out, stray


# ---------------------------------------------------------------------------------------------------------------- cases and claims

class Case(tuple):
    """(name, ids, shift, F) and, beside the tuple, .claims"""

    def __new__(cls, name, ids, shift, f, claims=()):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        assert ids.size and ids.min() >= INT_MIN and ids.max() <= INT_MAX and 0 <= shift < PER and f in SETS
        self = super().__new__(cls, (name, ids.astype(np.int32), int(shift), int(f)))
        self.claims = tuple(claims)
        return self

    name = property(lambda self: self[0])

    def want(self):
        return histogram(self[1], self[3])


def folded(case):
    """the ids as the kernel compares them, by element of the aligned ints: 0 in front of the list, for junk and behind it, up to a whole
    trip"""
    _, ids, shift, f = case
    n = (shift + ids.size + TRIP - 1) // TRIP * TRIP
    out = np.zeros(n, dtype=np.int64)
    v = ids.astype(np.int64)
    out[shift:shift + ids.size] = np.where((v >= 1) & (v <= f), v, 0)
    return out


def wave_runs(p):
    """(start, end, id) of every run of a wave, end exclusive, as elements of the aligned ints: runs of equal folded ids, cut where a wave
    ends"""
    head = np.ones(p.size, dtype=bool)
    head[1:] = p[1:] != p[:-1]
    head[::WAVE] = True
    start = np.flatnonzero(head)
    return start, np.append(start[1:], p.size), p[start]


def place(j, grid):
    """element j of the aligned ints -> (block, trip, wave, lane, k)"""
    q = j // PER
    return (q // THREADS) % grid, q // THREADS // grid, (q % THREADS) // 64, q % 64, j % PER


def trips_of(block, quads, grid):
    return len(range(block * THREADS, quads, grid * THREADS))


def claim_holds(case, claim, compute_units):
    """one claim of the case, from its list and the grid of `compute_units` alone"""
    name, ids, shift, f = case
    count = int(ids.size)
    grid = launch_grid(count, compute_units)
    quads = (shift + count + PER - 1) // PER
    p = folded(case)
    kind, args = claim[0], claim[1:]
    if kind == "count":
        return count == args[0]
    if kind == "run":                                     # a valid run from lane a, k = b to (its last element) lane c, k = d of one wave
        a, b, c, d = args
        start, end, what = wave_runs(p)
        s, e = start % WAVE, (end - 1) % WAVE
        return bool(np.any((what != 0) & (s == a * PER + b) & (e == c * PER + d)))
    if kind == "no_head":                                 # the lane has no head in a wave in which a lane below and a lane above have one
        lane, = args
        for w in range(0, p.size, WAVE):
            el = p[w:w + WAVE]
            h = np.ones(WAVE, dtype=bool)
            h[1:] = el[1:] != el[:-1]
            per_lane = h.reshape(64, PER).any(axis=1)
            if not per_lane[lane] and per_lane[:lane].any() and per_lane[lane + 1:].any() and el[lane * PER] != 0:
                return True
        return False
    if kind == "spans":                                   # one valid run on both sides of element j, the first of a wave inside a trip / of a trip's 1024
        j, what = args
        at = place(j, grid)
        edge = at[3:] == (0, 0) and (at[2] != 0 if what == "wave" else at[2] == 0 and j > 0)
        return bool(edge and p[j - 1] == p[j] != 0)
    if kind == "ends_with_wave":                          # a valid run whose last element is a wave's last, the next element another id or none
        start, end, what = wave_runs(p)
        hit = (what != 0) & (end % WAVE == 0) & (start % WAVE != 0)
        return bool(np.any(hit & np.array([e >= p.size or p[e] != w for e, w in zip(end.tolist(), what.tolist())])))
    if kind == "fills_wave":                              # a valid run that is exactly a wave's 256 elements, other ids on both sides
        start, end, what = wave_runs(p)
        hit = np.flatnonzero((what != 0) & (end - start == WAVE))
        return any(p[start[h] - 1] != what[h] and (end[h] >= p.size or p[end[h]] != what[h]) for h in hit if start[h] > 0)
    if kind == "valid_run":                               # a maximal run of one valid id over elements [a, b)
        a, b = args
        return bool(p[a] != 0 and np.all(p[a:b] == p[a]) and p[a - 1] != p[a] and p[b] != p[a])
    if kind == "cut_by_junk":                             # x J x inside the list: one junk id between two runs of one valid id
        raw = ids.astype(np.int64)
        bad = (raw < 1) | (raw > f)
        i = np.flatnonzero(bad[1:-1] & ~bad[:-2] & ~bad[2:]) + 1
        return bool(np.any(raw[i - 1] == raw[i + 1]))
    if kind == "junk_between":                            # a run of junk of at least `n` different values between two valid ids
        n, = args
        raw = ids.astype(np.int64)
        bad = ((raw < 1) | (raw > f)).astype(np.int8)
        edge = np.flatnonzero(np.diff(np.concatenate([[0], bad, [0]])))
        return any(lo > 0 and hi < count and len(set(raw[lo:hi].tolist())) >= n for lo, hi in zip(edge[::2].tolist(), edge[1::2].tolist()))
    if kind == "every_element_heads":
        return bool(np.all(p[shift + 1:shift + count] != p[shift:shift + count - 1]) and np.all(p[shift:shift + count] != 0))
    if kind == "one_run":                                 # the whole list is one valid id
        return bool(np.all(ids == ids[0]) and 1 <= ids[0] <= f)
    if kind == "waves_of_one_run":                        # at least n waves whose 256 elements are one valid run
        start, end, what = wave_runs(p)
        return int(np.count_nonzero((what != 0) & (end - start == WAVE))) >= args[0]
    if kind == "partial_run":                             # a valid run from inside the partial first quad to inside the partial last one
        if shift == 0 or (shift + count) % PER == 0 or quads < 3:
            return False
        start, end, what = wave_runs(p)
        first = np.flatnonzero((start == shift) & (what != 0))
        return bool(first.size and PER * (quads - 1) < end[first[0]] <= shift + count - 1)
    if kind == "junk_first":
        return not 1 <= int(ids[0]) <= f and 1 <= int(ids[1]) <= f
    if kind == "junk_last":
        return not 1 <= int(ids[-1]) <= f and 1 <= int(ids[-2]) <= f
    if kind == "contains":
        return set(args) <= set(ids.tolist())
    if kind == "quads":                                   # the quads of the list as the address cuts it: `whole` by one 16-byte load
        total, whole = args
        lo, hi = (shift + PER - 1) // PER, (shift + count) // PER
        return quads == total and max(hi - lo, 0) == whole
    if kind == "grid":
        return grid == args[0]
    if kind == "trips":                                   # block b (negative: from the last) takes n trips
        b, n = args
        return trips_of(b % grid, quads, grid) == n
    if kind == "one_thread_in_last_trip":                 # the last trip of block 0 is one quad
        return quads == (trips_of(0, quads, grid) - 1) * grid * THREADS + 1
    if kind == "no_quad":                                 # the last block of the grid has no quad
        return grid >= 2 and trips_of(grid - 1, quads, grid) == 0 and trips_of(grid - 2, quads, grid) == 1
    if kind == "last_block_one_quad":
        return grid >= 2 and quads == (grid - 1) * THREADS + 1
    if kind == "passes":                                  # the list is more than n passes of the grid
        return count > args[0] * grid * TRIP and grid == BLOCKS_PER_CU * compute_units
    if kind == "in_every_trip":                           # the id occurs in every trip of the block, of which there are at least n
        i, b, n = args
        where = np.flatnonzero(p == i)
        at = {(x // TRIP // grid) for x in where.tolist() if (x // TRIP) % grid == b}
        return trips_of(b, quads, grid) >= n and at == set(range(trips_of(b, quads, grid)))
    if kind == "share_slot":                              # ids (all in the list, all valid) of one slot
        s, members = args[0], args[1:]
        return all(slot_of(i) == s and 1 <= i <= f for i in members) and set(members) <= set(ids.tolist()) and len(set(members)) == len(members)
    if kind == "whole_slot":                              # ... and they are all the ids of the set in that slot
        s, members = args[0], args[1:]
        return sorted(members) == slots(f).get(s, [])
    if kind == "every_id":                                # every id of the set occurs n times
        return bool(np.all(histogram(ids, f)[1:] == args[0]))
    if kind == "claimed_then_hit":                        # block b: trip 0 brings x and no other id of its slot, trip 1 brings y of that slot and not x
        b, x, y = args
        same = [i for i in slots(f)[slot_of(x)]]
        if slot_of(y) != slot_of(x) or x == y or trips_of(b, quads, grid) < 2:
            return False
        seen = []
        for trip in (0, 1):
            lo = (trip * grid + b) * TRIP
            seen.append({i for i in same if np.any(p[lo:lo + TRIP] == i)})
        return seen == [{x}, {y}]
    if kind == "mode":
        return ("direct" if f + 1 <= LDS_WORDS else "cache") == args[0]
    if kind == "last_word":                               # id F counts into lds[16383]
        return f + 1 == LDS_WORDS and f in ids.tolist()
    raise AssertionError("unknown claim %r" % (claim,))


def check_claims(case, compute_units):
    assert case.claims, case.name
    for claim in case.claims:
        assert claim_holds(case, claim, compute_units), (case.name, claim, compute_units)


def random_runs(n, seed, f=FIVE, junk=(0, -1, INT_MAX, INT_MIN), most=6, tail=()):
    """n ids in runs of 1 .. most: ids of [1, f] (for a large set: of its first 40 and last 3) and junk, f + 1 among it; the last ids are
    `tail`"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pool = np.array(list(range(1, min(f, 40) + 1)) + [f - 2, f - 1, f] * (f > 40) + list(junk) + [f + 1], dtype=np.int64)
    length = rng.integers(1, most + 1, n)
    ids = np.repeat(pool[rng.integers(0, pool.size, n)], length)[:n]
    ids[n - len(tail):] = tail
    return ids


# ---------------------------------------------------------------------------------------------------------------- A: quads

A_SMALL = (1, 1, 2, 3, 3, 3, 5, 4, 4)
A_JUNK = ((-1, FIVE + 1), (0, INT_MIN))


def quads_claim(shift, count):
    return ("quads", (shift + count + PER - 1) // PER, max((shift + count) // PER - (shift + PER - 1) // PER, 0))


def quad_cases():
    """FAMILY A.  j >= shift && j + 4 <= end on both sides, for the first quad and for the last"""
    out = []
    for shift in range(PER):
        for count in range(1, 10):
            out.append(Case("A-shift%d-%d" % (shift, count), A_SMALL[:count], shift, FIVE, [("count", count), quads_claim(shift, count)]))
        for count in range(1020, 1030):
            out.append(Case("A-shift%d-%d" % (shift, count), random_runs(count, 100 * shift + count), shift, FIVE,
                            [("count", count), quads_claim(shift, count), ("contains", 0, -1, FIVE + 1, INT_MIN)]))
        for count in (3, 9, 1025):
            out.append(Case("A-shift%d-one-run-%d" % (shift, count), [3] * count, shift, FIVE, [("one_run",), quads_claim(shift, count)]))
        for k, (first, last) in enumerate(A_JUNK):
            ids = [first, 1, 1, 2, 2, 2, 2, 2, 4, 4, last]
            out.append(Case("A-shift%d-junk-at-both-ends-%d" % (shift, k), ids, shift, FIVE, [("junk_first",), ("junk_last",), ("contains", first, last)]))
    for shift in (1, 2, 3):
        n = 8 + (PER - shift) + 1                                  # the run ends on the first int of the last quad; one other id behind it
        out.append(Case("A-shift%d-run-from-partial-to-partial" % shift, [1] * n + [3], shift, FIVE, [("partial_run",), quads_claim(shift, n + 1)]))
    return out


# ---------------------------------------------------------------------------------------------------------------- B: runs in and across waves

B_SHIFTS = (0, 3)
B_LANE = 5
B_ENDS = (("same-lane", B_LANE), ("next-lane", B_LANE + 1), ("two-lanes-on", B_LANE + 2), ("lane63", 63))
B_WAVE = 1                                 # the wave of block 0 the runs are built in: behind the list's first ints at every shift


def background(n):
    """n elements of the aligned ints in which every element heads a run: 4, 5, 4, 5, ..."""
    return 4 + (np.arange(n, dtype=np.int64) & 1)


def b_case(name, p, shift, claims):
    return Case("B-shift%d-%s" % (shift, name), p[shift:], shift, FIVE, claims)


def run_cases():
    """FAMILY B.  runs of id 1 in a background of alternating 4 and 5, placed by element of the aligned ints: the same lanes at either shift"""
    out = []
    w = B_WAVE * WAVE
    for shift in B_SHIFTS:
        for what, last in B_ENDS:
            for sk in range(PER):
                for ek in range(PER):
                    if last == B_LANE and ek < sk:
                        continue
                    p = background(3 * WAVE)
                    p[w + B_LANE * PER + sk:w + last * PER + ek + 1] = 1
                    claims = [("run", B_LANE, sk, last, ek)]
                    if last == B_LANE + 2 or (last == 63 and ek < PER - 1):      # (a run to the wave's end: no head above it at all)
                        claims.append(("no_head", B_LANE + 1))
                    if (last, ek) == (63, PER - 1):
                        claims.append(("ends_with_wave",))
                    out.append(b_case("k%d-to-%s-k%d" % (sk, what, ek), p, shift, claims))
        for name, lo, hi, n, claims in (
                ("run-of-256-fills-a-wave", w, w + WAVE, 3 * WAVE, [("fills_wave",), ("valid_run", w, w + WAVE)]),
                ("run-of-257-from-a-wave's-first", w, w + WAVE + 1, 3 * WAVE, [("valid_run", w, w + WAVE + 1), ("spans", w + WAVE, "wave"), ("waves_of_one_run", 1)]),
                ("run-of-256-from-a-wave's-second", w + 1, w + WAVE + 1, 3 * WAVE, [("valid_run", w + 1, w + WAVE + 1), ("spans", w + WAVE, "wave")]),
                ("run-over-255|256", 250, 262, 2 * WAVE, [("valid_run", 250, 262), ("spans", 256, "wave")]),
                ("run-over-1023|1024", 1019, 1030, TRIP + WAVE, [("valid_run", 1019, 1030), ("spans", 1024, "trip")]),
                ("last-run-of-a-wave", w + 201, w + WAVE, 3 * WAVE, [("valid_run", w + 201, w + WAVE), ("ends_with_wave",)])):
            p = background(n)
            p[lo:hi] = 1
            out.append(b_case(name, p, shift, claims))
        p = background(WAVE)                                       # ... and as the end of the list: the last run of the last wave
        p[170:] = 2
        out.append(b_case("last-run-ends-the-list", p, shift, [("ends_with_wave",), ("count", WAVE - shift)]))
        p = background(2 * WAVE)
        p[40:90] = 1
        p[61] = -1
        p[300:330] = 2
        p[311] = FIVE + 1
        out.append(b_case("run-cut-by-one-junk-id", p, shift, [("cut_by_junk",), ("contains", -1, FIVE + 1)]))
        p = np.repeat(np.array([1, 0, -1, FIVE + 1, INT_MIN, 2, 2, INT_MAX, 0, 0, 3, -1, 1, 1, 1, 1, 1, FIVE + 1, INT_MIN, -7, 5] * 30, dtype=np.int64),
                      np.array([3, 1, 1, 1, 1, 2, 1, 2, 1, 1, 1, 5, 1, 1, 1, 1, 1, 1, 1, 1, 2] * 30))
        out.append(b_case("runs-of-mixed-junk", p, shift, [("junk_between", 4), ("junk_between", 3), ("contains", 0, -1, FIVE + 1, INT_MIN, INT_MAX)]))
        p = 1 + (np.arange(2 * WAVE + 7, dtype=np.int64) % 3)
        out.append(b_case("alternating-ids", p, shift, [("every_element_heads",)]))
    return out


# ---------------------------------------------------------------------------------------------------------------- C: trips and grid

C_TAIL = (4, 5, 5)
C_NAMES = ("C-pass-1", "C-pass", "C-pass+1", "C-3pass+5", "C-pass-2-shift3", "C-1024k-shift0", "C-1024k-2-shift3", "C-id-in-every-trip", "C-one-run")


def trip_cases(compute_units):
    """FAMILY C.  one pass of the grid is 2 C blocks of 1024 ids.  The last three ids of a random list are valid: what a last trip of one
    quad holds decides a count"""
    full = BLOCKS_PER_CU * int(compute_units)
    one = full * TRIP
    k = full - 1
    out = [Case("C-pass-1", random_runs(one - 1, 1, tail=C_TAIL), 0, FIVE, [("count", one - 1), ("grid", full), ("trips", 0, 1), ("trips", -1, 1)]),
           Case("C-pass", random_runs(one, 2, tail=C_TAIL), 0, FIVE, [("count", one), ("grid", full), ("trips", 0, 1), ("trips", -1, 1)]),
           Case("C-pass+1", random_runs(one + 1, 3, tail=C_TAIL), 1, FIVE, [("grid", full), ("trips", 0, 2), ("trips", -1, 1), ("passes", 1)]),
           Case("C-3pass+5", random_runs(3 * one + 5, 4, tail=C_TAIL), 2, FIVE, [("grid", full), ("trips", 0, 4), ("trips", -1, 3), ("passes", 3)]),
           Case("C-pass-2-shift3", random_runs(one - 2, 5, tail=C_TAIL), 3, FIVE, [("grid", full), ("trips", 0, 2), ("one_thread_in_last_trip",), ("trips", -1, 1)]),
           Case("C-1024k-shift0", random_runs(TRIP * k, 6, tail=C_TAIL), 0, FIVE, [("count", TRIP * k), ("grid", k + 1), ("no_quad",)]),
           Case("C-1024k-2-shift3", random_runs(TRIP * k - 2, 7, tail=C_TAIL), 3, FIVE, [("count", TRIP * k - 2), ("grid", k + 1), ("last_block_one_quad",), ("trips", -1, 1)])]
    ids = 1 + (np.arange(3 * one + 5, dtype=np.int64) // 3) % 2              # runs of three of ids 1 and 2; id 3 once in every trip of block 0
    ids[np.arange(4) * one + np.array([0, 517, TRIP - 1, 2])] = 3
    out.append(Case("C-id-in-every-trip", ids, 0, FIVE, [("in_every_trip", 3, 0, 4), ("passes", 3), ("trips", 0, 4)]))
    out.append(Case("C-one-run", np.full(2 * one + 7, 2), 0, FIVE, [("one_run",), ("waves_of_one_run", 2 * one // WAVE), ("passes", 2), ("trips", 0, 3)]))
    assert tuple(c[0] for c in out) == C_NAMES
    return out


# ---------------------------------------------------------------------------------------------------------------- D: the cache

D_SETS = (16384, 16385)
D_LISTS = ("two-ids-of-a-slot-alternating", "a-full-slot-in-runs", "a-full-slot-interleaved", "every-id-once", "every-id-three-times-shuffled",
           "slots-0-and-8191", "id-F-among-junk", "claimed-in-trip-0-hit-in-trip-1")


def cache_cases(compute_units):
    """FAMILY D.  ids chosen by their slot"""
    by = check_slots()
    full_slot = min(s for s, v in by.items() if len(v) == 4)
    four = by[full_slot]
    zero, last = by[0], by[SLOTS - 1]
    one = BLOCKS_PER_CU * int(compute_units) * TRIP
    out = []
    for f in D_SETS:
        assert slots(f)[full_slot] == four and slots(f)[0] == zero, "id 16385 joins neither slot"
        lists = {}
        a, b = zero[0], zero[1]
        # (a lane of a, a lane of b at shift 0: both head at k = 0, so the order of the lanes decides who owns the slot)
        lists[D_LISTS[0]] = (np.tile(np.repeat([a, b], PER), 250), [("share_slot", 0, a, b), ("run", 0, 0, 0, PER - 1), ("run", 1, 0, 1, PER - 1)])
        lists[D_LISTS[1]] = (np.repeat(np.array(four * 3), [5, 1, 300, 2, 1, 7, 260, 3, 1, 1, 1, 520]),
                             [("share_slot", full_slot, *four), ("whole_slot", full_slot, *four)])
        lists[D_LISTS[2]] = (np.tile(four, 300), [("share_slot", full_slot, *four), ("whole_slot", full_slot, *four), ("every_element_heads",)])
        lists[D_LISTS[3]] = (np.arange(1, f + 1), [("every_id", 1), ("every_element_heads",)])
        rng = np.random.Generator(np.random.PCG64(f))
        lists[D_LISTS[4]] = (rng.permutation(np.repeat(np.arange(1, f + 1), 3)), [("every_id", 3)])
        lists[D_LISTS[5]] = (np.repeat(np.array((zero + last) * 40), np.arange(1, 1 + 40 * (len(zero) + 1)) % 7 + 1),
                             [("share_slot", 0, *zero), ("whole_slot", 0, *zero), ("share_slot", SLOTS - 1, *last), ("whole_slot", SLOTS - 1, *last)])
        lists[D_LISTS[6]] = (np.repeat(np.array([f, f + 1, f, 0, -1, f, f, INT_MAX, INT_MIN, f, f - 1, f + 1] * 50), np.arange(600) % 5 + 1),
                             [("contains", f, f + 1, 0, -1, INT_MAX, INT_MIN), ("junk_between", 2)])
        x, y = four[0], four[3]
        filler = np.array([i for i in range(1, 1200) if slot_of(i) != full_slot][:1000], dtype=np.int64)
        ids = filler[(np.arange(one + TRIP) // 3) % filler.size]
        ids[100:110] = x
        ids[700] = x
        ids[one + 50:one + 60] = y
        ids[one + 1000] = y
        lists[D_LISTS[7]] = (ids, [("claimed_then_hit", 0, x, y), ("share_slot", full_slot, x, y), ("trips", 0, 2), ("passes", 1)])
        assert tuple(lists) == D_LISTS
        for k, (what, (ids, claims)) in enumerate(lists.items()):
            out.append(Case("D-F%d-%s" % (f, what), ids, k % PER, f, claims + [("mode", "cache")]))
    return out


# ---------------------------------------------------------------------------------------------------------------- E: the threshold

E_SETS = (16383, 16384)
E_LISTS = ("id-F-as-one-run", "id-F-and-F+1-alternating", "F-1-F-F+1-in-runs")


def threshold_cases():
    """FAMILY E.  F + 1 == kCountDirect: id F counts into the last LDS word; F + 1 == kCountDirect + 1: the same list through the cache"""
    out = []
    for f in E_SETS:
        mode = [("mode", "direct"), ("last_word",)] if f + 1 == LDS_WORDS else [("mode", "cache")]
        out.append(Case("E-F%d-%s" % (f, E_LISTS[0]), np.full(2 * TRIP + 9, f), 1, f, [("one_run",), ("waves_of_one_run", 7)] + mode))
        out.append(Case("E-F%d-%s" % (f, E_LISTS[1]), np.tile([f, f + 1], 700), 0, f, [("contains", f, f + 1), ("cut_by_junk",)] + mode))
        out.append(Case("E-F%d-%s" % (f, E_LISTS[2]), np.repeat(np.array([f - 1, f, f + 1, f, f - 1, f + 1] * 60), np.arange(360) % 9 + 1), 2, f,
                        [("contains", f - 1, f, f + 1), ("junk_between", 1)] + mode))
    return out


# ---------------------------------------------------------------------------------------------------------------- all of them

def families(compute_units):
    return {"A": quad_cases(), "B": run_cases(), "C": trip_cases(compute_units), "D": cache_cases(compute_units), "E": threshold_cases()}


def by_name(cases):
    out = {c[0]: c for c in cases}
    assert len(out) == len(cases), "case names are unique"
    return out


NAMES = {family: tuple(c[0] for c in cases) for family, cases in families(1).items()}      # the names do not depend on the device
