"""Fixtures for the edges of pfac_scan_tiled (tests/test_tiled_edges_host.py, test_tiled_edges_gpu.py): test infrastructure only.
Every builder is seeded, a pure function of its arguments and cached for the process; pattern_file(name) goes with all of them but the fuzz.

  pattern_file()            ONE set for every case but the fuzz: `q`, `zz`, a dozen patterns of 3..40 bytes (some of them prefixes of
                            others), a 60-byte pair that shares 31 bytes, a 200-byte and a 600-byte pattern (deeper than the 128 bytes
                            the kernel stages behind a group) and TAIL_CUT, whose first 30 bytes are the last 30 of the 600-byte one.
                            The filler -- `0123` -- starts no pattern.
  ragged(n)                 A: `q` runs over the first 40 and the last 41 bytes, LONG_A cut off by the end of the input, sparse middle
  walks(group, in_off, n)   B: plants across every group boundary (at group * k - in_off) and 128-byte halo edge; C: the same in 8 MiB
  shape_switch(group, off)  C: 8 MiB + 1 bytes with walks()' plants and dense stretches; the caller scans a prefix of n bytes
  thresholds_small/_big()   D: groups whose level-1 survivor counts (tests/filter_model.py: level1_model) sit on either side of the
                            kernel's crowded (> 256) and dense (survivors * 2 >= positions) thresholds
  fuzz_case(dir, seed)      E: random sets over tiny alphabets (the generator of test_fuzzed_pattern_sets_over_tiny_alphabets)
"""
import atexit
import functools
import os
import shutil
import tempfile

import numpy as np

from pfac_amd import api
from pfac_amd import workloads as wl
from tests.filter_model import level1_model

TILE, HALO = 1024, 128                           # scan_tiled.hip: kTiledTile, kTiledHalo
GROUP_SMALL, GROUP_BIG, GROUP_REF = 1024, 4096, 2048       # bytes of a wave's group: small shape, big shape, big shape of PFACX_KERNEL_REFTABLE
BIG_BYTES = 8 << 20                              # kTiledBigBytes: ScanArgs::owned from which a launch takes the big shape
LIST = 256                                       # kTiledList: a group with more survivors is `crowded`
Q, Z = ord("q"), ord("z")
FILLER = np.frombuffer(b"0123", dtype=np.uint8)

_DIR = tempfile.mkdtemp(prefix="pfac_tiled_edges_")
atexit.register(shutil.rmtree, _DIR, ignore_errors=True)


def _letters(rng, lo, hi, count):
    return bytes(rng.integers(lo, hi, count, dtype=np.uint8))


_rng = np.random.Generator(np.random.PCG64(7101))
LONG_A = _letters(_rng, 97, 113, 15) + b"q" * 45                     # 'a'..'p', then a run of the 1-byte pattern: one long single-successor chain
LONG_B = LONG_A[:31] + _letters(_rng, 65, 91, 29)                    # shares 31 bytes, then diverges
P200 = _letters(_rng, 97, 113, 200)
P600 = _letters(_rng, 97, 113, 600)
TAIL_CUT = P600[570:] + b"ABCDEFGH"                                  # behind a P600 that ends with the input: 30 bytes match, the rest lies beyond n
PREFIXES = [LONG_A[:9], LONG_A[:17], LONG_B[:40], LONG_A[5:25]]       # patterns that are prefixes (or pieces) of patterns
SHORT = [_letters(_rng, 97, 113, k) for k in (3, 4, 5, 8, 12, 16, 24, 33, 40)]
PATTERNS = [b"q", b"zz"] + SHORT + PREFIXES + [TAIL_CUT, LONG_A, LONG_B, P200, P600]
# The 1-byte pattern is folded into the 3-gram bitmap as every 3-gram that begins with it, and a set this small gets the smallest
# bitmap (8192 bits): the 65 536 3-grams fill it, nine filler positions in ten pass the early-out and EVERY group of the tiled
# kernel is dense (test_tiled_edges_host.py pins that).  So every case runs under two sets: "q" -- this one: the dense branch at
# every edge -- and "qq", the same lines with `qq` in the place of `q`: no filler position passes, a group is as dense as its
# `q` runs make it, and the sparse result paths (LDS tile, whole zero lines, per-position stores), the plain and the crowded
# listing run at the same edges.  Only "qq" can place a group on either side of a threshold.
SETS = {"q": PATTERNS, "qq": [b"qq"] + PATTERNS[1:]}
del _rng


def pattern_id(p):
    """the result the oracle reports for a match of p: its line in the pattern file, from 1"""
    return PATTERNS.index(p) + 1


@functools.lru_cache(maxsize=None)
def pattern_file(name="q"):
    return wl.write_pattern_file(os.path.join(_DIR, f"tiled_edges_{name}.pat"), SETS[name])


@functools.lru_cache(maxsize=None)
def host_handle(name="q"):
    """a host-only handle: the compiled filter tables for the model (never destroyed: cached for the process)"""
    h = api.PFAC.createHostOnly()
    h.readPatternFromFile(pattern_file(name))
    return h


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle import binding as ob
    return ob.Oracle(pattern_file(name), hashed=False)


def want(data, name="q", omp=False):
    """the oracle's result vector for exactly these bytes under the set `name`"""
    return _oracle(name).match(data, omp=omp)


def _put(data, at, p):
    data[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)


def _filler(rng, n):
    return FILLER[rng.integers(0, 4, n)].copy()


# ------------------------------------------------------------------------------------------------------------------------------- A

RAGGED_M = (1, 2, 3, 7, 15, 16, 17, 31, 33, 1023, 1024, 1025, 1151, 1152, 1153, 4095, 4096, 4097, 4224, 65537)
RAGGED_CUT = 56                                  # LONG_A planted this far in front of the end: 4 of its 60 bytes lie beyond n


def ragged_sizes(in_off):
    """m and m - in_off (where positive): the input, or the input with the bytes in front of it, ends at the 16-byte lane, the
    1 KiB group, the group plus halo, the four waves of a block"""
    return sorted({n for m in RAGGED_M for n in (m, m - in_off) if n > 0})


@functools.lru_cache(maxsize=None)
def ragged(n):
    """data: `q` runs over the first 40 and the last 41 bytes (a `q` at 0 and at n - 1; a first or last group that holds
    little more than its run is dense AND partial), in front of the last run the 15 letters of LONG_A -- whose 60 bytes would
    need 4 bytes beyond n: the oracle reports LONG_A[:17] -- and a sparse middle."""
    rng = np.random.Generator(np.random.PCG64(5000 + n))
    data = _filler(rng, n)
    pool = [LONG_A[:17], b"zz", b"q", LONG_B[:40], SHORT[2], LONG_A[:59] + b"#", SHORT[8], LONG_B]
    at, k = 48, 0
    while at + 60 < n - RAGGED_CUT:
        _put(data, at, pool[k % len(pool)])
        at += 60 + int(rng.integers(30, 400))
        k += 1
    data[:40] = Q
    data[max(0, n - RAGGED_CUT + 15):] = Q
    if n - RAGGED_CUT >= 40:
        _put(data, n - RAGGED_CUT, LONG_A[:15])
    data.setflags(write=False)
    return data


# --------------------------------------------------------------------------------------------------------------------------- B and C

WALKS_N = 110 * 1024 + 777                       # one boundary per plant: 72 + 24 + 12 of them
_ROTATION = [LONG_A, LONG_A[:59] + b"#", LONG_B, LONG_A[:17], LONG_B[:40], LONG_A[:9] + b"#", LONG_A[:30] + b"#"]
START_BEFORE = (1, 16, 71, 72, 73, 199)          # a long pattern starts this far in front of a group's end
END_BEHIND = (127, 128, 129)                     # ... or ENDS this far behind it: the last byte from the stage, the first from global memory, one further


def plant_specs():
    """[(bytes, offset of the plant's first byte from a group boundary, complete pattern or None)]: what walks() plants, one per boundary"""
    specs = []
    for j in range(72):                          # a 60-byte walk (or its near miss, twin, prefix-patterns) straddles the boundary at every offset
        p = _ROTATION[j % len(_ROTATION)]
        specs.append((p, -j, p if p in PATTERNS else None))
    deep = {}
    for p in (P200, P600):
        deep[len(p)] = []
        for whole in (True, False):
            q = p if whole else p[:-1] + b"#"    # near miss: walked to its last byte, nothing (or a shorter pattern) reported
            deep[len(p)] += [(q, -d, p if whole else None) for d in START_BEFORE]
            deep[len(p)] += [(q, e + 1 - len(p), p if whole else None) for e in END_BEHIND]
    for a, b in zip(deep[200], deep[600]):       # in turn: a P600 that ends just behind a boundary begins 472 bytes in front of it
        specs += [a, b]
    return specs


def _plant_at_boundaries(data, specs, boundaries, planted):
    """every plant across the next of the (ascending) boundaries it reaches without touching the plant in front of it"""
    boundaries = iter(boundaries)
    free = 0
    for p, rel, whole in specs:
        at = next(boundaries) + rel
        while at < free:
            at = next(boundaries) + rel
        b = at - rel
        assert at >= 0 and at + len(p) + 2 <= data.size and at <= b < at + max(len(p), 72)     # across (a short one: up to) the boundary, inside the input
        _put(data, at, p)
        free = at + len(p) + 8
        if whole is not None:
            planted.append((at, pattern_id(whole)))


@functools.lru_cache(maxsize=None)
def walks(group=GROUP_SMALL, in_off=0, n=WALKS_N):
    """(data, planted): every plant of plant_specs() across its own group boundary -- the groups of a call whose input
    pointer is in_off bytes behind a 16-byte address end at group * k - in_off --, a P600 that ends exactly at n, TAIL_CUT running
    into n behind it.  planted = [(position, pattern id)] of the complete patterns."""
    rng = np.random.Generator(np.random.PCG64(6000 + group + in_off))
    data = _filler(rng, n)
    specs, planted = plant_specs(), []
    _plant_at_boundaries(data, specs, range(group - in_off, n - 1300, group), planted)
    _put(data, n - 600, P600)
    planted.append((n - 600, pattern_id(P600)))
    data.setflags(write=False)
    return data, planted


SWITCH_SIZES = (BIG_BYTES - 1, BIG_BYTES, BIG_BYTES + 1)


@functools.lru_cache(maxsize=4)
def shape_switch(group, in_off):
    """(data, planted) of 8 MiB + 1 bytes, to be scanned as data[:n] for n in SWITCH_SIZES (the oracle runs on those very
    bytes): walks()' plants relative to the groups of the big shape -- all of them from the third boundary on (at 4 KiB a group they
    reach beyond the first 256 KiB: a boundary takes one plant), every fifth again in the last 64 KiB --, isolated `q`s and short
    patterns sprinkled over the filler, and dense stretches (`q`: a match at every position; `z`: `zz` at every position) over the
    first group, over the last, partial one (up to the last byte, for every n), over one group between sparse neighbours and over
    ten groups in a row."""
    n = BIG_BYTES + 1
    rng = np.random.Generator(np.random.PCG64(7000 + group + in_off))
    data = _filler(rng, n)
    data[rng.integers(0, n, n // 700)] = Q
    for at in rng.integers(0, n - 64, 3000):
        _put(data, int(at), PATTERNS[int(at) % len(SHORT + PREFIXES) + 2])
    specs, planted = plant_specs(), []
    _plant_at_boundaries(data, specs, range(group * 3 - in_off, n, group), planted)
    last = (n + in_off) // group * group - in_off            # the boundary in front of the last group of every n
    tail = specs[::5][:(64 << 10) // group - 3]
    _plant_at_boundaries(data, tail, range(last - group * (len(tail) + 1), last - group, group), planted)
    data[:group + 300] = Q
    data[last - group - 700:] = Z                            # (8 MiB - 1 may end one group earlier than 8 MiB + 1)
    lone = group * 1000 - in_off
    data[lone:lone + group] = Q
    data[(2 << 20) + 77:(2 << 20) + 77 + 10 * group] = Z
    data.setflags(write=False)
    return data, planted


# ------------------------------------------------------------------------------------------------------------------------------- D

def survivors(data, group, index, name="qq"):
    """positions of group `index` (aligned input: positions [group * index, group * (index + 1))) that pass the kernel's early-out"""
    lo = group * index
    return int(level1_model(host_handle(name), data[lo:lo + group + 2])[:group].sum())


def _fit_group(data, lo, size, target):
    """`q`s in the filler of data[lo:lo + size] until exactly `target` of its positions survive level 1 under the "qq" set: a `q`
    in front of a `q` survives (the 2-byte pattern is folded into the bitmap), so `qq` every size / target bytes -- or, for half
    of the positions and more, `qqq` every four -- to begin with; then, since a 3-gram with one `q` may hit the bitmap as well,
    one byte at a time against the model."""
    h = host_handle("qq")

    def count():
        return int(level1_model(h, data[lo:lo + size + 2])[:size].sum())

    if target == size:
        data[lo:lo + size + 1] = Q
    elif 3 * target <= size:
        for k in range(target):
            data[lo + k * (size // target):lo + k * (size // target) + 2] = Q
    else:
        for k in range(min(target // 2, size // 4)):
            data[lo + 4 * k:lo + 4 * k + 3] = Q
    def around(at):                                # the positions whose 3-gram holds byte `at`
        a, b = max(lo, at - 2), min(at + 1, lo + size)
        return int(level1_model(h, data[a:b + 2])[:b - a].sum())

    have = count()
    top = lo + size - 2                            # what lies behind it has been tried in this direction
    while have != target:
        for at in range(top, lo - 1, -1):
            add = have < target
            if (data[at] == Q) == add:
                continue
            old, before = data[at], around(at)
            data[at] = Q if add else FILLER[at & 3]
            now = have + around(at) - before
            if (have < now <= target) if add else (target <= now < have):
                have, top = now, at
                break
            data[at] = old
        else:
            raise AssertionError(f"no single byte brings {have} survivors nearer to {target}")
    assert count() == target


SMALL_TARGETS = (255, 256, 257, 511, 512, 513, 1024)       # of 1024: either side of `crowded` (> 256) and of dense (>= 512), and all


@functools.lru_cache(maxsize=None)
def thresholds_small():
    """(data, groups): 1 KiB groups (aligned input, small shape) with exactly SMALL_TARGETS survivors, and two skewed
    crowded ones -- `lane16`: 19 lanes hold all 16 positions of their 16 bytes (`q` runs at 16-byte aligned offsets), the others
    next to none; `lane5`: every lane holds about 5 (`qq` every four bytes) -- each between two sparse groups.  groups = {target or name: group index}."""
    names = list(SMALL_TARGETS) + ["lane16", "lane5"]
    n = (2 * len(names) + 1) * GROUP_SMALL + 333
    rng = np.random.Generator(np.random.PCG64(8001))
    data = _filler(rng, n)
    groups = {}
    for k, name in enumerate(names):
        g = 2 * k + 1
        lo = g * GROUP_SMALL
        groups[name] = g
        if name == "lane16":
            for lane in range(0, 57, 3):
                data[lo + 16 * lane:lo + 16 * lane + 17] = Q
        elif name == "lane5":
            for off in (0, 1, 4, 5, 8, 9, 12, 13):
                data[lo + off:lo + GROUP_SMALL:16] = Q
        else:
            _fit_group(data, lo, GROUP_SMALL, name)
    _put(data, n - 300, LONG_B)
    data.setflags(write=False)
    return data, groups


BIG_TARGETS = {GROUP_BIG: (2047, 2048, 2049), GROUP_REF: (1023, 1024, 1025)}     # either side of dense: half of the group's positions


@functools.lru_cache(maxsize=None)
def thresholds_big():
    """(data, groups) of exactly 8 MiB (aligned: the big shape): 4 KiB groups with 2047, 2048 and 2049 survivors (the
    chained-table kernel's group) and 2 KiB groups with 1023, 1024 and 1025 (PFACX_KERNEL_REFTABLE's), each between sparse groups,
    in a stream of filler with isolated `q`s and short patterns.  groups = {(group bytes, target): group index}."""
    n = BIG_BYTES
    rng = np.random.Generator(np.random.PCG64(8002))
    data = _filler(rng, n)
    data[rng.integers(0, n, n // 700)] = Q
    for at in rng.integers(0, n - 700, 2000):
        _put(data, int(at), PATTERNS[int(at) % (len(PATTERNS) - 2) + 2])
    groups = {}
    first = {GROUP_BIG: 40, GROUP_REF: 1500}
    for group, targets in BIG_TARGETS.items():
        for k, target in enumerate(targets):
            g = first[group] + 2 * k
            data[group * g - 64:group * (g + 1) + 64] = _filler(rng, group + 128)
            _fit_group(data, group * g, group, target)
            groups[group, target] = g
    data.setflags(write=False)
    return data, groups


# ------------------------------------------------------------------------------------------------------------------------------- E

def fuzz_case(workdir, seed):
    """(pattern_file, data): a random pattern set over a 2-4 symbol alphabet -- patterns that are prefixes of patterns at every depth,
    long single-successor chains, 1- and 2-byte patterns (odd seeds), bytes 0x00 / 0xFF -- and 40 000..200 000 bytes over the same
    alphabet, in which almost every position walks, with the set's longest string planted once."""
    rng = np.random.Generator(np.random.PCG64(900 + seed))
    alphabet = [bytes([b]) for b in rng.choice([0x00, 0xFF, 0x41, 0x42, 0x7A, 0x20, 0x0D], size=int(rng.integers(2, 5)), replace=False)]
    pats = set()
    base = b"".join(alphabet[int(i)] for i in rng.integers(0, len(alphabet), 48))
    for cut in rng.integers(1, 48, int(rng.integers(3, 14))):           # prefixes of one long string
        pats.add(base[:int(cut)])
    while len(pats) < int(rng.integers(8, 70)):
        ln = int(rng.integers(1 if seed % 2 else 3, 41))
        pats.add(b"".join(alphabet[int(i)] for i in rng.integers(0, len(alphabet), ln)))
    pats = sorted(pats, key=lambda p: (rng.random(), p))               # file order = pattern IDs: shuffled
    pf = wl.write_pattern_file(os.path.join(workdir, f"fuzz{seed}.pat"), pats)
    n = int(rng.integers(40_000, 200_000))
    idx = rng.integers(0, len(alphabet), n)
    data = np.frombuffer(b"".join(alphabet), dtype=np.uint8)[idx].copy()
    at = int(rng.integers(0, n - 100))
    data[at:at + len(base)] = np.frombuffer(base, dtype=np.uint8)
    return pf, data
