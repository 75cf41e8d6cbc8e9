"""Fixtures for the edges of pfac_scan_filter (tests/test_filter_edges_host.py, test_filter_edges_gpu.py) and a model of its launch
plan: test infrastructure only.  Every builder is seeded, a pure function of its arguments and cached for the process.  The generators
walks(), plant_specs() and fuzz_case() and the sets "q" and "qq" are those of tests/tiled_edges.py.

  plan(in_off, n, max_len, reduce)  what scan() / reduceScan() (scan_module.hip: headPositions, filterLength) and launchFilter
                            (scan_filter.hip) make of a PFACX_KERNEL_FILTER call whose input pointer lies in_off bytes behind a 16-byte
                            address: head, main_len, chunks, blocks, parts
  expected_stats(...)       what PFACX_getScanStats reports of that launch: level1Hits is the sum of `listed` in scan_filter.hip -- the level-1
                            hits of the chunks of [head, head + main_len) that do NOT go on the dense list (a dense chunk lists nothing, the
                            bounded walks of the ends are not filtered at all); denseChunks the chunks with more than PFAC_DENSE_HITS hits
  SETS                      "q" (every chunk dense), "qq" (sparse; a tail table in LDS and the exact 2-byte bitmap: VETO = 1, HAS_SHORT),
                            "long" ("qq" without the patterns of fewer than three bytes: VETO = 1 without HAS_SHORT) and "min3" (six 3-byte
                            patterns: maxPatternLen 3, the smallest margin; no tail table: the plain window walker)
  seam(...)                 A: one input per (set, in_off, k, d, v): n = head + 2048 k + margin + d, plants around the end of the main part
  handout(...)              B: one plant per chunk, at a chunk-specific offset, with a cycling pattern
  boundary_walks(...)       B: tiled_edges.walks() across the 2 KiB chunk boundaries of a call at this input offset
  dense_case(...)           C: handout() with `q` runs over chosen chunks
  hit_chunks(...)           D: chunks with exactly HIT_TARGETS level-1 hits among quiet filler
  walk_chunks()             D: chunks with exactly WALK_COUNTS whole patterns of one length

Two fillers: tiled_edges' `0123`, of whose 64 3-grams three (`110`, `112`, `113`) pass the full-result kernel's level 1 under "qq" -- about
a position in twenty, candidates that the level-4 test drops --, and QUIET (`023`), which passes level 1 nowhere under "qq", "long" and "min3",
for the chunks whose hit counts are set to the unit."""
import functools
import os

import numpy as np

from pfac_amd import api
from pfac_amd import workloads as wl
from tests import tiled_edges as te
from tests.filter_model import level1_model, reduce_filter_model

# The constants of the launch plan and of the per-wave buffers, each named after its source.  tests/test_filter_edges_host.py reads the sources'
# defaults and compares: a retune fails there instead of moving the edges away from the sizes below.
SOURCES = {                                      # name: (file under pfac_amd/csrc, regular expression with the value as group 1)
    "kChunkTiles": ("pfac_context.h", r"constexpr int kChunkTiles = (\d+);"),
    "PFAC_WORK_PARTS": ("pfac_context.h", r"#define PFAC_WORK_PARTS (\d+)"),
    "PFAC_BLOCK_THREADS": ("scan_common.h", r"#define PFAC_BLOCK_THREADS (\d+)"),
    "PFAC_QUEUE_CAP": ("scan_common.h", r"#define PFAC_QUEUE_CAP (\d+)"),
    "kDenseStage": ("scan_common.h", r"constexpr uint32_t kDenseStage = (\d+);"),
    "PFAC_DENSE_HITS": ("scan_common.h", r"#define PFAC_DENSE_HITS (\d+)"),
    "kWalkHalo": ("scan_common.h", r"constexpr uint32_t kWalkHalo = (\d+);"),
    "PFAC_LIST_CAP": ("scan_filter.hip", r"#define PFAC_LIST_CAP (\d+)"),
    "PFAC_REDUCE_PARTS": ("scan_filter.hip", r"#define PFAC_REDUCE_PARTS (\d+)"),
    "PFAC_FRONT_LOG2": ("scan_filter.hip", r"#define PFAC_FRONT_LOG2 (-?\d+)"),
    "PFAC_WRITERS": ("scan_filter.hip", r"#define PFAC_WRITERS (\d+)"),
    "PFAC_SPAN_LOG2": ("scan_filter.hip", r"#define PFAC_SPAN_LOG2 (\d+)"),
    "PFAC_APPEND_MIN": ("scan_filter.hip", r"#define PFAC_APPEND_MIN (\d+)"),
    "PFAC_MERGE_MIN": ("scan_filter.hip", r"#define PFAC_MERGE_MIN (\d+)"),
    "kReduceCap": ("scan_filter.hip", r"constexpr uint32_t kReduceCap = (\d+);"),
}
kChunkTiles, PFAC_WORK_PARTS, PFAC_BLOCK_THREADS, PFAC_QUEUE_CAP, kDenseStage, PFAC_DENSE_HITS, kWalkHalo = 2, 2, 1024, 64, 8, 1024, 128
PFAC_LIST_CAP, PFAC_REDUCE_PARTS, PFAC_FRONT_LOG2, PFAC_WRITERS, PFAC_SPAN_LOG2, PFAC_APPEND_MIN, PFAC_MERGE_MIN, kReduceCap = 128, 32, 4, 3, 2, 48, 48, 16

CHUNK = kChunkTiles * 1024                       # kChunkBytesHost
kSpanChunks = 1 << PFAC_SPAN_LOG2                # chunks a writer wave claims at a time (full result)
GRANULE = kSpanChunks << PFAC_FRONT_LOG2         # chunks dealt to one part before the next part's turn (full result)
BATCH = 1 << PFAC_FRONT_LOG2                     # kTicketBatch: chunks a scanning wave claims per atomic (compacted output: a piece is a chunk)
SCANNERS_FULL = PFAC_BLOCK_THREADS // 64 - PFAC_WRITERS      # FilterLds::kScanners
SCANNERS_REDUCE = PFAC_BLOCK_THREADS // 64
RESIDENT = 256                                   # launchFilter: multiProcessorCount * blocks per CU -- an MI355X has 256 CUs, a block takes a CU's whole LDS
Q = te.Q
QUIET = np.frombuffer(b"023", dtype=np.uint8)

LONG = [p for p in te.SETS["qq"] if len(p) >= 3]
MIN3 = [te.LONG_A[:3], te.P600[:3], te.P600[597:], te.P600[598:] + b"A", te.SHORT[0], b"qqq"]      # (the fourth: two bytes of a P600 that ends with the input + one behind it)
SETS = {"q": te.SETS["q"], "qq": te.SETS["qq"], "long": LONG, "min3": MIN3}
MAX_LEN = {name: max(len(p) for p in pats) for name, pats in SETS.items()}


@functools.lru_cache(maxsize=None)
def pattern_file(name):
    return wl.write_pattern_file(os.path.join(te._DIR, f"filter_edges_{name}.pat"), SETS[name])


@functools.lru_cache(maxsize=None)
def host_handle(name):
    """a host-only handle: the compiled filter tables for the model (never destroyed: cached for the process)"""
    h = api.PFAC.createHostOnly()
    h.readPatternFromFile(pattern_file(name))
    return h


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle import binding as ob
    return ob.Oracle(pattern_file(name), hashed=False)


def want(data, name):
    """the oracle's result vector for exactly these bytes under the set `name`"""
    return _oracle(name).match(data)


# ------------------------------------------------------------------------------------------------------------------- the launch plan

def head16(in_off):
    """positions in front of the first 16-byte aligned input byte (headPositions, for an input longer than that)"""
    return (16 - in_off % 16) % 16


def margin(max_len):
    """filterLength: bytes of input that stay behind the last chunk of the main part"""
    return max_len + 64 + kWalkHalo


def plan(in_off, n, max_len, reduce, resident=RESIDENT):
    """(head, main_len, chunks, blocks, parts) of a PFACX_KERNEL_FILTER call: positions [0, head) and [head + main_len, n) are walked with
    bounds by the same launch (ScanArgs::endsIn); chunks == 0: no filter launch, the tiled kernel takes the call"""
    head = min(head16(in_off), n)
    safe_end = n - margin(max_len) if n > margin(max_len) else 0
    main_len = (safe_end - head) // CHUNK * CHUNK if safe_end > head else 0
    chunks = main_len // CHUNK
    scanners = SCANNERS_REDUCE if reduce else SCANNERS_FULL
    blocks = min(-(-chunks // scanners), resident)
    parts = min(blocks, PFAC_REDUCE_PARTS if reduce else PFAC_WORK_PARTS)
    return head, main_len, chunks, blocks, parts


def size_for(in_off, chunks, max_len, d=0):
    """the smallest n whose main part has `chunks` chunks, plus d (0 <= d < CHUNK keeps the count; d = -1 loses the last chunk)"""
    return head16(in_off) + CHUNK * chunks + margin(max_len) + d


def chunk_hits(h, max_len, data, in_off, reduce):
    """level-1 hits of every chunk of the main part, in the launch's own grid: the full-result kernel's 3-gram test, or the
    compacted-output kernel's (gram1)"""
    head, main_len, chunks, _, _ = plan(in_off, data.size, max_len, reduce)
    if chunks == 0:
        return np.zeros(0, dtype=np.int64)
    piece = data[head:head + main_len + 2]                 # (the margin: the bytes behind the last chunk are the input's)
    hits = reduce_filter_model(h, piece)[0] if reduce else level1_model(h, piece)
    return hits[:main_len].reshape(chunks, CHUNK).sum(axis=1)


def expected_stats(h, max_len, data, in_off, reduce):
    """(level1Hits, denseChunks) of the launch (see the module's docstring; the compacted-output kernel has no dense list)"""
    hits = chunk_hits(h, max_len, data, in_off, reduce)
    dense = np.zeros(hits.size, dtype=bool) if reduce else hits > PFAC_DENSE_HITS
    return int(hits[~dense].sum()), int(dense.sum())


def stats_of(name, data, in_off, reduce):
    return expected_stats(host_handle(name), MAX_LEN[name], data, in_off, reduce)


def _put(data, at, p):
    """p at `at`, cut off by the end of the input"""
    p = np.frombuffer(p, dtype=np.uint8)[:max(0, data.size - at)]
    assert at >= 0
    data[at:at + p.size] = p


def _quiet(rng, n):
    return QUIET[rng.integers(0, QUIET.size, n)].copy()


# ------------------------------------------------------------------------------------------------------------------------------- A

A_SETS = ("qq", "long", "min3")
A_K = (1, 2)
A_D = (-1, 0, 1, CHUNK // 2, CHUNK - 1)          # d = -1 at k = 1: the last size the tiled kernel takes alone; CHUNK - 1: the longest tail
A_VARIANTS = 4
A_AROUND = dict(front=Q, behind=b"ABCDEFGH")     # what lies around the input in device memory
_SPRINKLE = [te.SHORT[0], te.SHORT[3], te.LONG_A[:17], te.SHORT[6], b"qqq", te.LONG_B[:40]]
SEAM_CLEAR = 160                                 # bytes behind main_end that belong to the plant at the seam


@functools.lru_cache(maxsize=None)
def seam(name, in_off, k, d, v):
    """data of n = head + CHUNK k + margin + d bytes (quiet filler).  With main_end = head + main_len (k chunks; k - 1 for d = -1; for the one
    size without a filter launch the end that one byte more would give):
      v = 0, 1, 2: LONG_A from main_end - 1, main_end, main_end - 60 (its last byte is the last of the last chunk); v = 3: P600 from main_end - 450
      (it starts in the last chunk and ends in the tail);
      LONG_B[:40] from position 0 (v = 0, 3), from head - 1 (v = 1) and from the first aligned byte (v = 2);
      the end of P600 -- all of it where the tail has the room -- ending exactly at n: the bytes behind the input would complete TAIL_CUT (under
      "min3": the pattern of P600's last two bytes + `A`);
      short patterns sprinkled over the main part and over the tail."""
    max_len = MAX_LEN[name]
    n = size_for(in_off, k, max_len, d)
    head, main_len, chunks, _, _ = plan(in_off, n, max_len, False)
    main_end = head + (main_len if chunks else CHUNK * k)
    rng = np.random.Generator(np.random.PCG64(9000 + 1000 * in_off + 100 * k + 10 * A_D.index(d) + v))
    data = _quiet(rng, n)
    tail_piece = min(len(te.P600), n - (main_end + SEAM_CLEAR))
    for j, at in enumerate(range(head + 70, main_end - 520, 157)):
        _put(data, at, _SPRINKLE[j % len(_SPRINKLE)])
    for j, at in enumerate(range(main_end + SEAM_CLEAR + 10, n - max(tail_piece, 0) - 60, 157)):
        _put(data, at, _SPRINKLE[(j + 2) % len(_SPRINKLE)])
    if v < 3:
        _put(data, main_end - (1, 0, 60)[v], te.LONG_A)
    else:
        _put(data, main_end - 450, te.P600)
    _put(data, (0, max(head - 1, 0), head, 0)[v], te.LONG_B[:40])
    if tail_piece >= 3:
        _put(data, n - tail_piece, te.P600[len(te.P600) - tail_piece:])
    data.setflags(write=False)
    return data


# ------------------------------------------------------------------------------------------------------------------------------- B

IN_OFFS = (0, 5, 15)
FULL_CHUNKS = tuple(sorted(set(
    list(range(1, kSpanChunks + 2)) +                                      # one chunk ... one span and a chunk: the partial last span
    [SCANNERS_FULL - 1, SCANNERS_FULL, SCANNERS_FULL + 1] +                # the grid grows from one block to two: parts = min(gridDim, kParts)
    [2 * SCANNERS_FULL, 2 * SCANNERS_FULL + 1] +                           # ... to three: the third block serves part 0 again
    [GRANULE - 1, GRANULE, GRANULE + 1] +                                  # chunk GRANULE is the first that part 1 ever gets
    [GRANULE + kSpanChunks, GRANULE + kSpanChunks + 1] +
    [2 * GRANULE - 1, 2 * GRANULE + 1, 3 * GRANULE + 1])))
REDUCE_CHUNKS = tuple(sorted({1, BATCH - 1, BATCH, BATCH + 1, 2 * BATCH, 2 * BATCH + 1,
                              PFAC_REDUCE_PARTS * BATCH - 1, PFAC_REDUCE_PARTS * BATCH, PFAC_REDUCE_PARTS * BATCH + 1,
                              (PFAC_REDUCE_PARTS + 1) * BATCH, (PFAC_REDUCE_PARTS + 1) * BATCH + 1}))
DENSE_SET_CHUNKS = (1, kSpanChunks + 1, SCANNERS_FULL, SCANNERS_FULL + 1, GRANULE, GRANULE + 1, 2 * GRANULE + 1)     # the "q" set: a subset of FULL_CHUNKS
_HANDOUT = te.SHORT + te.PREFIXES                # 13 patterns of 3 .. 40 bytes, all of them in "q", "qq" and "long"
HANDOUT_TAIL = 333


def handout_plants(in_off, chunks):
    """[(position, pattern)]: one per chunk, at an offset and with a pattern that depend on the chunk's number"""
    head = head16(in_off)
    return [(head + CHUNK * c + (389 * c) % (CHUNK - 64), _HANDOUT[c % len(_HANDOUT)]) for c in range(chunks)]


@functools.lru_cache(maxsize=None)
def handout(in_off, chunks, filler="0123"):
    """data whose main part has exactly `chunks` chunks under a set of maxPatternLen 600 (HANDOUT_TAIL bytes more than the smallest such
    input), handout_plants() in it, LONG_B in the tail: a chunk that no wave took lacks its match (full result: holds the poison), a chunk taken
    twice has its pair twice"""
    n = size_for(in_off, chunks, 600, HANDOUT_TAIL)
    rng = np.random.Generator(np.random.PCG64(9100 + 16 * chunks + in_off))
    data = te._filler(rng, n) if filler == "0123" else _quiet(rng, n)
    for at, p in handout_plants(in_off, chunks):
        _put(data, at, p)
    _put(data, n - 300, te.LONG_B)
    data.setflags(write=False)
    return data


WALK_BOUNDARIES = len(te.plant_specs()) + 5      # a boundary per plant, and a few to spare (a plant that would begin in front of the input takes the next)
WALKS_N = CHUNK * WALK_BOUNDARIES + 1300 + 777


def boundary_walks(in_off):
    """tiled_edges.walks() with its groups on the chunks of a filter launch: chunk k of a call at this input offset begins at head + CHUNK k,
    so the call's pointer lies (CHUNK - head) % CHUNK bytes behind a chunk boundary -- walks()' `in_off`, which for the tiled kernel (groups cut
    at 16-byte addresses from the one in FRONT of the pointer) is the offset itself"""
    return te.walks(CHUNK, (CHUNK - head16(in_off)) % CHUNK, WALKS_N)


# ------------------------------------------------------------------------------------------------------------------------------- C

_SIX = kSpanChunks + 2
DENSE_CASES = {                                  # name: (chunks, the chunks under a `q` run, a run across main_end)
    "first": (_SIX, (0,), False),
    "last": (_SIX, (_SIX - 1,), False),
    "partial-span": (2 * kSpanChunks - 1, tuple(range(kSpanChunks, 2 * kSpanChunks - 1)), False),
    "part-1": (GRANULE + 2, (GRANULE,), False),
    "stage": (SCANNERS_FULL - 1, tuple(range(1, 1 + kDenseStage)), False),
    "stage+1": (SCANNERS_FULL - 1, tuple(range(1, 2 + kDenseStage)), False),
    "all": (SCANNERS_FULL + 1, tuple(range(SCANNERS_FULL + 1)), False),
    "across-the-end": (_SIX, (), True),
}
CROSS = (1500, 500)                              # the run across main_end: this many bytes in front of it (the last chunk is dense) and behind it


@functools.lru_cache(maxsize=None)
def dense_case(in_off, case):
    chunks, dense, cross = DENSE_CASES[case]
    data = handout(in_off, chunks).copy()
    head = head16(in_off)
    for c in dense:
        data[head + CHUNK * c:head + CHUNK * (c + 1)] = Q
    if cross:
        main_end = head + CHUNK * chunks
        data[main_end - CROSS[0]:main_end + CROSS[1]] = Q
    data.setflags(write=False)
    return data


def dense_chunks_of(case):
    chunks, dense, cross = DENSE_CASES[case]
    return tuple(sorted(set(dense) | ({chunks - 1} if cross else set())))


# ------------------------------------------------------------------------------------------------------------------------------- D

HIT_TARGETS = (PFAC_LIST_CAP - 1, PFAC_LIST_CAP, PFAC_LIST_CAP + 1, 2 * PFAC_LIST_CAP - 1, 2 * PFAC_LIST_CAP + 1, PFAC_DENSE_HITS - 1, PFAC_DENSE_HITS)
RUN_BYTE = {"qq": Q, "long": ord("&")}           # a run of it passes level 1 at every position (under "long": a collision in the 8192-bit bitmap; no pattern holds the byte)
WALK_COUNTS = (1, kReduceCap - 1, kReduceCap, kReduceCap + 1, PFAC_QUEUE_CAP - 1, PFAC_QUEUE_CAP, PFAC_QUEUE_CAP + 1, 2 * PFAC_QUEUE_CAP + 1, 300)
WALK_PATTERN = te.SHORT[2]                       # 5 bytes


def _fit_chunk(count, data, lo, target, byte):
    """`byte` over the quiet filler of data[lo:lo + CHUNK] until count() == target: a run to begin with, then one byte at a time against the model
    (a byte that would overshoot stays filler)"""
    at = lo + 8
    bulk = max(0, target - 16)
    data[at:at + bulk] = byte
    at += bulk
    have = count()
    assert have <= target, (have, target)
    while have < target:
        assert at < lo + CHUNK - 8, f"{have} hits, want {target}"
        old = data[at]
        data[at] = byte
        now = count()
        if have <= now <= target:
            have = now
        else:
            data[at] = old
        at += 1


@functools.lru_cache(maxsize=None)
def hit_chunks(name, reduce=False):
    """(data, {target: chunk}): aligned input, quiet filler, every second chunk with exactly HIT_TARGETS level-1 hits under the set `name`
    -- of the full-result kernel's level 1, or (reduce) of the compacted-output kernel's"""
    chunks = 2 * len(HIT_TARGETS) + 1
    n = size_for(0, chunks, MAX_LEN[name], 100)
    data = _quiet(np.random.Generator(np.random.PCG64(9200)), n)
    h = host_handle(name)
    at = {}
    for k, target in enumerate(HIT_TARGETS):
        c = 2 * k + 1
        lo = CHUNK * c

        def count():
            piece = data[lo:lo + CHUNK + 2]
            return int((reduce_filter_model(h, piece)[0] if reduce else level1_model(h, piece))[:CHUNK].sum())

        _fit_chunk(count, data, lo, target, RUN_BYTE[name])
        at[target] = c
    data.setflags(write=False)
    return data, at


@functools.lru_cache(maxsize=None)
def walk_chunks():
    """(data, {count: chunk}): aligned input, quiet filler, every second chunk with `count` copies of one 5-byte pattern, six bytes apart: walks
    that start together and end together"""
    chunks = 2 * len(WALK_COUNTS) + 1
    n = size_for(0, chunks, 600, 100)
    data = _quiet(np.random.Generator(np.random.PCG64(9300)), n)
    at = {}
    for k, count in enumerate(WALK_COUNTS):
        c = 2 * k + 1
        for j in range(count):
            _put(data, CHUNK * c + 4 + 6 * j, WALK_PATTERN)
        at[count] = c
    data.setflags(write=False)
    return data, at


# ------------------------------------------------------------------------------------------------------------------------------- E

FUZZ_MIN_CHUNKS = 5


def fuzz_input(workdir, seed):
    """(pattern file, data) of tiled_edges.fuzz_case, the data repeated until the main part of a call has FUZZ_MIN_CHUNKS chunks at least"""
    pf, data = te.fuzz_case(workdir, seed)
    need = size_for(15, FUZZ_MIN_CHUNKS, 48, 0)
    if data.size < need:
        data = np.tile(data, -(-need // data.size))
    return pf, data
