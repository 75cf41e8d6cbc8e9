"""Pattern sets of 100 000 and 300 000 patterns and the streams that go with them (tests/test_scale_host.py, test_scale_gpu.py): test
infrastructure only.  Every builder is a pure function of its arguments, cached for the process, and asserts its own preconditions --
properties of the filter model (tests/filter_model.py) or of the oracle on the fixture, never of the code under test.

The dense table of these sets would be 256 x 4 x states bytes (1.6 GB / 4.9 GB): everything here goes through the HASHED oracle.

  S100, S300            wl.snort_patterns(count): 1.6 M / 4.8 M states
  text(count, n)        the C3 stream (its pool is built from the 30 000-pattern set, so the text is the same under every set) with a
                        few hundred patterns of the set under test planted verbatim, some across 2 KiB chunk boundaries, one ending
                        exactly at n and one cut off by the end
  threshold_stream(n)   per-chunk level-1 hit counts of S300 on both sides of the 1024 at which the filter kernel hands a chunk to the
                        tiled kernel (scan_common.h: kDenseHits)
  density_stream(t, n)  the C3 stream with whole patterns of C3's set planted until the oracle's share of non-zero positions is t
"""
import atexit
import contextlib
import functools
import os
import shutil
import tempfile

import numpy as np

from pfac_amd import api
from pfac_amd import workloads as wl
from tests.filter_model import prefilter_model

S100, S300, C3 = 100_000, 300_000, 30_000
CHUNK = 2048                 # input bytes of a chunk of the filter kernel (scan_common.h: kChunkTiles KiB)
DENSE_HITS = 1024            # kDenseHits: a chunk with MORE level-1 hits goes on the dense list
LIST_CODES, LIST_CODES_VETO2 = 128, 256          # codes of the filter kernel's hit list (kListCapK), of its VETO = 2 instance
BIG = (40 << 20) + 1237      # above the 32 MiB below which PFACX_KERNEL_AUTO takes the tiled kernel alone, and odd
THRESHOLD_BYTES = (33 << 20) + 517
DENSITIES = (0.005, 0.02, 0.10)

_DIR = tempfile.mkdtemp(prefix="pfac_scale_")
atexit.register(shutil.rmtree, _DIR, ignore_errors=True)


@functools.lru_cache(maxsize=None)
def patterns(count):
    return wl.snort_patterns(count)


@functools.lru_cache(maxsize=None)
def pattern_file(count, extra=()):
    """the pattern file of snort_patterns(count) followed by the `extra` patterns (a tuple of bytes)"""
    name = f"s{count}" + "".join(f"_{p.hex()}" for p in extra) + ".pat"
    return wl.write_pattern_file(os.path.join(_DIR, name), list(patterns(count)) + list(extra))


def scratch_path(name):
    return os.path.join(_DIR, name)


@functools.lru_cache(maxsize=None)
def host_handle(count):
    """a host-only handle in hashed mode: the compiled filter tables for the model (never destroyed: cached for the process)"""
    h = api.PFAC.createHostOnly()
    h.setPerfMode(api.PFAC_SPACE_DRIVEN)
    h.readPatternFromFile(pattern_file(count))
    return h


@functools.lru_cache(maxsize=None)
def _oracle(pf):
    from oracle import binding as ob
    return ob.Oracle(pf, dense=False, hashed=True)


def want(pf, data):
    """the hashed oracle's result vector (OpenMP over positions); the oracle of a pattern file is built once"""
    return _oracle(pf).match(data, hashed=True, omp=True)


def assert_same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"{what}: {bad.size} mismatches; first at {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}")


@contextlib.contextmanager
def hashed_oracle():
    """tests/stream_ref.py and flows_ref.py build `Oracle(pattern_file, hashed=False)` -- the dense table, gigabytes at this scale.  Inside
    this context that name gives the cached hashed oracle (same results: tests/test_oracle_golden.py, test_scale_host.py pin both forms)."""
    from oracle import binding as ob

    class Hashed:
        def __init__(self, pattern_file, dense=True, hashed=True):
            self._o = _oracle(pattern_file)

        def match(self, data, hashed=False, omp=False, threads=0):
            return self._o.match(data, hashed=True, omp=omp, threads=threads)

        def close(self):
            pass

    plain = ob.Oracle
    ob.Oracle = Hashed
    try:
        yield
    finally:
        ob.Oracle = plain


# ----------------------------------------------------------------------------------------------------------------- the filter model

def level1_counts(count, data, block=4 << 20):
    """level-1 hits of every whole 2 KiB chunk of `data` (chunks from offset 0) under the set's compiled tables: prefilter_model, run
    over blocks (a level-1 test reads three bytes; the model pads with zeros, so a block brings the 320 bytes behind it along)"""
    h = host_handle(count)
    chunks = data.size // CHUNK
    out = np.zeros(chunks, dtype=np.int64)
    for at in range(0, chunks * CHUNK, block):
        end = min(at + block, chunks * CHUNK)
        level1 = prefilter_model(h, data[at:min(end + 320, data.size)], veto=False)[0][:end - at]
        out[at // CHUNK:end // CHUNK] = level1.reshape(-1, CHUNK).sum(axis=1)
    return out


# ---------------------------------------------------------------------------------------------------------------------- the streams

@functools.lru_cache(maxsize=None)
def _c3_stream(n):
    data = wl.http_stream(n, wl.http_message_pool(patterns(C3)))
    data.setflags(write=False)
    return data


def plain_text(n):
    """n bytes of the C3 stream (a writable copy)"""
    return np.array(_c3_stream(n), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def text(count, n):
    data = plain_text(n)
    pats = patterns(count)
    rng = np.random.Generator(np.random.PCG64(count + 17))
    longer = [p for p in pats[C3:] if len(p) >= 8]             # patterns only this set has (the smaller sets are its first patterns)
    planted = 0
    for k in range(300):                                        # anywhere
        p = np.frombuffer(longer[int(rng.integers(0, len(longer)))], dtype=np.uint8)
        at = int(rng.integers(0, n - 4096))
        data[at:at + p.size] = p
        planted += 1
    for k in range(100):                                        # across a chunk boundary, 1 .. len - 1 bytes beyond it
        p = np.frombuffer(longer[int(rng.integers(0, len(longer)))], dtype=np.uint8)
        boundary = CHUNK * int(rng.integers(1, n // CHUNK - 1))
        at = boundary - int(rng.integers(1, p.size))
        data[at:at + p.size] = p
        planted += 1
    last = np.frombuffer(longer[7], dtype=np.uint8)             # ends exactly at n
    cut = np.frombuffer(longer[11], dtype=np.uint8)             # cut off by the end of the input in front of it: all but its last two bytes
    data[n - last.size:] = last
    data[n - last.size - (cut.size - 2):n - last.size] = cut[:-2]
    w = want(pattern_file(count), data)
    assert w[n - last.size] > 0 and np.count_nonzero(w) >= planted, (int(w[n - last.size]), int(np.count_nonzero(w)))
    across = np.flatnonzero(w)
    lengths = np.array([0] + [len(p) for p in pats], dtype=np.int64)
    assert np.count_nonzero(across // CHUNK != (across + lengths[w[across]] - 1) // CHUNK) >= 80       # matches that cross a chunk boundary
    data.setflags(write=False)
    return data


def check_text_hits(count, data):
    """the precondition of the S100 text: every chunk has more level-1 hits than the hit list has codes (128: several list rounds, with
    leftover candidates carried between them), and at least half of the chunks more than the VETO = 2 instance's 256"""
    hits = level1_counts(count, data)
    assert hits.min() > LIST_CODES and np.median(hits) > LIST_CODES_VETO2, (int(hits.min()), float(np.median(hits)))
    assert np.count_nonzero(hits > LIST_CODES_VETO2) * 2 >= hits.size
    return hits


def _chunk_hits(data, k):
    lo = k * CHUNK
    return int(prefilter_model(host_handle(S300), data[lo:lo + CHUNK + 320], veto=False)[0][:CHUNK].sum())


def _tune(data, k, target, rng, tries=4000):
    """single bytes of chunk k replaced (URL-safe characters, from the chunk's third byte on: no other chunk's 3-grams change) until the
    model counts `target` level-1 hits in it"""
    have = _chunk_hits(data, k)
    for _ in range(tries):
        if have == target:
            return
        at = k * CHUNK + int(rng.integers(2, CHUNK))
        old = data[at]
        data[at] = wl.URL_SAFE[int(rng.integers(0, wl.URL_SAFE.size))]
        now = _chunk_hits(data, k)
        if abs(now - target) < abs(have - target):
            have = now
        else:
            data[at] = old
    raise AssertionError(f"chunk {k}: {have} level-1 hits, could not reach {target}")


@functools.lru_cache(maxsize=None)
def threshold_stream(n=THRESHOLD_BYTES):
    """(data, level-1 hits per whole chunk under S300).  Plain C3 text has a median of ~957 hits per chunk under S300; in two chunks of
    three a stretch of 0 .. 1600 bytes of pattern PREFIX records (the first three bytes of a pattern -- what level 1 tests -- one in
    eleven the whole pattern, 0 .. 1 other bytes: two positions in three pass level 1, against 47 % of the text) at a random place
    inside the chunk lifts the count by up to ~250.  Two chunks are then
    tuned byte by byte to exactly 1024 and 1025.  The last 16 KiB stay plain and at or below the threshold."""
    rng = np.random.Generator(np.random.PCG64(1024))
    data = plain_text(n)
    pats = patterns(S300)
    longer = [p for p in pats if len(p) >= 8]
    chunks = n // CHUNK
    recs = []
    for k in range(60000):
        q = longer[int(rng.integers(0, len(longer)))]
        recs.append(np.frombuffer(q if k % 11 == 0 else q[:3], dtype=np.uint8))
        recs.append(wl.ALNUM[rng.integers(0, wl.ALNUM.size, int(rng.integers(0, 2)))])
    pool = np.concatenate(recs)
    for k in range(chunks - 8):
        if k % 3 == 2:
            continue
        ln = int(rng.integers(0, 1601))
        src = int(rng.integers(0, pool.size - ln))
        at = k * CHUNK + int(rng.integers(0, CHUNK - ln))
        data[at:at + ln] = pool[src:src + ln]
    hits = level1_counts(S300, data)
    near = np.argsort(np.abs(hits[:chunks - 8] - DENSE_HITS), kind="stable")
    exact = [int(near[0]), int(near[1])]
    for k, target in zip(exact, (DENSE_HITS, DENSE_HITS + 1)):
        _tune(data, k, target, rng)
        hits[k] = _chunk_hits(data, k)           # (no other chunk's count has changed)
    check_threshold(hits)
    data.setflags(write=False)
    return data, hits


def check_threshold(hits):
    dense = hits > DENSE_HITS
    assert dense.mean() >= 0.10 and (~dense).mean() >= 0.10, float(dense.mean())
    assert np.count_nonzero(dense[1:] != dense[:-1]) >= 200
    assert np.count_nonzero((hits > DENSE_HITS) & (hits <= DENSE_HITS + 8)) >= 50
    assert np.count_nonzero((hits <= DENSE_HITS) & (hits >= DENSE_HITS - 8)) >= 50
    assert np.any(hits == DENSE_HITS) and np.any(hits == DENSE_HITS + 1)
    assert not dense[-8:].any()              # the end of the input (walked with bounds, not in chunks) lies in text below the threshold


@functools.lru_cache(maxsize=None)
def density_stream(target, n=BIG):
    """(data, oracle result, achieved density) over C3's 30 000 patterns: whole patterns planted one behind the other, 1 / target bytes
    apart on average (patterns short enough to fit), the spacing corrected by what the oracle counts until the share of non-zero
    positions lies within [0.8, 1.25] x target"""
    pf = pattern_file(C3)
    pats = patterns(C3)
    period = 1.0 / target
    fit = [p for p in pats if len(p) <= max(4, int(period * 0.6))]
    by_len = {}
    for p in fit:
        by_len.setdefault(len(p), []).append(np.frombuffer(p, dtype=np.uint8))
    sizes = np.array(sorted(by_len))
    weight = np.array([len(by_len[s]) for s in sizes], dtype=np.float64)
    weight /= weight.sum()
    base = _c3_stream(n)
    for attempt in range(6):
        rng = np.random.Generator(np.random.PCG64(int(target * 1e6)))
        count = int(n / period) + 16
        ln = rng.choice(sizes, size=count, p=weight)
        gap = rng.integers(0, max(1, int(2 * (period - float((sizes * weight).sum()))) + 1), size=count)
        at = np.concatenate([[0], np.cumsum(ln + gap)[:-1]])
        keep = at + ln <= n
        at, ln = at[keep], ln[keep]
        data = np.array(base, dtype=np.uint8)
        for s in sizes:
            mine = at[ln == s]
            table = np.stack(by_len[int(s)])
            data[mine[:, None] + np.arange(int(s))] = table[rng.integers(0, table.shape[0], mine.size)]
        w = want(pf, data)
        density = np.count_nonzero(w) / n
        if 0.95 * target <= density <= 1.05 * target:
            break
        period *= density / target
    assert 0.8 * target <= density <= 1.25 * target, (target, density)
    data.setflags(write=False)
    return data, w, density


ONE_BYTE = (b"e", b"/", b"7", b"Z", b"-", b"q", b"%", b"A")      # URL-safe characters: each is about one byte in 75 of the text


@functools.lru_cache(maxsize=None)
def one_byte_set(k, n=BIG):
    """(pattern file of C3's 30 000 patterns + k one-byte patterns, plain C3 stream, oracle result)"""
    pf = pattern_file(C3, ONE_BYTE[:k])
    data = _c3_stream(n)
    for p in ONE_BYTE[:k]:
        assert np.count_nonzero(data == p[0]) > n // 200
    return pf, data, want(pf, data)
