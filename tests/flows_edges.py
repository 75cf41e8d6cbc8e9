"""Cases for the edges of the flows seam and merge kernels (pfac_amd/csrc/scan_flows.hip, seamBlock of scan_passes.h, pfac_stream_seam of
scan_stream.hip; tests/test_flows_edges_host.py, test_flows_edges_gpu.py): test infrastructure only, no GPU code and no call of the library.
Every builder is seeded, a pure function of its arguments and cached for the process.

A case is a Case(patterns, nocase, F, steps, name, M, info): pattern-file bytes, whether the handle reads them with PFACX_READ_NOCASE, the
number of flows, and the schedule as tests/flows_ref.py writes it (Batch and End steps, so flows_ref.run and the feeders of
tests/test_flows_gpu.py take it unchanged: model(case)).  `info` keeps what the expected answers were made from, for check_edges() and the
oracle comparison of the host test.

Pattern sets, one per M = maxPatternLen (pattern_list): `a`, `ab`, L = `a` + M - 1 seeded bytes of b..y (non-periodic: its first byte occurs
nowhere else in it), and for M >= 3 S = `b` + M - 2 seeded bytes.  The caseless form has every other letter in upper case.

The model.  The flows' streams lie one behind the other in ONE buffer with M - 1 bytes 0x00 (in no pattern) between them, longest_at()
runs once over it and the list is cut per flow.  A piece call reports the positions [R, max(R, T - (M - 1))) of its flow (the finality
rule of tests/stream_ref.py), so the expected arrays of a batch are ranges of that one list, gathered in piece order; check_edges()
compares them flow by flow with stream_ref.split over the flow's own list (every flow of a case up to 1024 flows, a sample that holds
the block and trip edges beyond).

Families (what each pins is listed in DESIGN.md 5e "edges under test")
  A  piece_counts(P)      P = F flows of M = 4, three steps: every flow once, every flow in a permutation, the flush in another
  B  block_positions(w)   3 x 256 + 1 pieces of M = 4; where the pairs sit relative to a block of 256 pieces (B_WHICH)
  C  seam_shapes(span)    28 flows = carry state x second-piece length for M - 1 = span in C_SPANS, L placed across the cuts
  D  dense_seams(span, z) 5 flows whose every carried position is a seam pair, M - 1 = span in D_SPANS
"""
import collections
import functools

import numpy as np

from pfac_amd import api
from tests import flows_ref as fr
from tests import stream_ref as sr

PIECE_BLOCK = api.PFACX_FLOWS_PIECE_BLOCK        # scan_flows.hip: kPieceBlock
WAVE_SEAM_MAX = api.PFACX_FLOWS_WAVE_SEAM_MAX    # kWaveSeamMax
WAVE_SEAM_PIECES = api.PFACX_FLOWS_WAVE_SEAM_PIECES      # kWaveSeamWaves
SEAM_BLOCK = api.PFACX_STREAM_SEAM_BLOCK         # kSeamBlock (scan_flows.hip and scan_stream.hip)
SEAM_LDS = api.PFACX_STREAM_SEAM_LDS             # pfac::kStreamSeamLdsBytes
SUMS_TRIP = PIECE_BLOCK * PIECE_BLOCK            # pieces behind one trip of pfac_flows_sums: kPieceBlock block sums of kPieceBlock pieces

A_COUNTS = (1, WAVE_SEAM_PIECES - 1, WAVE_SEAM_PIECES, WAVE_SEAM_PIECES + 1, PIECE_BLOCK - 1, PIECE_BLOCK, PIECE_BLOCK + 1,
            2 * PIECE_BLOCK - 1, 2 * PIECE_BLOCK, 2 * PIECE_BLOCK + 1, SUMS_TRIP - 1, SUMS_TRIP, SUMS_TRIP + 1, 2 * SUMS_TRIP + 1)
A_HOST_MAX = 2 * PIECE_BLOCK + 1                 # the largest case of A that the host test also runs through the host calls
A_M = 4
LENS = (0, 1, 2, 3, 4, 5, 9)                     # piece lengths of A and B: empty, below, at and above M - 1 = 3
B_PIECES = 3 * PIECE_BLOCK + 1
B_WHICH = ("two-at-the-block-edge", "empty-block", "short-block", "last-piece-only", "all-a", "empty-runs")
C_SPANS = (1, 2, WAVE_SEAM_MAX - 1, WAVE_SEAM_MAX, WAVE_SEAM_MAX + 1, 127, 128, 129, SEAM_BLOCK - 1, SEAM_BLOCK, SEAM_BLOCK + 1,
           2 * SEAM_BLOCK + 1, SEAM_LDS // 2, SEAM_LDS // 2 + 1)
C_NOCASE_SPANS = (WAVE_SEAM_MAX, WAVE_SEAM_MAX + 1, SEAM_LDS // 2 + 1)
C_FLOWS = 28
D_SPANS = (WAVE_SEAM_MAX, 200, 1500)             # a full ballot; more than one round of the lane loop of pfac_flows_first; two trips of seamBlock
D_FLOWS = 5
SEPARATOR = 0x00

Case = collections.namedtuple("Case", "patterns nocase F steps name M info")
Info = collections.namedtuple("Info", "buffer start length sizes pos ids orders")
# buffer: the streams with their separators; start[f], length[f]: flow f's stream in it; sizes[f, k]: flow f's k-th piece; pos, ids: the
# model's list over `buffer`; orders: per step the flows it names (a batch: of piece column k = its index among the batches)


# ---------------------------------------------------------------------------------------------------------------------- pattern sets

def _seeded(M, salt, n):
    rng = np.random.Generator(np.random.PCG64(7000 + 2 * M + salt))
    return bytes(rng.integers(ord("b"), ord("y") + 1, n, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def pattern_list(M):
    """[`a`, `ab`, L, S] (ids 1..4; no S below M = 3).  L's second byte is never `b`, so `ab` is no prefix of L"""
    assert M >= 2
    body = _seeded(M, 0, M - 1)
    long_ = b"a" + (b"c" if body[:1] == b"b" else body[:1]) + body[1:]
    pats = [b"a", b"ab", long_]
    if M >= 3:
        pats.append(b"b" + _seeded(M, 1, M - 2))
    assert len(long_) == M and long_.count(b"a") == 1 and (M < 3 or not long_.startswith(pats[3])) and len(set(pats)) == len(pats)
    assert all(b"\n" not in p and bytes([SEPARATOR]) not in p and b"z" not in p for p in pats)
    return pats


def _mixed(p):
    return bytes(c - 32 if i % 2 else c for i, c in enumerate(p))        # (all letters: every other one in upper case)


def pattern_set(M, nocase=False):
    """the pattern-file bytes of M's set; nocase: in mixed case, for PFACX_READ_NOCASE"""
    return b"".join((_mixed(p) if nocase else p) + b"\n" for p in pattern_list(M))


def parse_patterns(raw):
    return raw.split(b"\n")[:-1]


def fold_array(a):
    a = np.asarray(a, dtype=np.uint8)
    return np.where((a >= 0x41) & (a <= 0x5A), a + 32, a).astype(np.uint8)


# --------------------------------------------------------------------------------------------------------------------------- matcher

def longest_at(patterns, data, nocase=False):
    """for every position of `data` the id (line number from 1) of the longest pattern that starts there, 0: none.  One- and two-byte
    patterns by numpy, longer ones by bytes.find from occurrence to occurrence; a caseless set matches the ASCII fold of both sides"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    if nocase:
        data, patterns = fold_array(data), [bytes(p).lower() for p in patterns]
    out = np.zeros(data.size, dtype=np.int32)
    raw = data.tobytes()
    for k in sorted(range(len(patterns)), key=lambda k: len(patterns[k])):         # the longer pattern overwrites the shorter
        p = patterns[k]
        if len(p) == 1:
            out[data == p[0]] = k + 1
        elif len(p) == 2:
            out[:-1][(data[:-1] == p[0]) & (data[1:] == p[1])] = k + 1
        else:
            at = raw.find(p)
            while at >= 0:
                out[at] = k + 1
                at = raw.find(p, at + 1)
    return out


# ----------------------------------------------------------------------------------------------------------------------- the builder

def _ranges(starts, lens):
    """the indices starts[0] .. starts[0] + lens[0] - 1, starts[1] .., one range behind the other"""
    starts, lens = np.asarray(starts, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    total = int(lens.sum())
    if total == 0:
        return np.zeros(0, dtype=np.int64)
    before = np.cumsum(lens) - lens
    return np.repeat(starts - before, lens) + np.arange(total, dtype=np.int64)


def _first(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def _build(name, M, nocase, flat, sizes, schedule):
    """flat: the flows' streams one behind the other; sizes[F, K]: how each is cut; schedule: ("batch", order) feeds the next piece column
    to the flows of `order` (a flow left out of a batch has an empty piece in that column), ("flush", order) ends them"""
    flat = np.ascontiguousarray(flat, dtype=np.uint8)
    sizes = np.asarray(sizes, dtype=np.int64)
    F, span = sizes.shape[0], M - 1
    length = sizes.sum(axis=1)
    assert int(length.sum()) == flat.size
    plain = np.concatenate([[0], np.cumsum(length)])[:-1]              # where flow f's stream starts in `flat`
    start = plain + np.arange(F, dtype=np.int64) * span                # ... and in the buffer with the separators
    buffer = np.full(flat.size + F * span, SEPARATOR, dtype=np.uint8)
    buffer[_ranges(start, length)] = flat
    full = longest_at(pattern_list(M), buffer, nocase)
    pos = np.flatnonzero(full).astype(np.int64)
    ids = full[pos].astype(np.int32)

    off = np.cumsum(sizes, axis=1) - sizes                             # the stream offset of every piece
    steps, orders, column, R = [], [], 0, np.zeros(F, dtype=np.int64)
    for kind, order in schedule:
        order = np.asarray(order, dtype=np.int64)
        orders.append(order)
        if kind == "batch":
            lens = sizes[:, column]
            named = np.zeros(F, dtype=bool)
            named[order] = True
            assert order.size == np.count_nonzero(named) and not lens[~named].any(), "a flow named twice, or left out with bytes to feed"
            R2 = np.where(lens > 0, np.maximum(R, off[:, column] + lens - span), R)
            lo, hi = np.searchsorted(pos, (start + R)[order]), np.searchsorted(pos, (start + R2)[order])
            at = _ranges(lo, hi - lo)
            origin = (start + off[:, column])[order]
            steps.append(fr.Batch(flat[_ranges((plain + off[:, column])[order], lens[order])], _first(lens[order]).astype(np.uintp), order.astype(np.uint32),
                                  ids[at], (pos[at] - np.repeat(origin, hi - lo)).astype(np.int32), _first(hi - lo), off[order, column].astype(np.uint64)))
            R = R2
            column += 1
        else:
            assert column == sizes.shape[1], "the flush comes behind the last piece column"
            lo, hi = np.searchsorted(pos, (start + R)[order]), np.searchsorted(pos, (start + length)[order])
            at = _ranges(lo, hi - lo)
            steps.append(fr.End("flush", order.astype(np.uint32), ids[at], (pos[at] - np.repeat((start + length)[order], hi - lo)).astype(np.int32), _first(hi - lo)))
    return Case(pattern_set(M, nocase), nocase, F, steps, name, M, Info(buffer, start, length, sizes, pos, ids, orders))


def model(case, steps=None):
    """the schedule as tests/flows_ref.py's run() and the feeders take it"""
    m = fr.Model()
    m.M, m.F, m.steps = case.M, case.F, list(case.steps if steps is None else steps)
    return m


def twice_with_a_reset(case):
    """the case's batches, a reset of every flow in place of the flush -- the carries of the last batch are dropped --, and the whole case again"""
    return model(case, case.steps[:-1] + [fr.End("reset", np.arange(case.F, dtype=np.uint32), None, None, None)] + case.steps)


def _tokens(rng, n, tokens):
    """n bytes of tokens drawn at random and written one behind the other (the last one cut)"""
    longest = max(len(t) for t in tokens)
    table = np.zeros((len(tokens), longest), dtype=np.uint8)
    for i, t in enumerate(tokens):
        table[i, :len(t)] = np.frombuffer(t, dtype=np.uint8)
    tlen = np.array([len(t) for t in tokens], dtype=np.int64)
    drawn = rng.integers(0, len(tokens), size=n // int(tlen.min()) + 1)
    flat = table.reshape(-1)[_ranges(drawn * longest, tlen[drawn])]
    return flat[:n].copy()


def _small_filler(rng, n):
    """bytes of which about half start a pattern of M = 4's set: `a` x 3, `ab` x 2, L, S and `c`, cut wherever the pieces end"""
    a, ab, long_, short = pattern_list(A_M)
    return _tokens(rng, n, [a, a, a, ab, ab, long_, short, b"c"])


def _pieces_of(F, per_piece, sizes_of_piece):
    """sizes[F, K] of K batches: sizes_of_piece[k][j] is the length of PIECE j of batch k, which names the flows per_piece[k][j]"""
    sizes = np.zeros((F, len(per_piece)), dtype=np.int64)
    for k, order in enumerate(per_piece):
        sizes[order, k] = sizes_of_piece[k]
    return sizes


# --------------------------------------------------------------------------------------------------------------- A: piece-count edges

@functools.lru_cache(maxsize=None)
def piece_counts(P):
    rng = np.random.Generator(np.random.PCG64(8100 + P))
    sizes = rng.choice(np.array(LENS), size=(P, 2))
    sizes[-1] = (5, 9)
    sizes[0] = (9, 5)
    flat = _small_filler(rng, int(sizes.sum()))
    # the first and the last flow are runs of `a`, the last one the last piece of batch 2 and the first one the last of the flush: seam and scan
    # pairs in the first piece of a call and in the last piece of its last, partly filled block
    flat[:14] = ord("a")
    flat[flat.size - 14:] = ord("a")
    second, last = np.concatenate([rng.permutation(P - 1), [P - 1]]), np.concatenate([1 + rng.permutation(P - 1), [0]])
    if P >= 3 and np.array_equal(second, np.arange(P)):
        second[:P - 1] = np.roll(second[:P - 1], 1)
    return _build(f"A-{P}", A_M, False, flat, sizes, [("batch", np.arange(P)), ("batch", second), ("flush", last)])


# --------------------------------------------------------------------------------------------- B: pairs relative to a block of pieces

@functools.lru_cache(maxsize=None)
def block_positions(which):
    """batch 1 names flow f as piece f, batch 2 the flows in a permutation: `which` says what PIECE j of batch 2 looks like"""
    F, blk = B_PIECES, PIECE_BLOCK
    rng = np.random.Generator(np.random.PCG64(8200 + B_WHICH.index(which)))
    second, last = rng.permutation(F), rng.permutation(F)
    _, _, long_, _ = pattern_list(A_M)
    len1, len2 = rng.choice(np.array(LENS), size=F), rng.choice(np.array(LENS), size=F)         # by flow, by piece of batch 2
    if which in ("two-at-the-block-edge", "last-piece-only"):
        # the chosen pieces: a full carry `a` + L's first two bytes, then the rest of L (seam pairs at -3 and -2), `aab`, L, `a` -- scan pairs at
        # 2, 3 and 5 of 10 bytes, the last `a` pending until the flush; every other flow is `z` throughout
        chosen = [blk - 1, blk] if which == "two-at-the-block-edge" else [F - 1]
        len1[:] = A_M - 1
        streams = [b"z" * int(len1[f]) for f in range(F)]
        piece2 = [b"z" * int(n) for n in len2]
        for j in chosen:
            streams[second[j]] = b"a" + long_[:2]
            piece2[j] = long_[2:] + b"aab" + long_ + b"a"
            len2[j] = len(piece2[j])
        for j in range(F):
            streams[second[j]] += piece2[j]
        flat = np.frombuffer(b"".join(streams), dtype=np.uint8)
    else:
        if which == "empty-block":
            len2[blk:2 * blk] = 0
        elif which == "short-block":
            len1[second[blk:2 * blk]] = 9                                  # a full carry in front of every short piece
            len2[blk:2 * blk] = rng.integers(1, A_M - 1, size=blk)
        elif which == "empty-runs":
            len2[[9, 19, 299, F - 10]] = 5
            for lo, hi in ((10, 11), (20, 22), (300, 600), (F - 9, F)):
                len2[lo:hi] = 0
            len2[[11, 22, 600]] = 9
            len1[second[[11, 22, 600]]] = 9
        total = int(len1.sum() + len2.sum())
        flat = np.full(total, ord("a"), dtype=np.uint8) if which == "all-a" else _small_filler(rng, total)
        if which == "empty-runs":                                          # the pieces behind the runs: every byte a pair, seams and scan
            sizes = _pieces_of(F, [np.arange(F), second], [len1, len2])
            plain = np.concatenate([[0], np.cumsum(sizes.sum(axis=1))])
            for j in (11, 22, 600):
                flat[plain[second[j]]:plain[second[j] + 1]] = ord("a")
    sizes = _pieces_of(F, [np.arange(F), second], [len1, len2])
    return _build(f"B-{which}", A_M, False, flat, sizes, [("batch", np.arange(F)), ("batch", second), ("flush", last)])


# ---------------------------------------------------------------------------------------------------------------- C: seam shapes by M

def seam_grid(span):
    """[(carry state, second-piece length)]: 4 x 7 (below M = 3 some coincide; no size is negative from M = 2 on)"""
    M = span + 1
    return [(c, n) for c in (0, 1, M - 2, M - 1) for n in (0, 1, M - 2, M - 1, M, M + 1, 2 * M + 5)]


@functools.lru_cache(maxsize=None)
def seam_shapes(span, nocase=False):
    """flow f = grid entry f: batch 1 its carry state, batch 2 the second piece, batch 3 M + 3 bytes, the flush.  L starts at the flow's
    first byte where there is a carry (1 byte, M - 2 or M - 1 bytes in front of the first cut; with a second piece shorter than the rest
    it crosses the second cut too) -- S instead in every other flow of the full carry: it ends with the carry -- and one byte in front of
    the second cut where there is none.  Batch 1 leaves one flow without a carry out: 27 pieces"""
    M = span + 1
    pats = pattern_list(M)
    rng = np.random.Generator(np.random.PCG64(8300 + 2 * span + nocase))
    grid = seam_grid(span)
    assert len(grid) == C_FLOWS and C_FLOWS % WAVE_SEAM_PIECES == 0
    sizes = np.array([(c, n, M + 3) for c, n in grid], dtype=np.int64)
    streams = []
    for f, (c, n) in enumerate(grid):
        s = _tokens(rng, c + n + M + 3, [b"a", b"ab", b"b", b"c", pats[2][:2], b"z"])
        if c == 0:
            if n >= 1:
                s[n - 1:n - 1 + M] = np.frombuffer(pats[2], dtype=np.uint8)
        elif c == M - 1 and f % 2 and M >= 3:
            s[:M - 1] = np.frombuffer(pats[3], dtype=np.uint8)
        else:
            s[:M] = np.frombuffer(pats[2], dtype=np.uint8)
        streams.append(s)
    flat = np.concatenate(streams)
    if nocase:
        flat[rng.random(flat.size) < 0.5] ^= 0x20                          # (letters only: no separator in `flat`)
        assert np.all(fold_array(flat) >= ord("a"))
    left_out = next(f for f, (c, n) in enumerate(grid) if c == 0 and n == M)
    first = np.array([f for f in rng.permutation(C_FLOWS) if f != left_out])
    schedule = [("batch", first), ("batch", rng.permutation(C_FLOWS)), ("batch", rng.permutation(C_FLOWS)), ("flush", rng.permutation(C_FLOWS))]
    return _build(f"C-{span}{'-nocase' if nocase else ''}", M, nocase, flat, sizes, schedule)


def straddles(case):
    """how the occurrences of L in the model's list lie across their flow's cuts: {"one-in-front", "span-in-front", "two-cuts"} -> count"""
    i = case.info
    seen = collections.Counter()
    for f in range(case.F):
        a, b = np.searchsorted(i.pos, i.start[f]), np.searchsorted(i.pos, i.start[f] + i.length[f])
        cuts = np.unique(np.cumsum(i.sizes[f])[:-1])
        for p in (i.pos[a:b][i.ids[a:b] == 3] - i.start[f]).tolist():
            inside = [int(c) for c in cuts if p < c < p + case.M]
            seen["one-in-front"] += any(c == p + 1 for c in inside)
            seen["span-in-front"] += any(c == p + case.M - 1 for c in inside)
            seen["two-cuts"] += len(inside) >= 2
    return seen


# -------------------------------------------------------------------------------------------------------------------- D: dense seams

@functools.lru_cache(maxsize=None)
def dense_seams(span, behind):
    """every flow: M - 1 bytes `a` (the carry: all of them pending), then a piece of M - 1 + x bytes `behind` (`a` or `z`), the flush"""
    M = span + 1
    rng = np.random.Generator(np.random.PCG64(8400 + span))
    extra = (1, 2, 7, M, 2 * M + 5)
    assert len(extra) == D_FLOWS
    sizes = np.array([(span, span + x) for x in extra], dtype=np.int64)
    flat = np.concatenate([np.frombuffer(b"a" * span + behind * (span + x), dtype=np.uint8) for x in extra])
    every = np.arange(D_FLOWS)
    return _build(f"D-{span}-{behind.decode()}", M, False, flat, sizes, [("batch", every), ("batch", rng.permutation(D_FLOWS)), ("flush", rng.permutation(D_FLOWS))])


# ------------------------------------------------------------------------------------------------------------------ coverage asserts

def pairs_per_piece(step):
    return np.diff(np.asarray(step.first, dtype=np.int64))


def piece_lengths(step):
    return np.diff(step.offsets.astype(np.int64))


def _seam_pairs_per_piece(step):
    """of every piece the pairs with a negative position: those that start in carried bytes"""
    owner = np.repeat(np.arange(step.flows.size), pairs_per_piece(step))
    return np.bincount(owner[step.pos < 0], minlength=step.flows.size)


def sampled_flows(case):
    """the flows whose answers check_edges() derives again with stream_ref.split: all of up to 1024, else the first and last fifty, those
    named at the block and trip edges of every step, and 400 drawn at random"""
    if case.F <= 1024:
        return np.arange(case.F)
    rng = np.random.Generator(np.random.PCG64(8500))
    picked = set(range(50)) | set(range(case.F - 50, case.F)) | {int(f) for f in rng.choice(case.F, size=400, replace=False)}
    for order in case.info.orders:
        for edge in range(PIECE_BLOCK, order.size, SUMS_TRIP // 4):
            picked |= {int(f) for f in order[max(0, edge - 2):edge + 2]}
        for edge in range(SUMS_TRIP, order.size, SUMS_TRIP):
            picked |= {int(f) for f in order[edge - 2:edge + 2]}
    return np.array(sorted(picked))


def check_split(case):
    """the gathered arrays of every step equal stream_ref.split over the flow's own list, for the flows of sampled_flows()"""
    i = case.info
    where = []
    for order in i.orders:
        at = np.full(case.F, -1, dtype=np.int64)
        at[order] = np.arange(order.size)
        where.append(at)
    for f in sampled_flows(case).tolist():
        a, b = np.searchsorted(i.pos, i.start[f]), np.searchsorted(i.pos, i.start[f] + i.length[f])
        calls, flush = sr.split(i.pos[a:b] - i.start[f], i.ids[a:b], i.sizes[f].tolist(), case.M)
        column = 0
        for step, at in zip(case.steps, where):
            j = int(at[f])
            if isinstance(step, fr.Batch):
                want_ids, want_pos, want_off = calls[column]
                column += 1
                if j < 0:
                    assert want_ids.size == 0 and i.sizes[f, column - 1] == 0
                    continue
                assert int(step.offs[j]) == want_off and int(step.offsets[j + 1] - step.offsets[j]) == i.sizes[f, column - 1], (case.name, f)
            else:
                want_ids, want_pos = flush
            lo, hi = int(step.first[j]), int(step.first[j + 1])
            assert np.array_equal(step.ids[lo:hi], want_ids) and np.array_equal(step.pos[lo:hi], want_pos), (case.name, f)


def check_edges(case):
    """asserts on the model alone that the case holds what its family claims"""
    batches = [s for s in case.steps if isinstance(s, fr.Batch)]
    flush = case.steps[-1]
    assert isinstance(flush, fr.End) and flush.kind == "flush" and flush.flows.size == case.F
    for s in case.steps:
        assert s.first[0] == 0 and s.first[-1] == s.ids.size == s.pos.size and s.first.size == s.flows.size + 1
        assert np.unique(s.flows).size == s.flows.size
    for b in batches:
        assert b.offsets[-1] == b.buf.size < (1 << 20) or case.name.startswith("C-")
        owner = np.repeat(np.arange(b.flows.size), pairs_per_piece(b))
        assert np.all(b.pos >= -(case.M - 1)) and np.all(b.pos < np.maximum(piece_lengths(b)[owner] - (case.M - 1), 0))
    check_split(case)
    family = case.name[0]
    if family == "A":
        P = case.F
        assert [b.flows.size for b in batches] == [P, P] and np.array_equal(batches[0].flows, np.arange(P))
        if P > 1:
            assert (P == 2 or not np.array_equal(batches[1].flows, batches[0].flows)) and not np.array_equal(flush.flows, batches[1].flows)
        for b in batches:
            assert set(piece_lengths(b).tolist()) <= set(LENS)
        if P >= PIECE_BLOCK - 1:
            for b in batches:
                assert set(piece_lengths(b).tolist()) == set(LENS)
                hit = np.count_nonzero(longest_at(pattern_list(A_M), b.buf)) / b.buf.size
                assert 0.35 < hit < 0.65, f"{case.name}: {hit:.2f} of all positions hit"
            assert set(np.concatenate([b.ids for b in batches]).tolist()) == {1, 2, 3, 4}
        for s in batches[1:] + [flush]:                           # pairs in the last piece: the last, partly filled block where there is one
            assert pairs_per_piece(s)[-1] > 0, case.name
        assert _seam_pairs_per_piece(batches[1])[-1] == A_M - 1 and pairs_per_piece(batches[0])[0] == 9 - (A_M - 1)
        if P > SUMS_TRIP:
            for s in case.steps:                                  # pieces behind the first trip of pfac_flows_sums hold pairs
                assert pairs_per_piece(s)[SUMS_TRIP:].sum() > 0 and pairs_per_piece(s)[:SUMS_TRIP].sum() > 0
            assert _seam_pairs_per_piece(batches[1])[SUMS_TRIP:].sum() > 0
    elif family == "B":
        blk = PIECE_BLOCK
        assert case.F == B_PIECES and [b.flows.size for b in batches] == [B_PIECES, B_PIECES]
        b = batches[1]
        n, lens, seam = pairs_per_piece(b), piece_lengths(b), _seam_pairs_per_piece(b)
        which = case.name[2:]
        if which in ("two-at-the-block-edge", "last-piece-only"):
            chosen = [blk - 1, blk] if which == "two-at-the-block-edge" else [B_PIECES - 1]
            assert np.flatnonzero(n).tolist() == chosen
            assert all(seam[j] == 2 and n[j] - seam[j] == 3 for j in chosen), "seam and scan pairs in every chosen piece"
            assert np.flatnonzero(pairs_per_piece(flush)).size == len(chosen) and not pairs_per_piece(batches[0]).any()
        elif which == "empty-block":
            assert not lens[blk:2 * blk].any() and not n[blk:2 * blk].any() and n[:blk].sum() > 0 and n[2 * blk:3 * blk].sum() > 0
            assert seam[:blk].sum() > 0 and seam[2 * blk:].sum() > 0
        elif which == "short-block":
            short = slice(blk, 2 * blk)
            assert lens[short].min() >= 1 and lens[short].max() < case.M - 1
            assert np.array_equal(n[short], seam[short]) and np.count_nonzero(n[short]) > blk // 4, "seam pairs only, in many pieces"
            assert (n - seam)[:blk].sum() > 0 and (n - seam)[2 * blk:].sum() > 0
        elif which == "all-a":
            assert all(np.all(s.buf == ord("a")) for s in batches) and all(np.all(s.ids == 1) for s in case.steps)
            assert sum(s.ids.size for s in case.steps) == sum(s.buf.size for s in batches), "every position is a pair, once"
            final = np.maximum(lens - (case.M - 1), 0)
            assert np.array_equal(n - seam, final) and set(lens.tolist()) == set(LENS)
            for j in np.flatnonzero(final).tolist():              # the first and the last final position of every piece, and no pending one
                own = b.pos[b.first[j] + seam[j]:b.first[j + 1]]
                assert own[0] == 0 and own[-1] == final[j] - 1
        else:
            assert which == "empty-runs"
            for lo, hi in ((10, 11), (20, 22), (300, 600), (B_PIECES - 9, B_PIECES)):
                assert not lens[lo:hi].any() and not n[lo:hi].any()
            for j in (11, 22, 600):
                assert lens[j] == 9 and lens[j - 1] == 0 and seam[j] == case.M - 1 and n[j] - seam[j] == 9 - (case.M - 1)
            assert lens[9] > 0 and lens[19] > 0 and lens[299] > 0 and lens[B_PIECES - 10] > 0
    elif family == "C":
        span = case.M - 1
        assert [b.flows.size for b in batches] == [C_FLOWS - 1, C_FLOWS, C_FLOWS] and (C_FLOWS - 1) % WAVE_SEAM_PIECES != 0
        assert sorted(map(tuple, case.info.sizes[:, :2].tolist())) == sorted(seam_grid(span)) and np.all(case.info.sizes[:, 2] == case.M + 3)
        for b in batches[:2]:                                     # the batches name the flows in an order of their own
            assert not np.array_equal(b.flows, np.sort(b.flows))
        seen = straddles(case)
        assert seen["one-in-front"] >= 1 and seen["span-in-front"] >= 1, (case.name, seen)
        if case.M >= 3:
            assert seen["two-cuts"] >= 1, (case.name, seen)
            assert 4 in set(batches[1].ids.tolist()) | set(batches[2].ids.tolist()), "S, which ends with the carry, is reported"
        assert sum(_seam_pairs_per_piece(b).sum() for b in batches[1:]) >= C_FLOWS // 2
        if case.nocase:
            raw = np.concatenate([b.buf for b in batches])
            assert 0.3 < np.count_nonzero(raw < ord("a")) / raw.size < 0.7, "upper and lower case mixed"
            assert case.patterns != case.patterns.lower() and case.patterns != case.patterns.upper()
    else:
        assert family == "D" and case.F == D_FLOWS and [b.flows.size for b in batches] == [D_FLOWS, D_FLOWS]
        span = case.M - 1
        assert not batches[0].ids.size, "the carry is all pending"
        seam = _seam_pairs_per_piece(batches[1])
        assert np.all(seam == span), "every carried position is a seam pair"
        floor = {D_SPANS[0]: WAVE_SEAM_MAX, D_SPANS[1]: WAVE_SEAM_MAX + 1, D_SPANS[2]: SEAM_BLOCK + 1}[span]
        assert seam.min() >= floor
        scan = pairs_per_piece(batches[1]) - seam
        if case.name.endswith("-z"):
            assert not scan.any() and not flush.ids.size
        else:
            assert np.all(scan > 0) and np.all(pairs_per_piece(flush) == span)


def case_names(a_max=None):
    """the names of all cases (A up to a_max pieces): A-<pieces>, B-<which>, C-<span>[-nocase], D-<span>-<a|z>"""
    return ([f"A-{P}" for P in A_COUNTS if a_max is None or P <= a_max] + [f"B-{w}" for w in B_WHICH] + [f"C-{s}" for s in C_SPANS]
            + [f"C-{s}-nocase" for s in C_NOCASE_SPANS] + [f"D-{s}-{b}" for s in D_SPANS for b in "az"])


def case_named(name):
    family, _, rest = name.partition("-")
    if family == "A":
        return piece_counts(int(rest))
    if family == "B":
        return block_positions(rest)
    if family == "C":
        return seam_shapes(int(rest.split("-")[0]), rest.endswith("-nocase"))
    span, behind = rest.split("-")
    return dense_seams(int(span), behind.encode())
