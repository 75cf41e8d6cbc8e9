"""The model of the flows calls (PFACX_flows*) for tests/test_flows_host.py and test_flows_gpu.py.

Nothing here uses the library's stream or flow code.  F flows, each a slice of a workload cut by stream_ref.make_sizes; the expected
answer of every piece is stream_ref.split over the oracle's full list of that flow's bytes.  A seeded scheduler deals the pieces into
batches -- every batch a random subset of the flows that still have pieces, in shuffled order, one piece per flow, packed into one
buffer -- and the expected (ids, pos, pieceFirst, pieceOffsets) of a batch is the concatenation of its pieces' answers.  A flow may be
RESTARTED at a piece boundary: its bytes so far end there (the model's flush: the oracle over exactly those bytes) and the rest is a
fresh stream; the schedule then holds a flush or a reset of the flows that have reached their boundary, in the middle of the others.

build() asserts the coverage a lucky schedule could otherwise miss (see `check_coverage`).
"""
import numpy as np

from tests import stream_ref as sr


class Batch:
    def __init__(self, buf, offsets, flows, ids, pos, first, offs):
        self.buf, self.offsets, self.flows, self.ids, self.pos, self.first, self.offs = buf, offsets, flows, ids, pos, first, offs


class End:
    """the flows named flush (kind 'flush': with the expected pairs, flow by flow) or are reset (kind 'reset')"""

    def __init__(self, kind, flows, ids, pos, first):
        self.kind, self.flows, self.ids, self.pos, self.first = kind, flows, ids, pos, first


class Model:
    def __init__(self):
        self.M = 1
        self.F = 0
        self.steps = []            # Batch and End, in call order
        self.straddling = 0
        self.longer = 0            # occurrences of two bytes or more in all flows
        self.pieces = 0


def _list(o, data):
    if data.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int32)
    full = o.match(np.ascontiguousarray(data, dtype=np.uint8))
    pos = np.flatnonzero(full > 0).astype(np.int64)
    return pos, full[pos].astype(np.int32)


def _cat(parts, dtype):
    parts = [np.asarray(p, dtype=dtype) for p in parts]
    return np.concatenate(parts) if parts else np.zeros(0, dtype)


def build(pattern_file, data, F, seed, whole=False, restart=None, sizes_of=None, fold=None, big=True):
    """the schedule of F flows over `data` (whole: every flow gets all of it, for workloads of a dozen bytes; else flow f gets the f-th
    of F slices).  restart: {flow: ('flush' | 'reset', fraction of its bytes)}.  sizes_of(n, M, pos, ids, lengths, seed) replaces
    stream_ref.make_sizes.  fold: the model matches fold(bytes) (a caseless set) while the calls get the bytes as they are.
    big: assert the coverage of check_coverage (off only for inputs of a dozen bytes and the five-flow mixed sets of tests/nocase_ref.py, which
    cannot fill a batch of 64 pieces; test_flows_host.py: caseless_model covers a folding set with full coverage)"""
    from oracle import binding as ob
    data = np.ascontiguousarray(data, dtype=np.uint8)
    lengths = sr.pattern_lengths(pattern_file)
    m = Model()
    m.M = M = int(lengths.max())
    m.F = F
    rng = np.random.Generator(np.random.PCG64(seed))
    bounds = np.linspace(0, data.size, F + 1).astype(np.int64)
    restart = restart or {}
    queues = []                    # per flow: [(bytes, expected (ids, pos, off)) ... or ('end', kind, ids, pos)]
    o = ob.Oracle(pattern_file, hashed=False)
    try:
        for f in range(F):
            mine = data if whole else data[bounds[f]:bounds[f + 1]]
            segments = [mine]
            if f in restart:
                cut = int(mine.size * restart[f][1])
                segments = [mine[:cut], mine[cut:]]
            q = []
            for si, seg in enumerate(segments):
                pos, ids = _list(o, seg if fold is None else fold(seg))
                make = sizes_of or (lambda n, M_, p, i, l, s: sr.make_sizes(n, M_, p, i, l, seed=s, placed=8, twice=2, coarse=6))
                sizes = make(seg.size, M, pos, ids, lengths, seed * 1000 + 2 * f + si)
                calls, flush = sr.split(pos, ids, sizes, M)
                m.straddling += sr.straddling(pos, ids, lengths, sizes)
                m.longer += int(np.count_nonzero(lengths[ids] >= 2))
                off = 0
                for size, call in zip(sizes, calls):
                    q.append((seg[off:off + size], call))
                    off += size
                last = si == len(segments) - 1
                q.append(("end", "flush" if last else restart[f][0], flush[0], flush[1]))
            queues.append(q)
    finally:
        o.close()

    at = [0] * F
    round_no = 0
    while True:
        # flows that have reached a boundary in the middle of the schedule: flushed or reset before the next batch
        for kind in ("flush", "reset"):
            due = [f for f in range(F) if at[f] < len(queues[f]) - 1 and isinstance(queues[f][at[f]][0], str) and queues[f][at[f]][1] == kind]
            if due:
                due = [due[i] for i in rng.permutation(len(due))]
                ends = [queues[f][at[f]] for f in due]
                first = np.concatenate([[0], np.cumsum([e[2].size for e in ends])]).astype(np.int32)
                m.steps.append(End(kind, np.array(due, np.uint32), _cat([e[2] for e in ends], np.int32), _cat([e[3] for e in ends], np.int32), first))
                for f in due:
                    at[f] += 1
        active = [f for f in range(F) if at[f] < len(queues[f]) - 1]
        if not active:
            break
        if round_no < 2:
            chosen = active                                   # everybody: F pieces (make_sizes starts with an empty piece, then one byte)
        elif round_no == 2:
            chosen = [active[int(rng.integers(0, len(active)))]]      # a single piece
        else:
            chosen = list(rng.choice(active, size=int(rng.integers(1, len(active) + 1)), replace=False))
        chosen = [int(chosen[i]) for i in rng.permutation(len(chosen))]
        round_no += 1
        parts, exp = [], []
        for f in chosen:
            bytes_, call = queues[f][at[f]]
            at[f] += 1
            parts.append(bytes_)
            exp.append(call)
        offsets = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uintp)
        first = np.concatenate([[0], np.cumsum([e[0].size for e in exp])]).astype(np.int32)
        m.steps.append(Batch(_cat(parts, np.uint8), offsets, np.array(chosen, np.uint32), _cat([e[0] for e in exp], np.int32),
                             _cat([e[1] for e in exp], np.int32), first, np.array([e[2] for e in exp], np.uint64)))
        m.pieces += len(chosen)
    order = [int(f) for f in rng.permutation(F)]
    ends = [queues[f][-1] for f in order]
    first = np.concatenate([[0], np.cumsum([e[2].size for e in ends])]).astype(np.int32)
    m.steps.append(End("flush", np.array(order, np.uint32), _cat([e[2] for e in ends], np.int32), _cat([e[3] for e in ends], np.int32), first))
    if big:
        check_coverage(m)
    return m


def check_coverage(m):
    """what a schedule must contain to prove anything: occurrences that straddle two calls (as many as tests/test_stream_gpu.py::model
    demands of one stream), a batch of >= 64 pieces, one whose every piece is shorter than M - 1 and not all are empty (no scan is
    launched; M > 2), one with empty pieces, one of a single piece, a flow that sits a batch out and comes back"""
    batches = [s for s in m.steps if isinstance(s, Batch)]
    assert m.straddling >= min(20, m.longer), (m.straddling, m.longer)
    lens = [np.diff(b.offsets.astype(np.int64)) for b in batches]
    assert any(l.size >= 64 for l in lens), "no batch of 64 pieces"
    if m.M > 2:
        assert any(l.max() < m.M - 1 and l.max() > 0 for l in lens), "no batch of pieces all shorter than M - 1"
    assert any((l == 0).any() for l in lens), "no batch with an empty piece"
    assert any(l.size == 1 for l in lens), "no batch of a single piece"
    seen_gap = False
    last_in = {}
    for k, b in enumerate(batches):
        for f in b.flows.tolist():
            if f in last_in and last_in[f] < k - 1:
                seen_gap = True
            last_in[f] = k
    assert seen_gap, "no flow was absent from a batch and back in a later one"


def run(m, piece_call, flush_call, reset_call, what):
    """the schedule through piece_call(batch) -> (ids, pos, pieceFirst[numPieces + 1], pieceOffsets), flush_call(flow ids) -> (ids, pos,
    first[n + 1]) and reset_call(flow ids); every call compared with the model"""
    for k, s in enumerate(m.steps):
        where = f"{what}: step {k}"
        if isinstance(s, Batch):
            ids, pos, first, offs = piece_call(s)
            where += f" (batch of {s.flows.size} pieces, {s.buf.size} bytes)"
            assert np.array_equal(np.asarray(first), s.first), f"{where}: pieceFirst differs"
            assert np.array_equal(np.asarray(offs, dtype=np.uint64), s.offs), f"{where}: piece offsets differ"
            assert ids.size == s.ids.size, f"{where}: {ids.size} pairs, want {s.ids.size}"
            assert np.array_equal(pos, s.pos), f"{where}: positions differ"
            assert np.array_equal(ids, s.ids), f"{where}: ids differ"
        elif s.kind == "reset":
            reset_call(s.flows)
        else:
            ids, pos, first = flush_call(s.flows)
            assert np.array_equal(np.asarray(first), s.first), f"{where}: flush: first differs"
            assert np.array_equal(pos, s.pos) and np.array_equal(ids, s.ids), f"{where}: flush of {s.flows.size} flows differs"
