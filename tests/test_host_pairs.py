"""The one helper behind every host form that works on longest pairs (pfac_host.h: hostLongestPairs), on the CPU platforms (host-only handles:
no device needed).  For each input the pairs of PFAC_matchFromHostReduce are the non-zero entries of PFAC_matchFromHost's vector, in order; what
PFACX_matchAllFromHost, PFACX_countFromHost, PFACX_matchLinesFromHost and PFACX_matchSpansFromHost return then follows from those pairs alone,
through the models of tests/*_ref.py.  The inputs are the smallest that can go wrong in the shared code: one byte, a match that ends on the
last byte, no or a last '\\n', a run in which every position matches (the in-place compaction), bytes >= 0x80.  A host-fed stream and a
two-flow set in pieces of 1, M - 2, M - 1 and M bytes pin the read-ahead (owned < readable) and the negative position shift of a seam."""

import numpy as np
import pytest

from pfac_amd import api
from tests import allmatch_ref as am
from tests import count_ref, lines_ref, spans_ref, stream_ref

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
LONGEST = api.PFACX_COUNT_LONGEST

# (name, patterns, input); "dense_hits" and "binary" are the workloads of conftest.py
SMALL = [
    ("one-byte-match", [b"a", b"ab"], b"a"),
    ("one-byte-no-match", [b"ab"], b"a"),
    ("only-match-ends-on-the-last-byte", [b"needle", b"nee"], b"no newline here, then the needle"),
    ("no-newline", [b"ab", b"x", b"abc"], b"abc ab x-- abx"),
    ("ends-in-newline", [b"ab", b"x", b"abc"], b"abc\nnothing\n\nab x\nlast ab\n"),
]
CASES = [c[0] for c in SMALL] + ["dense_hits", "binary"]


def patterns_of(pattern_file):
    return open(pattern_file, "rb").read().split(b"\n")[:-1]


@pytest.fixture(scope="module")
def inputs(workdir, workloads):
    """{name: (pattern file, patterns, data)}"""
    from pfac_amd import workloads as wl
    out = {}
    for name, pats, data in SMALL:
        pf = wl.write_pattern_file(workdir + "/host_pairs_" + name + ".pat", pats)
        out[name] = (pf, pats, np.frombuffer(data, dtype=np.uint8))
    for name in ("dense_hits", "binary"):
        w = workloads[name]
        out[name] = (w.pattern_file, patterns_of(w.pattern_file), w.data)
    return out


def host_handle(pattern_file, platform):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    h.readPatternFromFile(pattern_file)
    return h


def host_pairs(h, data):
    """(pos, ids) of PFAC_matchFromHostReduce, from arrays of exactly `size` entries"""
    buf = data.copy()
    ids, pos = (np.full(buf.size, -7, dtype=np.int32) for _ in range(2))
    _, n = h.matchFromHostReduce(buf.ctypes.data, buf.size, ids.ctypes.data, pos.ctypes.data)
    assert np.array_equal(buf, data), "the caller's input was modified"
    return pos[:n].copy(), ids[:n].copy()


def vector_of(pos, ids, n):
    r = np.zeros(n, dtype=np.int32)
    r[pos] = ids
    return r


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("name", CASES)
def test_every_host_form_follows_from_the_pairs(inputs, monkeypatch, name, platform, pname):
    monkeypatch.setenv("OMP_NUM_THREADS", "4")          # CPU_OMP runs threads only with it set
    pf, pats, data = inputs[name]
    h = host_handle(pf, platform)
    try:
        pos, ids = host_pairs(h, data)
        full = h.match_host_array(data)
        assert np.array_equal(pos, np.flatnonzero(full)), "the positions are those of the vector's non-zero entries, in order"
        assert np.array_equal(ids, full[pos]), "the ids are the vector's non-zero entries, in order"
        if name in ("one-byte-match", "only-match-ends-on-the-last-byte"):
            assert pos.size == 1 and pos[0] + len(pats[ids[0] - 1]) == data.size, "the case is what its name says"
        r = vector_of(pos, ids, data.size)              # from here on: the pairs alone

        want_pos, want_ids = am.expand_longest(pats, r)
        got_pos, got_ids = h.match_all_host_array(data)
        assert np.array_equal(got_pos, want_pos) and np.array_equal(got_ids, want_ids), "matchAllFromHost"

        prefix, chain, _ = am.prefix_table(pats)
        for longest in (False, True):
            got, total = h.count_host_array(data, longest)
            count_ref.same(got, count_ref.counts_from_result(r, (prefix, chain), longest), f"countFromHost, longest {longest}")
            assert total == count_ref.total_of(r, (prefix, chain), longest)

        for invert in (False, True):
            lines_ref.same(h.match_lines_host_array(data, invert), lines_ref.lines_from_result(r, data, invert), f"matchLinesFromHost, invert {invert}")

        start, length, covered = h.match_spans_host_array(data)
        want = spans_ref.spans_from_result(r, spans_ref.pattern_lengths(pats))
        spans_ref.same((start, length), want, "matchSpansFromHost")
        assert covered == int(np.asarray(want[1], dtype=np.int64).sum())
    finally:
        h.destroy()


def piece_sizes(n, M, phase=0):
    """1, M - 2, M - 1, M, 1, ... bytes until n are used up"""
    cycle = [1, M - 2, M - 1, M]
    sizes, k = [], phase
    while sum(sizes) < n:
        sizes.append(min(cycle[k % 4], n - sum(sizes)))
        k += 1
    return sizes


@pytest.fixture(scope="module")
def dense_slice(inputs):
    """the end of a run of a's, the run of b's and the start of the abc's of dense_hits: every position of the first 200 bytes matches"""
    pf, pats, data = inputs["dense_hits"]
    return pf, max(len(p) for p in pats), np.ascontiguousarray(data[2800:4300])


@pytest.mark.parametrize("platform,pname", PLATFORMS)
def test_a_host_fed_stream_in_pieces_around_the_longest_pattern(dense_slice, monkeypatch, platform, pname):
    monkeypatch.setenv("OMP_NUM_THREADS", "4")
    pf, M, data = dense_slice
    assert M > 3
    h = host_handle(pf, platform)
    try:
        pos, ids = host_pairs(h, data)
        assert np.all(np.diff(pos[:200]) == 1), "a run in which every position matches"
        sizes = piece_sizes(data.size, M)
        calls, flush = stream_ref.split(pos.astype(np.int64), ids, sizes, M)
        assert any(c[1].size and c[1][0] < 0 for c in calls), "some seam reports a carried position"
        s = h.streamOpen()
        stream_ref.run(lambda off, size: s.match_host_array(data[off:off + size]), s.flush_host_array, data, sizes, calls, flush, pname)
        s.close()
    finally:
        h.destroy()


@pytest.mark.parametrize("platform,pname", PLATFORMS)
def test_a_two_flow_set_in_pieces_around_the_longest_pattern(dense_slice, monkeypatch, platform, pname):
    monkeypatch.setenv("OMP_NUM_THREADS", "4")
    pf, M, data = dense_slice
    h = host_handle(pf, platform)
    try:
        streams = [data[:900], data[600:]]              # flow 1 starts inside the a's and ends with the slice
        models = []
        for f, d in enumerate(streams):
            pos, ids = host_pairs(h, np.ascontiguousarray(d))
            sizes = piece_sizes(d.size, M, phase=f)     # the two flows are never at the same size
            models.append((sizes, *stream_ref.split(pos.astype(np.int64), ids, sizes, M)))
        fl = h.flowsOpen(2)
        at = [0, 0]
        for k in range(max(len(m[0]) for m in models)):
            flows = [f for f in (0, 1) if k < len(models[f][0])]
            pieces = [streams[f][at[f]:at[f] + models[f][0][k]] for f in flows]
            offsets = np.concatenate(([0], np.cumsum([p.size for p in pieces])))
            _, ids, pos, first, offs = fl.match_host_array(np.concatenate(pieces), offsets, flows)
            for j, f in enumerate(flows):
                want_ids, want_pos, want_off = models[f][1][k]
                where = f"{pname}: call {k}, flow {f}"
                assert offs[j] == want_off, where
                assert np.array_equal(ids[first[j]:first[j + 1]], want_ids), where + ": ids differ"
                assert np.array_equal(pos[first[j]:first[j + 1]], want_pos), where + ": positions differ"
                at[f] += pieces[j].size
        _, ids, pos, first = fl.flush_host_array([1, 0])
        for j, f in enumerate((1, 0)):
            want_ids, want_pos = models[f][2]
            assert np.array_equal(ids[first[j]:first[j + 1]], want_ids) and np.array_equal(pos[first[j]:first[j + 1]], want_pos), f"{pname}: flush of flow {f}"
        fl.close()
    finally:
        h.destroy()
