"""The cases of tests/flows_edges.py hold the piece counts, block positions, seam shapes and seam densities their names say, their matcher
agrees with the oracle over the same bytes, and PFACX_flowsMatchFromHost / PFACX_flowsFlush on a host-only handle return them call by call.
No device needed."""
import os
import re

import numpy as np
import pytest

from pfac_amd import api
from tests import flows_edges as fe
from tests import flows_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_name_the_kernels_constants():
    assert (api.PFACX_FLOWS_PIECE_BLOCK, api.PFACX_FLOWS_WAVE_SEAM_MAX, api.PFACX_FLOWS_WAVE_SEAM_PIECES, api.PFACX_STREAM_SEAM_BLOCK,
            api.PFACX_STREAM_SEAM_LDS) == (256, 64, 4, 1024, 49152)

    def src(name):
        with open(os.path.join(ROOT, "pfac_amd", "csrc", name)) as f:
            return f.read()

    def const(text, decl):
        return int(re.search(decl + r" = (\d+);", text).group(1))

    flows, stream, context = src("scan_flows.hip"), src("scan_stream.hip"), src("pfac_context.h")
    assert const(flows, "constexpr int kPieceBlock") == api.PFACX_FLOWS_PIECE_BLOCK
    assert const(flows, "constexpr int kWaveSeamMax") == api.PFACX_FLOWS_WAVE_SEAM_MAX
    assert const(flows, "constexpr int kWaveSeamBlock") == 64 * api.PFACX_FLOWS_WAVE_SEAM_PIECES and "kWaveSeamWaves = kWaveSeamBlock / 64;" in flows
    assert const(flows, "constexpr int kSeamBlock") == const(stream, "constexpr int kSeamBlock") == api.PFACX_STREAM_SEAM_BLOCK
    assert re.search(r"constexpr size_t kStreamSeamLdsBytes = 48 \* 1024;", context) and api.PFACX_STREAM_SEAM_LDS == 48 * 1024
    assert "base += kPieceBlock" in flows, "a trip of pfac_flows_sums takes kPieceBlock block sums"
    assert fe.A_COUNTS == (1, 3, 4, 5, 255, 256, 257, 511, 512, 513, 65535, 65536, 65537, 131073)
    assert fe.C_SPANS == (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2049, 24576, 24577) and fe.C_NOCASE_SPANS == (64, 65, 24577)
    assert 2 * fe.C_SPANS[-2] == api.PFACX_STREAM_SEAM_LDS and 2 * fe.C_SPANS[-1] == api.PFACX_STREAM_SEAM_LDS + 2
    assert fe.D_SPANS == (64, 200, 1500) and fe.B_PIECES == 769


def test_pattern_sets_and_the_matcher_on_a_known_answer():
    for M in (2, 3, 4, 65, 1025):
        pats = fe.pattern_list(M)
        assert pats[:2] == [b"a", b"ab"] and len(pats[2]) == M and (M < 3 or len(pats[3]) == M - 1) and len(pats) == (4 if M >= 3 else 3)
        assert fe.parse_patterns(fe.pattern_set(M)) == pats and [p.lower() for p in fe.parse_patterns(fe.pattern_set(M, True))] == pats
        for shift in range(1, M):                                       # non-periodic: L overlaps no shifted copy of itself
            assert pats[2][shift:] != pats[2][:M - shift]
    a, ab, long_, short = fe.pattern_list(4)
    data = np.frombuffer(b"zab" + long_ + b"a" + short + long_[:3] + b"\x00" + b"a", dtype=np.uint8)
    want = [0, 2, 0, 3, 0, 0, 0, 2, 4, 0, 0, 1, 0, 0, 0, 1]
    assert fe.longest_at([a, ab, long_, short], data).tolist() == want
    assert fe.longest_at(fe.parse_patterns(fe.pattern_set(4, True)), np.frombuffer(data.tobytes().upper(), dtype=np.uint8), nocase=True).tolist() == want
    assert not fe.longest_at([a, ab, long_, short], np.frombuffer(data.tobytes().upper(), dtype=np.uint8)).any()


@pytest.mark.parametrize("P", fe.A_COUNTS)
def test_piece_count_cases_hold_what_they_claim(P):
    case = fe.piece_counts(P)
    fe.check_edges(case)
    assert all(s.flows.size == P for s in case.steps)
    if P == fe.A_COUNTS[-1]:
        assert all(s.buf.size < (1 << 20) for s in case.steps[:2]), "a batch of 131 073 pieces stays under 1 MiB"
    if P > 1024:
        assert 400 <= fe.sampled_flows(case).size < 1024


def test_every_other_case_holds_what_it_claims():
    names = fe.case_names(a_max=0)
    assert len(names) == len(fe.B_WHICH) + len(fe.C_SPANS) + len(fe.C_NOCASE_SPANS) + 2 * len(fe.D_SPANS)
    for name in names:
        case = fe.case_named(name)
        assert case.name == name
        fe.check_edges(case)


def _oracle_full(workdir, case):
    """the oracle over the case's buffer (a caseless set: the folded set over the folded bytes, which is the definition)"""
    from oracle import binding as ob
    pats, data = fe.parse_patterns(case.patterns), case.info.buffer
    if case.nocase:
        pats, data = [p.lower() for p in pats], fe.fold_array(data)
    path = os.path.join(workdir, f"flows_edges_{case.name}.pat")
    with open(path, "wb") as f:
        f.write(b"".join(p + b"\n" for p in pats))
    o = ob.Oracle(path, hashed=False)
    try:
        return o.match(np.ascontiguousarray(data))
    finally:
        o.close()


ORACLE_CASES = [n for n in fe.case_names(a_max=0) if n[0] == "C" or (n[0] == "D" and n.endswith("-a"))] + [f"A-{2 * fe.PIECE_BLOCK + 1}"]


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_the_models_full_list_equals_the_oracles(workdir, name):
    """every pattern set of C and D (D's two variants share a set) and one flow set of A"""
    case = fe.case_named(name)
    full = _oracle_full(workdir, case)
    i = case.info
    mine = np.zeros(i.buffer.size, dtype=np.int32)
    mine[i.pos] = i.ids
    bad = np.flatnonzero(full != mine)
    assert bad.size == 0, f"{case.name}: {bad.size} positions differ, first at {bad[0]}: oracle {full[bad[0]]}, model {mine[bad[0]]}"
    assert i.pos.size > 0 and (name[0] == "D" or set(i.ids.tolist()) >= {1, 2, 3})


def _host_handle(case):
    h = api.PFAC.createHostOnly()
    h.readPatternFromMemoryEx(case.patterns, api.PFACX_READ_NOCASE if case.nocase else 0)
    return h


def feed_host_only(h, m, what):
    """the schedule through the host calls of one flow set, as tests/test_flows_gpu.py: feed_host does; the caller's arrays stay as they were"""
    fl = h.flowsOpen(m.F)

    def piece(b):
        buf, off, flows = b.buf.copy(), b.offsets.copy(), b.flows.copy()
        out = fl.match_host_array(buf, off, flows)[1:]
        assert np.array_equal(buf, b.buf) and np.array_equal(off, b.offsets) and np.array_equal(flows, b.flows), f"{what}: input arrays were modified"
        return out

    try:
        fr.run(m, piece, lambda flows: fl.flush_host_array(flows)[1:], lambda flows: fl.reset(flows), what)
    finally:
        fl.close()


@pytest.mark.parametrize("name", fe.case_names(a_max=fe.A_HOST_MAX))
def test_the_host_calls_return_every_case(name):
    case = fe.case_named(name)
    h = _host_handle(case)
    try:
        assert h.info().maxPatternLen == case.M
        feed_host_only(h, fe.model(case), f"{case.name} host-only")
        if case.name == "B-all-a":
            feed_host_only(h, fe.twice_with_a_reset(case), f"{case.name} host-only, twice with a reset")
    finally:
        h.destroy()
