"""Pattern sets of 100 000 and 300 000 patterns on the host (tests/scale_sets.py): the product's CPU engine and the reference's own CPU
matcher against the hashed oracle at 1.6 M / 4.8 M states, the compiled-set round trip of the large set, and the preconditions of every
fixture tests/test_scale_gpu.py runs on -- checked here, without a device, by the filter model and the oracle."""

import numpy as np
import pytest

from oracle import binding as ob
from pfac_amd import api
from tests import scale_sets as ss
from tests.scale_sets import assert_same

HOST_BYTES = 8 << 20


@pytest.mark.parametrize("perf,pname", [(api.PFAC_SPACE_DRIVEN, "hashed"), (api.PFAC_TIME_DRIVEN, "dense")])
@pytest.mark.parametrize("count", [ss.S100, ss.S300])
def test_cpu_engine_equals_the_hashed_oracle(count, perf, pname):
    """PFAC_PLATFORM_CPU and PFAC_PLATFORM_CPU_OMP in both perf modes over 8 MiB (PFAC_TIME_DRIVEN walks the dense table on the host:
    1.6 GB / 4.9 GB while this test runs)."""
    data = ss.text(count, HOST_BYTES)
    want = ss.want(ss.pattern_file(count), data)
    assert np.count_nonzero(want) > 400
    h = api.PFAC.createHostOnly()
    try:
        h.setPerfMode(perf)
        h.readPatternFromFile(ss.pattern_file(count))
        for platform, name in ((api.PFAC_PLATFORM_CPU, "CPU"), (api.PFAC_PLATFORM_CPU_OMP, "CPU_OMP")):
            h.setPlatform(platform)
            assert_same(h.match_host_array(data), want, f"{count} patterns / {name} / {pname}")
    finally:
        h.destroy()


def test_reference_matcher_on_the_oracles_hash_tables_of_the_large_set():
    """The reference's CPU matcher over the oracle's hash_row / hash_val of S300 gives the oracle's vector on 4 MiB: the construction of
    the hash tables every GPU test of tests/test_scale_gpu.py rests on, at 4.8 M states.  (Without the reference library -- a checkout
    that never saw the reference tree -- the oracle's scalar and OpenMP matchers are still compared.)"""
    data = ss.text(ss.S300, HOST_BYTES)[:4 << 20]
    o = ss._oracle(ss.pattern_file(ss.S300))
    want = o.match(data, hashed=True, omp=True)
    assert o.num_states > 4_500_000 and np.count_nonzero(want) > 200
    assert_same(o.match(data, hashed=True), want, "oracle, scalar against OpenMP")
    if ob.have_reference():
        row, val = o.hash_row(), o.hash_val()
        for omp in (False, True):
            assert_same(ob.Reference.match_hash(data, row, val, o.num_patterns, o.initial_state, omp), want, f"reference matcher, omp={omp}")


def test_fixture_text_of_the_100k_set_takes_several_list_rounds_in_every_chunk():
    hits = ss.check_text_hits(ss.S100, ss.text(ss.S100, HOST_BYTES)[:4 << 20])
    print(f"\n[S100 text, 4 MiB] level-1 hits per chunk: min {hits.min()} median {np.median(hits):.0f} max {hits.max()}")


def test_fixture_text_of_the_300k_set_sits_below_the_dense_threshold():
    """plain text under S300: close to the 1024 hits of a dense chunk, (nearly) never above -- what threshold_stream starts from"""
    hits = ss.level1_counts(ss.S300, ss.text(ss.S300, HOST_BYTES)[:4 << 20])
    print(f"\n[S300 text, 4 MiB] level-1 hits per chunk: min {hits.min()} median {np.median(hits):.0f} max {hits.max()}")
    assert 850 < np.median(hits) <= ss.DENSE_HITS and np.count_nonzero(hits > ss.DENSE_HITS) * 20 < hits.size


def test_fixture_threshold_stream_straddles_the_dense_threshold():
    data, hits = ss.threshold_stream()
    ss.check_threshold(hits)                                   # (the builder has asserted it; said again where a reader looks for it)
    assert data.size >= 33 << 20 and hits.size == data.size // ss.CHUNK
    assert np.count_nonzero(ss.want(ss.pattern_file(ss.S300), data)) > 10000
    dense = hits > ss.DENSE_HITS
    print(f"\n[threshold stream] {hits.size} chunks, {np.count_nonzero(dense)} above 1024, {np.count_nonzero(dense[1:] != dense[:-1])} changes of side, "
          f"{np.count_nonzero(np.abs(hits - 1024.5) < 8)} within 8 of the threshold")


@pytest.mark.parametrize("target", ss.DENSITIES)
def test_fixture_density_streams_reach_their_density(target):
    data, want, density = ss.density_stream(target)
    assert data.size == ss.BIG and 0.8 * target <= density <= 1.25 * target and density == np.count_nonzero(want) / data.size
    print(f"\n[density stream {target}] achieved {density:.5f}")


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_fixture_one_byte_patterns_make_the_stream_dense(k):
    pf, data, want = ss.one_byte_set(k, HOST_BYTES)
    density = np.count_nonzero(want) / data.size
    print(f"\n[{k} one-byte patterns] density {density:.4f}")
    assert density > k / 100                          # every one of these bytes is about one byte in 75 of the text


def test_compiled_set_round_trip_of_the_large_set(tmp_path):
    """PFACX_saveCompiled / PFACX_loadCompiled of S300 on host-only handles: the same facts, the same filter and hash tables, the
    same CPU result."""
    a = ss.host_handle(ss.S300)
    path = str(tmp_path / "s300.pfacx")
    a.saveCompiled(path)
    b = api.PFAC.createHostOnly()
    try:
        b.loadCompiled(path)
        ia, ib = a.info(), b.info()
        for field, _ in api.PFACX_info._fields_:
            if field not in ("structSize", "deviceTableBytes", "deviceScratchBytes", "multiProcessorCount", "hasDevice"):
                assert getattr(ia, field) == getattr(ib, field), field
        assert ia.numOfPatterns == ss.S300 and ia.numOfStates > 4_500_000 and ia.filterTailGlobalEntries > 0
        for which in (api.PFACX_TABLE_HASH_ROWPTR, api.PFACX_TABLE_HASH_VALPTR, api.PFACX_TABLE_INITIAL_ROW, api.PFACX_TABLE_FILTER_GRAM3,
                      api.PFACX_TABLE_FILTER_SHORT, api.PFACX_TABLE_FILTER_LADDER, api.PFACX_TABLE_FILTER_FINAL3, api.PFACX_TABLE_CHAIN,
                      api.PFACX_TABLE_FILTER_GRAM1, api.PFACX_TABLE_FILTER_PREFIX4, api.PFACX_TABLE_FILTER_TAIL, api.PFACX_TABLE_FILTER_TAIL_GLOBAL,
                      api.PFACX_TABLE_FILTER_SKIP, api.PFACX_TABLE_PREFIX_PATTERN):
            ta, tb = a.table(which), b.table(which)
            assert ta.size == tb.size and np.array_equal(ta, tb), which
        data = ss.text(ss.S300, HOST_BYTES)
        b.setPlatform(api.PFAC_PLATFORM_CPU_OMP)
        assert_same(b.match_host_array(data), ss.want(ss.pattern_file(ss.S300), data), "loaded set, CPU_OMP")
    finally:
        b.destroy()
