"""PFACX_matchAllFromHost on the CPU platforms (host-only handles: no device needed) against an all-match list computed without
the library's trie (tests/allmatch_ref.py), PFACX_TABLE_PREFIX_PATTERN and maxMatchesPerPosition, compiled sets, truncation and the
argument checks of the three all-match calls."""

import ctypes as C
import os

import numpy as np
import pytest

from oracle import binding as ob
from pfac_amd import api
from pfac_amd import workloads as wl
from tests import allmatch_ref as ref

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
PERFS = [(api.PFAC_TIME_DRIVEN, "dense"), (api.PFAC_SPACE_DRIVEN, "hashed")]
A_RUN = [b"a" * k for k in range(1, 9)]


def write_patterns(path, pats):
    """a pattern file as the library reads it (duplicate lines allowed, unlike wl.write_pattern_file)"""
    with open(path, "wb") as f:
        f.write(b"".join(bytes(p) + b"\n" for p in pats))
    return path


def host_handle(pf, platform=api.PFAC_PLATFORM_CPU, perf=api.PFAC_TIME_DRIVEN):
    h = api.PFAC.createHostOnly()
    h.setPerfMode(perf)
    h.setPlatform(platform)
    h.readPatternFromFile(pf)
    return h


def _small_sets(workdir):
    """{name: (pattern list, input)} -- small enough for the brute force"""
    rng = np.random.Generator(np.random.PCG64(77))
    out = {}
    c2 = wl.random_patterns(300)
    d2 = wl.random_bytes(24 << 10, seed=5).copy()
    for p in c2[:60]:
        at = int(rng.integers(0, d2.size - 40))
        d2[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
    # nested prefixes on top of the random set: the chains the expansion follows
    nested = c2 + [p[:k] for p in c2[:40] for k in (3, 5, 7) if k < len(p)]
    nested = list(dict.fromkeys(nested))
    out["c2"] = (c2, d2)
    out["c2-nested"] = (nested, d2)
    p5 = wl.adversarial_patterns(120)
    out["c5"] = (p5, wl.adversarial_stream(16 << 10, wl.adversarial_pool(p5, pool_size=64)))
    out["a-run"] = (A_RUN, np.frombuffer(b"a" * 300 + b"b" + b"a" * 7 + b"ba", dtype=np.uint8))
    out["get-admin"] = ([b"GET", b"GET /admin"], np.frombuffer(b"GET /admin HTTP/1.1\r\nGET /index GET /admi", dtype=np.uint8))
    one = [b"q", b"Z", b"qu", b"quo", b"Zed", b"x"]
    out["one-byte"] = (one, rng.choice(np.frombuffer(b"qZuoedx ", dtype=np.uint8), size=5000))
    binary = [b"\x00", b"\x00\x00", b"\xff", b"\xff\xff\x00", b"\xff\xff", b"\x00\xff"]
    out["bytes-00-ff"] = (binary, rng.choice(np.array([0x00, 0xFF, 0x01], dtype=np.uint8), size=5000))
    out["duplicates"] = ([b"ab", b"abc", b"ab", b"b", b"abc", b"bc"], np.frombuffer(b"abcabcab bc abc", dtype=np.uint8))
    whole = b"the whole input"
    out["whole-input"] = ([whole, b"the", b"the whole", b"in"], np.frombuffer(whole, dtype=np.uint8))
    for name in list(out):
        pats, data = out[name]
        out[name] = (write_patterns(os.path.join(workdir, "all_" + name + ".pat"), pats), pats,
                     np.ascontiguousarray(data, dtype=np.uint8))
    return out


@pytest.fixture(scope="module")
def small_sets(workdir):
    return _small_sets(workdir)


SMALL = ["c2", "c2-nested", "c5", "a-run", "get-admin", "one-byte", "bytes-00-ff", "duplicates", "whole-input"]


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("perf,perfname", PERFS)
@pytest.mark.parametrize("name", SMALL)
def test_all_matches_equal_brute_force(small_sets, name, platform, pname, perf, perfname):
    pf, pats, data = small_sets[name]
    want_pos, want_ids = ref.brute_all(pats, data)
    h = host_handle(pf, platform, perf)
    try:
        pos, ids = h.match_all_host_array(data)
    finally:
        h.destroy()
    assert pos.size == want_pos.size, f"{name}/{pname}/{perfname}: {pos.size} pairs, want {want_pos.size}"
    assert np.array_equal(pos, want_pos) and np.array_equal(ids, want_ids), f"{name}/{pname}/{perfname}"


def test_get_admin_reports_both_rules(small_sets):
    pf, pats, data = small_sets["get-admin"]
    h = host_handle(pf)
    try:
        pos, ids = h.match_all_host_array(data)
    finally:
        h.destroy()
    assert list(zip(pos[:2].tolist(), ids[:2].tolist())) == [(0, 2), (0, 1)]      # GET /admin (rule B) first, then GET (rule A)


@pytest.mark.parametrize("name", SMALL)
def test_first_pair_of_each_position_is_the_longest_match(small_sets, name):
    pf, pats, data = small_sets[name]
    h = host_handle(pf, api.PFAC_PLATFORM_CPU_OMP)
    try:
        pos, ids = h.match_all_host_array(data)
        r_ids = np.full(data.size, -7, dtype=np.int32)
        r_pos = np.full(data.size, -7, dtype=np.int32)
        _, n = h.matchFromHostReduce(data.ctypes.data, data.size, r_ids.ctypes.data, r_pos.ctypes.data)
    finally:
        h.destroy()
    first = np.ones(pos.size, dtype=bool)
    first[1:] = pos[1:] != pos[:-1]
    assert np.array_equal(pos[first], r_pos[:n]) and np.array_equal(ids[first], r_ids[:n])
    assert np.all(np.diff(pos) >= 0)


@pytest.mark.parametrize("name", ["c1", "c2", "c3", "c5", "dense_hits", "binary"])
def test_workloads_equal_the_oracle_expanded(workloads, oracle_results, name):
    w = workloads[name]
    pats = [ln for ln in open(w.pattern_file, "rb").read().split(b"\n")[:-1]]
    want_pos, want_ids = ref.expand_longest(pats, oracle_results[name])
    h = host_handle(w.pattern_file, api.PFAC_PLATFORM_CPU_OMP)
    try:
        pos, ids = h.match_all_host_array(w.data)
    finally:
        h.destroy()
    assert np.array_equal(pos, want_pos) and np.array_equal(ids, want_ids), name


@pytest.mark.parametrize("name", SMALL)
def test_prefix_table_and_max_matches_per_position(small_sets, name):
    pf, pats, _ = small_sets[name]
    want_prefix, _, want_max = ref.prefix_table(pats)
    h = host_handle(pf)
    try:
        assert np.array_equal(h.table(api.PFACX_TABLE_PREFIX_PATTERN), want_prefix)
        assert h.info().maxMatchesPerPosition == want_max
    finally:
        h.destroy()


def test_prefix_table_of_the_c3_generator_set(workdir):
    pats = wl.snort_patterns(30000)
    pf = wl.write_pattern_file(os.path.join(workdir, "all_c3_30k.pat"), pats)
    want_prefix, _, want_max = ref.prefix_table(pats)
    h = host_handle(pf)
    try:
        got = h.table(api.PFACX_TABLE_PREFIX_PATTERN)
        assert np.array_equal(got, want_prefix)
        assert np.count_nonzero(got) > 0 and h.info().maxMatchesPerPosition == want_max >= 2
    finally:
        h.destroy()


def test_no_nested_prefixes_means_one_match_per_position(workdir):
    pf = write_patterns(os.path.join(workdir, "all_flat.pat"), [b"abc", b"bcd", b"xyz"])
    h = host_handle(pf)
    try:
        assert h.info().maxMatchesPerPosition == 1
        assert not np.any(h.table(api.PFACX_TABLE_PREFIX_PATTERN))
    finally:
        h.destroy()


@pytest.mark.parametrize("perf,perfname", PERFS)
@pytest.mark.parametrize("name", ["c2-nested", "a-run", "one-byte", "bytes-00-ff"])
def test_compiled_set_round_trip_keeps_the_all_match_tables(small_sets, tmp_path, name, perf, perfname):
    """The prefix table is not part of the compiled-set file: loadCompiled derives it from the trie again."""
    pf, pats, data = small_sets[name]
    want_prefix, _, want_max = ref.prefix_table(pats)
    want_pos, want_ids = ref.brute_all(pats, data)
    cf = str(tmp_path / (name + ".pfacset"))
    h = host_handle(pf, api.PFAC_PLATFORM_CPU, perf)
    try:
        h.saveCompiled(cf)
    finally:
        h.destroy()
    h = api.PFAC.createHostOnly()
    try:
        h.loadCompiled(cf)
        assert np.array_equal(h.table(api.PFACX_TABLE_PREFIX_PATTERN), want_prefix)
        assert h.info().maxMatchesPerPosition == want_max
        pos, ids = h.match_all_host_array(data)
        assert np.array_equal(pos, want_pos) and np.array_equal(ids, want_ids)
    finally:
        h.destroy()


@pytest.mark.parametrize("platform,pname", PLATFORMS)
def test_truncated_list_reports_the_full_count(small_sets, platform, pname):
    pf, pats, data = small_sets["a-run"]
    want_pos, want_ids = ref.brute_all(pats, data)
    assert want_pos.size > data.size
    h = host_handle(pf, platform)
    try:
        guard = 16
        ids = np.full(data.size + guard, -7, dtype=np.int32)
        pos = np.full(data.size + guard, -7, dtype=np.int32)
        st, n = h.matchAllFromHost(data.ctypes.data, data.size, ids.ctypes.data, pos.ctypes.data, data.size)
        assert st == api.STATUS.OUTPUT_TRUNCATED and n == want_pos.size
        assert np.array_equal(ids[:data.size], want_ids[:data.size]) and np.array_equal(pos[:data.size], want_pos[:data.size])
        assert np.all(ids[data.size:] == -7) and np.all(pos[data.size:] == -7)       # nothing behind capacity
        # exactly the full count: success
        ids = np.full(n, -7, dtype=np.int32)
        pos = np.full(n, -7, dtype=np.int32)
        st, n2 = h.matchAllFromHost(data.ctypes.data, data.size, ids.ctypes.data, pos.ctypes.data, n)
        assert st == api.STATUS.SUCCESS and n2 == n
        assert np.array_equal(ids, want_ids) and np.array_equal(pos, want_pos)
        with pytest.raises(api.PFACError):                                          # the numpy helper raises on truncation
            h.match_all_host_array(data, capacity=data.size)
    finally:
        h.destroy()


def test_argument_checks(small_sets):
    pf, _, data = small_sets["a-run"]
    lib = api.load_library()
    n = C.c_size_t(99)
    buf = np.zeros(data.size, dtype=np.int32)
    p, i, d = buf.ctypes.data, buf.ctypes.data, data.ctypes.data
    assert lib.PFACX_matchAllFromHost(None, d, data.size, i, p, data.size, C.byref(n)) == api.STATUS.INVALID_HANDLE
    assert lib.PFACX_matchAllFromDevice(None, d, data.size, i, p, data.size, C.byref(n)) == api.STATUS.INVALID_HANDLE
    h = api.PFAC.createHostOnly()
    try:
        assert lib.PFACX_matchAllFromHost(h._h, d, data.size, i, p, data.size, C.byref(n)) == api.STATUS.PATTERNS_NOT_READY
        h.readPatternFromFile(pf)
        for args in ((None, data.size, i, p), (d, data.size, None, p), (d, data.size, i, None)):
            assert lib.PFACX_matchAllFromHost(h._h, args[0], args[1], args[2], args[3], data.size, C.byref(n)) == api.STATUS.INVALID_PARAMETER
        assert lib.PFACX_matchAllFromHost(h._h, d, data.size, i, p, data.size, None) == api.STATUS.INVALID_PARAMETER
        assert lib.PFACX_matchAllFromHost(h._h, d, data.size, i, p, data.size - 1, C.byref(n)) == api.STATUS.INVALID_PARAMETER
        assert lib.PFACX_matchAllFromHost(h._h, d, 1 << 31, i, p, 1 << 31, C.byref(n)) == api.STATUS.INVALID_PARAMETER
        n.value = 99
        assert lib.PFACX_matchAllFromHost(h._h, d, 0, i, p, 0, C.byref(n)) == api.STATUS.SUCCESS and n.value == 0
        # the GPU forms on a host-only handle
        assert lib.PFACX_matchAllFromDevice(h._h, d, data.size, i, p, data.size, C.byref(n)) == api.STATUS.LIB_NOT_EXIST
        offs = np.array([0, data.size], dtype=np.uint64)
        seg = np.zeros(2, dtype=np.uint64)
        assert lib.PFACX_matchAllBatchFromDevice(h._h, d, data.size, offs.ctypes.data, 1, i, p, data.size, seg.ctypes.data,
                                                 C.byref(n)) == api.STATUS.LIB_NOT_EXIST
        assert lib.PFACX_matchAllBatchFromDevice(h._h, d, data.size, offs.ctypes.data, 0, i, p, data.size, seg.ctypes.data,
                                                 C.byref(n)) == api.STATUS.INVALID_PARAMETER
        assert lib.PFACX_matchAllBatchFromDevice(h._h, d, data.size, offs.ctypes.data, 1, i, p, data.size, None,
                                                 C.byref(n)) == api.STATUS.INVALID_PARAMETER
        assert lib.PFACX_matchAllBatchFromDevice(h._h, d, data.size, offs.ctypes.data, 1, i, p, data.size - 1, seg.ctypes.data,
                                                 C.byref(n)) == api.STATUS.INVALID_PARAMETER
        # the GPU platform on a host-only handle: no silent CPU fallback
        h.setPlatform(api.PFAC_PLATFORM_GPU, check=False)
        if h.info().platform == api.PFAC_PLATFORM_GPU:
            assert lib.PFACX_matchAllFromHost(h._h, d, data.size, i, p, data.size, C.byref(n)) == api.STATUS.LIB_NOT_EXIST
    finally:
        h.destroy()


def test_error_string_of_the_new_status():
    assert api.STATUS.OUTPUT_TRUNCATED == 10100
    assert api.error_string(api.STATUS.OUTPUT_TRUNCATED).startswith("PFACX_STATUS_OUTPUT_TRUNCATED")
    assert api.error_string(10999).startswith("PFAC_STATUS_INTERNAL_ERROR")


def test_info_field_is_appended_after_the_existing_ones():
    names = [f for f, _ in api.PFACX_info._fields_]
    assert names[-1] == "maxMatchesPerPosition" and names[-2] == "filterSkipTags"


def test_oracle_binding_agrees_on_the_longest_pairs(small_sets):
    """the brute force and the oracle agree on the longest pattern of each position (the reference lists are consistent)"""
    pf, pats, data = small_sets["c2-nested"]
    o = ob.Oracle(pf)
    try:
        longest = o.match(data)
    finally:
        o.close()
    a = ref.expand_longest(pats, longest)
    b = ref.brute_all(pats, data)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
