"""Caseless pattern sets (PFACX_READ_NOCASE) on the CPU platforms: host-only handles, no device needed.

The definition (include/pfac_ext.h) is checked as it is written: a caseless handle's tables, dump and PFACX_getInfo equal those of a plain
handle loaded from the folded pattern bytes, and every host match call equals the oracle on the folded set over the folded input (and a
brute force over `bytes.lower()`).  Also: the bytes around the fold range, duplicates that folding makes, the caller's buffer left alone,
re-reading without the flag, compiled files of both kinds, unknown flag bits."""

import os

import numpy as np
import pytest

from oracle import binding as ob
from pfac_amd import api
from tests import allmatch_ref as ref
from tests import nocase_ref as nc

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
PERFS = [(api.PFAC_TIME_DRIVEN, "dense"), (api.PFAC_SPACE_DRIVEN, "hashed")]
READ_FLAGS = [(0, "plain"), (api.PFACX_READ_STRICT, "strict"), (api.PFACX_READ_STRIP_CR, "strip-cr"),
              (api.PFACX_READ_STRICT | api.PFACX_READ_STRIP_CR, "strict+strip-cr")]
TABLES = [api.PFACX_TABLE_INITIAL_ROW, api.PFACX_TABLE_FILTER_GRAM3, api.PFACX_TABLE_FILTER_SHORT, api.PFACX_TABLE_FILTER_LADDER,
          api.PFACX_TABLE_FILTER_FINAL3, api.PFACX_TABLE_FILTER_GRAM1, api.PFACX_TABLE_FILTER_PREFIX4, api.PFACX_TABLE_FILTER_TAIL,
          api.PFACX_TABLE_FILTER_TAIL_GLOBAL, api.PFACX_TABLE_FILTER_SKIP, api.PFACX_TABLE_CHAIN, api.PFACX_TABLE_PREFIX_PATTERN]


@pytest.fixture(scope="module")
def sets():
    return nc.mixed_sets()


def caseless(raw, flags=0, perf=api.PFAC_TIME_DRIVEN, platform=api.PFAC_PLATFORM_CPU):
    h = api.PFAC.createHostOnly()
    h.setPerfMode(perf)
    h.setPlatform(platform)
    h.readPatternFromMemoryEx(raw, flags | api.PFACX_READ_NOCASE)
    return h


def plain(raw, flags=0, perf=api.PFAC_TIME_DRIVEN, platform=api.PFAC_PLATFORM_CPU):
    h = api.PFAC.createHostOnly()
    h.setPerfMode(perf)
    h.setPlatform(platform)
    h.readPatternFromMemoryEx(raw, flags)
    return h


def oracle_folded(workdir, name, pats, data):
    """the oracle's result on the folded set over the folded input"""
    pf = nc.write_patterns(os.path.join(workdir, "nocase_" + name + ".pat"), [nc.fold(p) for p in pats])
    o = ob.Oracle(pf, hashed=False)
    try:
        return o.match(nc.fold_array(data))
    finally:
        o.close()


def brute_longest(pats, data):
    """longest match per position by brute force over bytes.lower() (the highest ID of patterns that fold to the same bytes)"""
    fp = [nc.fold(p) for p in pats]
    pos, ids = ref.brute_all(fp, np.frombuffer(nc.fold(bytes(data)), dtype=np.uint8))
    out = np.zeros(len(data), dtype=np.int32)
    first = np.ones(pos.size, dtype=bool)
    first[1:] = pos[1:] != pos[:-1]
    out[pos[first]] = ids[first]
    return out


def info_fields(info):
    return {name: getattr(info, name) for name, _ in api.PFACX_info._fields_}        # every field before caseInsensitive


@pytest.mark.parametrize("perf,perfname", PERFS)
@pytest.mark.parametrize("flags,flagname", READ_FLAGS)
@pytest.mark.parametrize("name", ["example", "c2", "c3"])
def test_tables_equal_those_of_the_folded_set(sets, tmp_path, name, flags, flagname, perf, perfname):
    pats, _ = sets[name]
    raw = nc.pattern_bytes(pats, crlf=bool(flags & api.PFACX_READ_STRIP_CR))
    a = caseless(raw, flags, perf)
    b = plain(nc.fold(raw), flags, perf)
    try:
        assert a.caseInsensitive() == 1 and b.caseInsensitive() == 0
        assert info_fields(a.info()) == info_fields(b.info())
        ref_tables = [api.PFACX_TABLE_DENSE] if perf == api.PFAC_TIME_DRIVEN else [api.PFACX_TABLE_HASH_ROWPTR, api.PFACX_TABLE_HASH_VALPTR]
        for which in TABLES + ref_tables:
            assert np.array_equal(a.table(which), b.table(which)), which
        da, db = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
        a.dumpTransitionTable(da)
        b.dumpTransitionTable(db)
        assert open(da, "rb").read() == open(db, "rb").read()
        assert a.info().numOfPatterns == len(pats)
    finally:
        a.destroy()
        b.destroy()


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("perf,perfname", PERFS)
@pytest.mark.parametrize("name", ["example", "c2", "c3", "edges"])
def test_host_calls_equal_the_folded_set_over_the_folded_input(sets, workdir, name, perf, perfname, platform, pname):
    pats, data = nc.edge_set() if name == "edges" else sets[name]
    want = oracle_folded(workdir, name, pats, data)
    if data.size <= (64 << 10):
        assert np.array_equal(brute_longest(pats, data), want)
    assert np.count_nonzero(want) > 0
    keep = data.copy()
    h = caseless(nc.pattern_bytes(pats), 0, perf, platform)
    try:
        assert np.array_equal(h.match_host_array(data), want)
        assert np.array_equal(data, keep)
        n = int(data.size)
        ids, pos = np.full(n, -9, dtype=np.int32), np.full(n, -9, dtype=np.int32)
        _, count = h.matchFromHostReduce(data.ctypes.data, n, ids.ctypes.data, pos.ctypes.data)
        nz = np.flatnonzero(want)
        assert count == nz.size and np.array_equal(pos[:count], nz) and np.array_equal(ids[:count], want[nz])
        assert np.array_equal(data, keep)
        # batches: cuts at random places, some of them inside planted patterns
        rng = np.random.Generator(np.random.PCG64(n))
        cuts = np.unique(np.concatenate([[0, n], rng.integers(0, n, size=40)])).astype(np.uint64)
        got = h.match_batch_host_array(data, cuts)
        exp = np.concatenate([oracle_folded(workdir, name + "_seg", pats, data[int(s):int(e)]) if e > s else np.zeros(0, np.int32)
                              for s, e in zip(cuts[:-1], cuts[1:])])
        assert np.array_equal(got, exp)
        assert np.array_equal(data, keep)
        # all matches: the folded set's list
        fp = [nc.fold(p) for p in pats]
        apos, aids = h.match_all_host_array(data)
        epos, eids = ref.expand_longest(fp, want)
        assert np.array_equal(apos, epos) and np.array_equal(aids, eids)
        assert np.array_equal(data, keep)
    finally:
        h.destroy()


@pytest.mark.parametrize("workers", [1, 3, 8])
def test_multi_worker_calls_fold_their_slices(sets, workdir, workers):
    pats, data = sets["c3"]
    data = data.copy()
    n = int(data.size)
    rng = np.random.Generator(np.random.PCG64(workers))
    longs = [p for p in pats if len(p) >= 12]
    for i in range(1, workers):
        b = (n * i // workers) // 1024 * 1024
        p = np.frombuffer(nc.flip_case(longs[i % len(longs)], rng), dtype=np.uint8)
        data[b - p.size // 2:b - p.size // 2 + p.size] = p            # across a slice boundary, in a case the set does not have
    want = oracle_folded(workdir, "multi", pats, data)
    keep = data.copy()
    for perf, _ in PERFS:
        h = caseless(nc.pattern_bytes(pats), 0, perf)
        try:
            got = np.full(n, -9, dtype=np.int32)
            h.matchFromHostMultiGPU(data.ctypes.data, n, got.ctypes.data, devices=list(range(workers)))
            assert np.array_equal(got, want)
            ids, pos = np.full(n, -9, dtype=np.int32), np.full(n, -9, dtype=np.int32)
            _, count = h.matchFromHostReduceMultiGPU(data.ctypes.data, n, ids.ctypes.data, pos.ctypes.data, devices=list(range(workers)))
            nz = np.flatnonzero(want)
            assert count == nz.size and np.array_equal(pos[:count], nz) and np.array_equal(ids[:count], want[nz])
            assert np.array_equal(data, keep)
        finally:
            h.destroy()


def test_bytes_around_the_fold_range_stay_distinct():
    pats = [bytes([c]) + b"q" for c in nc.FOLD_EDGES] + [b"Aq"]
    h = caseless(nc.pattern_bytes(pats))
    try:
        assert h.info().numOfPatterns == len(pats)
        data = np.frombuffer(b"".join(bytes([c]) + b"Q " for c in nc.FOLD_EDGES) + b"aQ AQ", dtype=np.uint8)
        got = h.match_host_array(data)
        for k in range(len(nc.FOLD_EDGES)):
            assert got[3 * k] == k + 1                                   # each byte only matches its own pattern
        base = 3 * len(nc.FOLD_EDGES)
        assert got[base] == len(pats) and got[base + 3] == len(pats)
        assert np.count_nonzero(got) == len(nc.FOLD_EDGES) + 2
    finally:
        h.destroy()


@pytest.mark.parametrize("platform,pname", PLATFORMS)
def test_patterns_equal_after_folding_are_duplicates(platform, pname):
    h = caseless(nc.pattern_bytes(nc.DUPLICATES), platform=platform)
    try:
        assert h.info().numOfPatterns == 4
        data = np.frombuffer(b"GET /A get /a GeT x", dtype=np.uint8)
        got = h.match_host_array(data)
        assert got[0] == 4 and got[7] == 4 and got[14] == 2               # 'get /a' under ID 4, 'get' under ID 2
        assert np.count_nonzero(got) == 3
        pos, ids = h.match_all_host_array(data)
        assert pos.tolist() == [0, 0, 7, 7, 14] and ids.tolist() == [4, 2, 4, 2, 2]   # each pattern listed once
        assert h.table(api.PFACX_TABLE_PREFIX_PATTERN).tolist() == [0, 0, 0, 0, 2]
    finally:
        h.destroy()


def test_reading_without_the_flag_is_case_sensitive_again():
    raw = nc.pattern_bytes([b"Hello", b"WORLD"])
    data = np.frombuffer(b"hello HELLO Hello world WORLD", dtype=np.uint8)
    h = caseless(raw)
    try:
        assert np.count_nonzero(h.match_host_array(data)) == 5
        h.readPatternFromMemory(raw)
        assert h.caseInsensitive() == 0
        got = h.match_host_array(data)
        assert np.flatnonzero(got).tolist() == [12, 24] and got[12] == 1 and got[24] == 2
        h.readPatternFromMemoryEx(raw, api.PFACX_READ_NOCASE)
        assert h.caseInsensitive() == 1
        h.readPatternFromMemoryEx(raw, api.PFACX_READ_STRICT)
        assert h.caseInsensitive() == 0
    finally:
        h.destroy()


def test_reading_from_a_file_with_the_flag(tmp_path):
    path = str(tmp_path / "p.pat")
    with open(path, "wb") as f:
        f.write(b"AbC\r\nxYz\r\n")
    h = api.PFAC.createHostOnly()
    try:
        h.readPatternFromFileEx(path, api.PFACX_READ_NOCASE | api.PFACX_READ_STRIP_CR | api.PFACX_READ_STRICT)
        assert h.caseInsensitive() == 1
        got = h.match_host_array(np.frombuffer(b"abc ABC XYZ", dtype=np.uint8))
        assert np.flatnonzero(got).tolist() == [0, 4, 8] and got.tolist()[8] == 2
    finally:
        h.destroy()


def _version(path):
    with open(path, "rb") as f:
        return int.from_bytes(f.read(12)[8:12], "little")


@pytest.mark.parametrize("perf,perfname", PERFS)
def test_compiled_files_keep_the_flag(sets, workdir, tmp_path, perf, perfname):
    pats, data = sets["c3"]
    raw = nc.pattern_bytes(pats)
    want = oracle_folded(workdir, "compiled", pats, data)
    a = caseless(raw, 0, perf)
    b = plain(raw, 0, perf)
    c = api.PFAC.createHostOnly()
    try:
        pa, pb = str(tmp_path / "a.pfacx"), str(tmp_path / "b.pfacx")
        a.saveCompiled(pa)
        b.saveCompiled(pb)
        assert _version(pa) == 8 and _version(pb) == 7
        c.loadCompiled(pa)
        assert c.caseInsensitive() == 1
        assert np.array_equal(c.match_host_array(data), want)
        for which in TABLES:
            assert np.array_equal(a.table(which), c.table(which)), which
        c.loadCompiled(pb)                                               # and back: a case-sensitive file
        assert c.caseInsensitive() == 0
        assert np.array_equal(c.match_host_array(data), b.match_host_array(data))
        assert not np.array_equal(c.match_host_array(data), want)
        c.loadCompiled(pa)
        assert c.caseInsensitive() == 1
        # a caseless file whose pattern bytes are not folded is refused (and the handle stays as it was)
        p = str(tmp_path / "bad.pfacx")
        rawb = bytearray(open(pb, "rb").read())
        rawb[8:12] = (8).to_bytes(4, "little")
        open(p, "wb").write(bytes(rawb))
        assert any(0x41 <= x <= 0x5A for x in raw)
        assert c.loadCompiled(p, check=False) == api.STATUS.INVALID_PARAMETER
        assert c.caseInsensitive() == 1
    finally:
        a.destroy()
        b.destroy()
        c.destroy()


def test_unknown_flag_bits_are_still_refused(tmp_path):
    path = str(tmp_path / "p.pat")
    with open(path, "wb") as f:
        f.write(b"abc\n")
    h = api.PFAC.createHostOnly()
    try:
        for bad in (4, 16, 1 << 31, api.PFACX_READ_NOCASE | 4):
            assert h.readPatternFromMemoryEx(b"abc\n", bad, check=False) == api.STATUS.INVALID_PARAMETER
            assert h.readPatternFromFileEx(path, bad, check=False) == api.STATUS.INVALID_PARAMETER
        assert h.readPatternFromMemoryEx(b"abc\n", api.PFACX_READ_NOCASE | api.PFACX_READ_STRICT | api.PFACX_READ_STRIP_CR) == 0
    finally:
        h.destroy()


def test_device_calls_on_a_host_only_handle_still_say_so():
    h = caseless(b"abc\n")
    buf = np.zeros(16, dtype=np.uint8)
    try:
        assert h.matchFromDevice(buf.ctypes.data, 4, buf.ctypes.data, check=False) == api.STATUS.LIB_NOT_EXIST
    finally:
        h.destroy()
