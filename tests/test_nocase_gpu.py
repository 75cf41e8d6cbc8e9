"""Caseless pattern sets (PFACX_READ_NOCASE) on the GPU: all twelve match entry points against the oracle on the folded set over the
folded input (include/pfac_ext.h), in every kernel variant, walker and table mode, with misaligned and odd-sized device input, guard words
around the outputs, and the caller's buffer -- device or host -- compared byte for byte before and after each call."""

import os
import subprocess

import numpy as np
import pytest

from pfac_amd import api
from pfac_amd import workloads as wl
from tests import allmatch_ref as ref
from tests import nocase_ref as nc
from tests.gpu_helpers import MODES, ROOT, VARIANTS, assert_same, oracle_match, torch

pytestmark = pytest.mark.gpu
GUARD = 64


def caseless_handle(pf, perf, tex, variant=api.PFACX_KERNEL_FILTER):
    h = api.PFAC.create()
    h.setPerfMode(perf)
    h.setTextureMode(tex)
    h.setKernelVariant(variant & 0xFF)
    if variant >> 8:
        h.setWalker(variant >> 8)
    h.readPatternFromFileEx(pf, api.PFACX_READ_NOCASE)
    return h


@pytest.fixture(scope="module")
def c3(workdir):
    """a mixed-case C3 set (file with the case as written, file with it folded) and a mixed-case stream of 40 MiB + 4321 bytes"""
    rng = np.random.Generator(np.random.PCG64(31))
    raw = wl.snort_patterns(3000)
    pats = [nc.flip_case(p, rng) for p in raw]
    pf = nc.write_patterns(os.path.join(workdir, "nocase_c3.pat"), pats)
    ff = nc.write_patterns(os.path.join(workdir, "nocase_c3_folded.pat"), [nc.fold(p) for p in pats])
    data = nc.flip_array(wl.http_stream((40 << 20) + 4321, wl.http_message_pool(raw, pool_size=512, embed_fraction=0.3)), rng)
    return pf, ff, pats, data


@pytest.fixture(scope="module")
def folded_oracle(c3):
    """the oracle of the folded set, loaded once (many small inputs)"""
    from oracle import binding as ob
    o = ob.Oracle(c3[1], hashed=False)
    yield o
    o.close()


@pytest.fixture(scope="module")
def c3_want(c3):
    _, ff, _, data = c3
    return oracle_match(ff, nc.fold_array(data), omp=True)


def to_device(data, offset=0):
    d = torch.zeros(int(data.size) + offset + GUARD, dtype=torch.uint8, device="cuda:0")
    if data.size:
        d[offset:offset + data.size] = torch.from_numpy(np.ascontiguousarray(data)).to("cuda:0")
    return d


def poisoned(n, dtype=torch.int32, value=-5):
    return torch.full((n + 2 * GUARD,), value, dtype=dtype, device="cuda:0")


def unguard(t, n, value=-5):
    a = t.cpu().numpy()
    assert np.all(a[:GUARD] == value) and np.all(a[GUARD + n:] == value), "wrote outside the output"
    return a[GUARD:GUARD + n]


def full_device(h, data, offset=0):
    n = int(data.size)
    d_in = to_device(data, offset)
    before = d_in.cpu().numpy()
    out = poisoned(n)
    h.matchFromDevice(d_in.data_ptr() + offset, n, out.data_ptr() + 4 * GUARD)
    torch.cuda.synchronize()
    assert np.array_equal(d_in.cpu().numpy(), before), "the caller's device input changed"
    return unguard(out, n)


def reduce_device(h, data, offset=0):
    n = int(data.size)
    d_in = to_device(data, offset)
    before = d_in.cpu().numpy()
    ids, pos = poisoned(n), poisoned(n)
    _, count = h.matchFromDeviceReduce(d_in.data_ptr() + offset, n, ids.data_ptr() + 4 * GUARD, pos.data_ptr() + 4 * GUARD)
    torch.cuda.synchronize()
    assert np.array_equal(d_in.cpu().numpy(), before), "the caller's device input changed"
    ids, pos = unguard(ids, n), unguard(pos, n)
    return ids[:count], pos[:count]


def dense(ids, pos, n):
    out = np.zeros(n, dtype=np.int32)
    out[pos] = ids
    return out


@pytest.mark.parametrize("variant,vname", VARIANTS)
@pytest.mark.parametrize("perf,tex,mname", MODES)
def test_device_calls_every_variant_and_mode(c3, c3_want, perf, tex, mname, variant, vname):
    pf, _, _, data = c3
    small, want_small = data[: (1 << 20) + 13], c3_want[: (1 << 20) + 13]
    h = caseless_handle(pf, perf, tex, variant)
    try:
        assert h.caseInsensitive() == 1
        assert_same(full_device(h, small, 3), want_small, f"{mname}/{vname} matchFromDevice")
        ids, pos = reduce_device(h, small, 5)
        assert_same(dense(ids, pos, small.size), want_small, f"{mname}/{vname} matchFromDeviceReduce")
        assert np.all(np.diff(pos) > 0)
        if vname in ("filter", "auto"):                # both sides of the 32 MiB small-call switch
            assert_same(full_device(h, data), c3_want, f"{mname}/{vname} matchFromDevice 40 MiB")
    finally:
        h.destroy()


@pytest.mark.parametrize("offset", list(range(1, 16)))
def test_misaligned_device_input_with_odd_sizes(c3, c3_want, folded_oracle, offset):
    pf, _, _, data = c3
    h = caseless_handle(pf, api.PFAC_SPACE_DRIVEN, api.PFAC_TEXTURE_ON, api.PFACX_KERNEL_AUTO)
    try:
        for n in (1, 7, 15, 16, 17, 31, 33, 4097 + 2 * offset, (256 << 10) + offset):
            assert_same(full_device(h, data[:n], offset), folded_oracle.match(nc.fold_array(data[:n])), f"offset {offset} size {n}")
        ids, pos = reduce_device(h, data[: (1 << 20) + offset], offset)
        assert_same(dense(ids, pos, (1 << 20) + offset), c3_want[: (1 << 20) + offset], f"reduce offset {offset}")
    finally:
        h.destroy()


def test_fold_of_every_byte_value(workdir):
    """every byte value, at every alignment: a one-byte pattern for every folded value but '\\n' -> the result says the folded byte"""
    pats = [bytes([b]) for b in range(256) if not 0x41 <= b <= 0x5A and b != 0x0A]
    pf = nc.write_patterns(os.path.join(workdir, "nocase_bytes.pat"), pats)
    idof = {p[0]: i + 1 for i, p in enumerate(pats)}
    idof[0x0A] = 0
    h = caseless_handle(pf, api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        data = np.tile(np.arange(256, dtype=np.uint8), 97)
        want = np.array([idof[b] for b in nc.fold_array(data)], dtype=np.int32)
        for offset in (0, 1, 2, 3, 4, 5, 8, 12, 15):
            for n in (data.size, data.size - 1, 255, 48, 33):
                assert_same(full_device(h, data[:n], offset), want[:n], f"offset {offset} size {n}")
    finally:
        h.destroy()


def test_batch_and_all_match_device_calls(c3, folded_oracle):
    pf, _, pats, data = c3
    n = 2 << 20
    data = data[:n].copy()
    rng = np.random.Generator(np.random.PCG64(8))
    longs = [p for p in pats if len(p) >= 10]
    cuts = [0]
    for k in range(1, 300):                                     # cuts inside planted patterns of a case the set does not have
        at = k * (n // 300)
        p = np.frombuffer(nc.flip_case(longs[k % len(longs)], rng), dtype=np.uint8)
        data[at:at + p.size] = p
        cuts.append(at + p.size // 2)
    cuts += list(rng.integers(0, n, size=200))
    offs = np.unique(np.array(cuts + [n], dtype=np.uint64))
    folded = nc.fold_array(data)
    want = np.concatenate([folded_oracle.match(folded[int(s):int(e)]) if e > s else np.zeros(0, np.int32) for s, e in zip(offs[:-1], offs[1:])])
    whole = folded_oracle.match(folded)
    fp = [nc.fold(p) for p in pats]
    for perf, tex, mname in MODES:
        h = caseless_handle(pf, perf, tex, api.PFACX_KERNEL_AUTO)
        try:
            d_in, d_off = to_device(data, 1), torch.from_numpy(offs.view(np.int64)).to("cuda:0")
            before = d_in.cpu().numpy()
            out = poisoned(n)
            h.matchBatchFromDevice(d_in.data_ptr() + 1, n, d_off.data_ptr(), offs.size - 1, out.data_ptr() + 4 * GUARD)
            torch.cuda.synchronize()
            assert_same(unguard(out, n), want, f"{mname} matchBatchFromDevice")
            ids, pos, first = poisoned(n), poisoned(n), poisoned(offs.size)
            _, count = h.matchBatchFromDeviceReduce(d_in.data_ptr() + 1, n, d_off.data_ptr(), offs.size - 1, ids.data_ptr() + 4 * GUARD,
                                                    pos.data_ptr() + 4 * GUARD, first.data_ptr() + 4 * GUARD)
            torch.cuda.synchronize()
            assert_same(dense(unguard(ids, n)[:count], unguard(pos, n)[:count], n), want, f"{mname} matchBatchFromDeviceReduce")
            seg_first = unguard(first, offs.size)
            assert np.array_equal(seg_first, np.searchsorted(np.flatnonzero(want), offs.astype(np.int64)))
            # all matches: whole buffer, then the batch form
            cap = n * max(1, h.info().maxMatchesPerPosition)
            aids, apos = poisoned(cap), poisoned(cap)
            st, cnt = h.matchAllFromDevice(d_in.data_ptr() + 1, n, aids.data_ptr() + 4 * GUARD, apos.data_ptr() + 4 * GUARD, cap)
            epos, eids = ref.expand_longest(fp, whole)
            assert st == 0 and cnt == epos.size
            assert np.array_equal(unguard(apos, cap)[:cnt], epos) and np.array_equal(unguard(aids, cap)[:cnt], eids)
            sf = poisoned(offs.size, torch.int64)
            st, cnt = h.matchAllBatchFromDevice(d_in.data_ptr() + 1, n, d_off.data_ptr(), offs.size - 1, aids.data_ptr() + 4 * GUARD,
                                                apos.data_ptr() + 4 * GUARD, cap, sf.data_ptr() + 8 * GUARD)
            bpos, bids = ref.expand_longest(fp, want)
            assert st == 0 and cnt == bpos.size
            assert np.array_equal(unguard(apos, cap)[:cnt], bpos) and np.array_equal(unguard(aids, cap)[:cnt], bids)
            # truncation: capacity == size, the count is the whole list
            small = 4096
            tid, tpos = poisoned(small), poisoned(small)
            st, cnt = h.matchAllFromDevice(d_in.data_ptr() + 1, small, tid.data_ptr() + 4 * GUARD, tpos.data_ptr() + 4 * GUARD, small)
            full_pos, full_ids = ref.expand_longest(fp, folded_oracle.match(folded[:small]))
            assert cnt == full_pos.size
            k = min(small, cnt)
            assert np.array_equal(unguard(tpos, small)[:k], full_pos[:k]) and np.array_equal(unguard(tid, small)[:k], full_ids[:k])
            assert st == (api.STATUS.OUTPUT_TRUNCATED if cnt > small else 0)
            assert np.array_equal(d_in.cpu().numpy(), before), "the caller's device input changed"
        finally:
            h.destroy()


@pytest.mark.parametrize("perf,tex,mname", MODES)
def test_host_calls_pinned_and_pageable(c3, c3_want, folded_oracle, perf, tex, mname):
    pf, _, _, data = c3
    n = int(data.size)
    h = caseless_handle(pf, perf, tex, api.PFACX_KERNEL_AUTO)
    try:
        for kind in ("pageable", "pinned"):
            h_in = torch.from_numpy(data.copy())
            h_out = torch.full((n,), -7, dtype=torch.int32)
            h_ids, h_pos = torch.full((n,), -7, dtype=torch.int32), torch.full((n,), -7, dtype=torch.int32)
            if kind == "pinned":
                h_in, h_out, h_ids, h_pos = h_in.pin_memory(), h_out.pin_memory(), h_ids.pin_memory(), h_pos.pin_memory()
            h.matchFromHost(h_in.data_ptr(), n, h_out.data_ptr())
            assert_same(h_out.numpy(), c3_want, f"{mname} {kind} matchFromHost")
            _, count = h.matchFromHostReduce(h_in.data_ptr(), n, h_ids.data_ptr(), h_pos.data_ptr())
            assert_same(dense(h_ids.numpy()[:count], h_pos.numpy()[:count], n), c3_want, f"{mname} {kind} matchFromHostReduce")
            assert np.array_equal(h_in.numpy(), data), "the caller's host input changed"
        part = data[: 3 << 20]
        offs = np.unique(np.concatenate([[0, part.size], np.random.Generator(np.random.PCG64(2)).integers(0, part.size, 500)])).astype(np.uint64)
        got = h.match_batch_host_array(part, offs)
        want = np.concatenate([folded_oracle.match(nc.fold_array(part[int(s):int(e)])) if e > s else np.zeros(0, np.int32)
                               for s, e in zip(offs[:-1], offs[1:])])
        assert_same(got, want, f"{mname} matchBatchFromHost")
        apos, aids = h.match_all_host_array(part)
        epos, eids = ref.expand_longest([nc.fold(p) for p in c3[2]], c3_want[: part.size])
        assert np.array_equal(apos, epos) and np.array_equal(aids, eids)
        assert np.array_equal(part, data[: 3 << 20])
    finally:
        h.destroy()


def test_a_big_host_call_and_a_big_device_call(c3):
    """~128 MiB: several staging pieces of the host path, one device call through the filter kernel"""
    pf, ff, _, data = c3
    big = np.concatenate([data, data, data])
    want = oracle_match(ff, nc.fold_array(big), omp=True)
    h = caseless_handle(pf, api.PFAC_SPACE_DRIVEN, api.PFAC_TEXTURE_ON, api.PFACX_KERNEL_AUTO)
    try:
        assert_same(h.match_host_array(big), want, "matchFromHost 120 MiB")
        assert_same(full_device(h, big, 7), want, "matchFromDevice 120 MiB")
    finally:
        h.destroy()


def test_multi_gpu_calls_on_device_zero(c3, c3_want):
    pf, _, pats, data = c3
    data = data.copy()
    n = int(data.size)
    rng = np.random.Generator(np.random.PCG64(4))
    longest = max(pats, key=len)
    for workers in (2, 3):
        for i in range(1, workers):
            cut = (n * i // workers) // 1024 * 1024
            p = np.frombuffer(nc.flip_case(longest, rng), dtype=np.uint8)
            data[cut - p.size // 2: cut - p.size // 2 + p.size] = p
    want = oracle_match(c3[1], nc.fold_array(data), omp=True)
    keep = data.copy()
    h = caseless_handle(pf, api.PFAC_SPACE_DRIVEN, api.PFAC_TEXTURE_ON, api.PFACX_KERNEL_AUTO)
    try:
        for devices in ([0], [0, 0], [0, 0, 0]):
            got = np.full(n, -7, dtype=np.int32)
            h.matchFromHostMultiGPU(data.ctypes.data, n, got.ctypes.data, devices)
            assert_same(got, want, f"multi-GPU devices {devices}")
            ids, pos = np.full(n, -7, dtype=np.int32), np.full(n, -7, dtype=np.int32)
            _, count = h.matchFromHostReduceMultiGPU(data.ctypes.data, n, ids.ctypes.data, pos.ctypes.data, devices)
            assert_same(dense(ids[:count], pos[:count], n), want, f"multi-GPU reduce devices {devices}")
        assert np.array_equal(data, keep)
    finally:
        h.destroy()


def test_scratch_is_counted_and_trimmed(c3):
    pf, _, _, data = c3
    h = caseless_handle(pf, api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF)
    try:
        before = h.info().deviceScratchBytes
        n = 3 << 20
        full_device(h, data[:n], 1)
        grown = h.info().deviceScratchBytes
        assert grown >= before + n
        h.trim()
        assert h.info().deviceScratchBytes <= grown - n
        # a case-sensitive set: no fold scratch at all
        h.readPatternFromFile(pf)
        full_device(h, data[:n], 1)
        assert h.info().deviceScratchBytes < n
    finally:
        h.destroy()


def test_case_sensitive_handles_are_unchanged(c3, c3_want):
    pf, _, _, data = c3
    part = data[: 4 << 20]
    want = oracle_match(pf, part)
    assert not np.array_equal(want, c3_want[: part.size])
    a = caseless_handle(pf, api.PFAC_SPACE_DRIVEN, api.PFAC_TEXTURE_ON, api.PFACX_KERNEL_AUTO)
    b = api.PFAC.create()
    try:
        b.setKernelVariant(api.PFACX_KERNEL_AUTO)
        b.readPatternFromFile(pf)
        assert b.caseInsensitive() == 0
        assert_same(full_device(a, part), c3_want[: part.size], "caseless")
        assert_same(full_device(b, part), want, "case-sensitive")
        assert_same(b.match_host_array(part), want, "case-sensitive host")
        a.readPatternFromFile(pf)                             # re-read without the flag
        assert_same(full_device(a, part), want, "re-read case-sensitive")
    finally:
        a.destroy()
        b.destroy()


def test_nocase_example_builds_and_runs():
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "nocase_example"], check=True, stdout=subprocess.PIPE)
    p = subprocess.run([os.path.join(ROOT, "examples", "nocase_example")], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0, p.stderr.decode()
    assert "caseInsensitive = 1" in out
    assert "position 10: rule 2 (Union Select)" in out and "position 16: rule 1 (select)" in out
    assert "position 42: rule 3 (/ETC/passwd)" in out and "position 55: rule 1 (select)" in out
    assert "input after the call: GET /?q=1 UNION SELECT pw FROM users; cat /etc/PASSWD; SeLeCt" in out
