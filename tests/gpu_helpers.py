"""Helpers shared by the GPU test files (tests/test_full_result.py, test_reduce.py, test_host_paths.py, test_hostile.py,
test_kernel_variants.py, test_full_size_digests.py, test_multi_gpu.py, test_tiled_edges_gpu.py, test_filter_edges_gpu.py with its fixtures
tests/filter_edges.py, checked on the host by test_filter_edges_host.py): handles in every table mode and kernel variant, poisoned
device buffers, the committed reference digests, event-timed launches.  Test infrastructure only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODES = [
    (api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF, "dense-global"),
    (api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_ON, "dense-buffer"),
    (api.PFAC_SPACE_DRIVEN, api.PFAC_TEXTURE_OFF, "hash-global"),
    (api.PFAC_SPACE_DRIVEN, api.PFAC_TEXTURE_ON, "hash-buffer"),
]
STAGE = api.PFACX_WALKER_STAGE << 8             # make_handle: the walker of the full-result filter kernel rides in the variant's second byte
VETO = api.PFACX_WALKER_VETO << 8
VARIANTS = [(api.PFACX_KERNEL_FILTER, "filter"), (api.PFACX_KERNEL_FILTER | STAGE, "filter-stage"), (api.PFACX_KERNEL_FILTER | VETO, "filter-veto"),
            (api.PFACX_KERNEL_NAIVE, "naive"), (api.PFACX_KERNEL_AUTO, "auto"), (api.PFACX_KERNEL_REFTABLE, "reftable")]
WALKERS = [(api.PFACX_WALKER_WINDOW, "window"), (api.PFACX_WALKER_STAGE, "stage")]


def perf_asserts():
    """Assertions that compare wall-clock or event times (one kernel variant against another, pinned against pageable buffers, a GB/s
    floor) run only when PFAC_PERF_FLOORS is set: the default `-m gpu` run asserts result equality and nothing else -- like the
    reference's own self-check (PFAC/test/omp_PFAC.cpp:420-439) -- so that a busy or power-capped box cannot turn it red.  The rates
    are printed either way."""
    return bool(os.environ.get("PFAC_PERF_FLOORS"))


def make_handle(pattern_file, perf, tex, variant=api.PFACX_KERNEL_FILTER):
    h = api.PFAC.create()
    h.setPerfMode(perf)
    h.setTextureMode(tex)
    h.setKernelVariant(variant & 0xFF)
    if variant >> 8:
        h.setWalker(variant >> 8)                  # (a whole session under one walker: PFAC_TEST_WALKER, pfac_amd/api.py)
    h.readPatternFromFile(pattern_file)
    return h


def _device_input(data, in_offset, front, behind):
    """the input in_offset bytes into a device buffer: `front` in every byte before it, `behind` (then zeros) in the 64 after it"""
    n = int(data.size)
    host = np.zeros(n + in_offset + 64, dtype=np.uint8)
    host[:in_offset] = front
    host[in_offset:in_offset + n] = data
    host[in_offset + n:in_offset + n + len(behind)] = np.frombuffer(behind, dtype=np.uint8)
    return torch.from_numpy(host).to("cuda:0")


def device_match(h, data, in_offset=0, out_offset=0, front=0, behind=b""):
    """matchFromDevice with poisoned output; optional byte/int offsets to misalign the pointers.  front / behind: what lies around the
    input in device memory (bytes that would complete a match if a kernel read them as input)."""
    n = int(data.size)
    d_in = _device_input(data, in_offset, front, behind)
    d_out = torch.full((n + out_offset + 64,), -5, dtype=torch.int32, device="cuda:0")
    h.matchFromDevice(d_in.data_ptr() + in_offset, n, d_out.data_ptr() + 4 * out_offset)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(out[:out_offset] == -5) and np.all(out[out_offset + n:] == -5), "wrote outside [0, n)"
    return out[out_offset:out_offset + n]


def device_reduce(h, data, in_offset=0, front=0, behind=b""):
    """matchFromDeviceReduce: (positions, ids) of the pairs.  Both arrays have room for a pair per position and 64 poisoned ints on
    either side, which stay as they were."""
    n = int(data.size)
    d_in = _device_input(data, in_offset, front, behind)
    d_ids = torch.full((n + 128,), -5, dtype=torch.int32, device="cuda:0")
    d_pos = torch.full((n + 128,), -5, dtype=torch.int32, device="cuda:0")
    _, count = h.matchFromDeviceReduce(d_in.data_ptr() + in_offset, n, d_ids.data_ptr() + 256, d_pos.data_ptr() + 256)
    torch.cuda.synchronize()
    ids, pos = d_ids.cpu().numpy(), d_pos.cpu().numpy()
    assert 0 <= count <= n, count
    for a in (ids, pos):
        assert np.all(a[:64] == -5) and np.all(a[64 + n:] == -5), "wrote outside the n pairs of the caller's arrays"
    return pos[64:64 + count], ids[64:64 + count]


def assert_pairs(pairs, want, what):
    """the pairs of a compacted-output call == the non-zero results of the full vector `want`, in position order"""
    pos, ids = pairs
    nz = np.flatnonzero(want)
    if not (pos.size == nz.size and np.array_equal(pos, nz) and np.array_equal(ids, want[nz])):
        raise AssertionError(f"{what}: {pos.size} pairs, want {nz.size}; first positions {pos[:4].tolist()} want {nz[:4].tolist()}")


def assert_same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"{what}: {bad.size} mismatches; first at {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}")


def digest_record(workload, slice_index, size_mib):
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "full_digests.json")))
    for r in doc["records"]:
        if (r["workload"], r["slice"], r["size_mib"]) == (workload, slice_index, size_mib):
            return r
    raise KeyError((workload, slice_index, size_mib))


def digests(workload, size_mib):
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "full_digests.json")))
    return {r["slice"]: r for r in doc["records"] if r["workload"] == workload and r["size_mib"] == size_mib}


def timed_match(h, data, steps=5):
    from pfac_amd import hiprt
    n = int(data.size)
    d_in = torch.from_numpy(np.ascontiguousarray(data)).to("cuda:0")
    d_out = torch.full((n,), -5, dtype=torch.int32, device="cuda:0")
    h.matchFromDevice(d_in.data_ptr(), n, d_out.data_ptr())
    torch.cuda.synchronize()
    a, b = hiprt.Event(), hiprt.Event()
    a.record(0)
    for _ in range(steps):
        h.matchFromDevice(d_in.data_ptr(), n, d_out.data_ptr())
    b.record(0)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), n / (a.elapsed_ms(b) / steps / 1e3) / 1e9


def oracle_match(pf, data, omp=False):
    from oracle import binding as ob
    o = ob.Oracle(pf, hashed=False)
    want = o.match(data, omp=omp)
    o.close()
    return want


def run_bench(*flags, timeout=900):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags, "--full", "--no-cpu-baseline", "--no-other-configs", "--pmc", "off"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    return json.loads([l for l in p.stdout.decode().splitlines() if l.startswith("{")][-1])

def o_prefix(pf, data):
    from oracle import binding as ob
    o = ob.Oracle(pf, dense=False, hashed=True)
    try:
        return o.match(data, hashed=True, omp=True)
    finally:
        o.close()
