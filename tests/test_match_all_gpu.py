"""PFACX_matchAllFromDevice / PFACX_matchAllBatchFromDevice / PFACX_matchAllFromHost (GPU platform) against all-match lists
computed without the library's trie (tests/allmatch_ref.py): every kernel variant, walker, perf and texture mode; sizes on both sides
of the small-call switch; guard words behind capacity; truncation; the fast path of sets without nested prefixes; batches; scratch
reuse; pair counts around the wave and the block, a capacity inside a chain, more pairs than one grid pass takes; the example program."""

import hashlib
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from pfac_amd import workloads as wl  # noqa: E402
from tests import allmatch_ref as ref  # noqa: E402
from tests.gpu_helpers import MODES, VARIANTS, make_handle, oracle_match  # noqa: E402
from tests.test_match_all_host import A_RUN, _small_sets, write_patterns  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


def device_all(h, data, capacity=None, in_offset=0):
    """matchAllFromDevice with poisoned output arrays of capacity + GUARD entries -> (status, count, pos, ids) of the written pairs;
    the guard words behind capacity must stay untouched"""
    n = int(data.size)
    cap = n * max(1, h.info().maxMatchesPerPosition) if capacity is None else int(capacity)
    d_in = torch.zeros(n + in_offset + 64, dtype=torch.uint8, device="cuda:0")
    d_in[in_offset:in_offset + n] = torch.from_numpy(np.ascontiguousarray(data)).to("cuda:0")
    d_ids = torch.full((cap + GUARD,), -5, dtype=torch.int32, device="cuda:0")
    d_pos = torch.full((cap + GUARD,), -5, dtype=torch.int32, device="cuda:0")
    st, cnt = h.matchAllFromDevice(d_in.data_ptr() + in_offset, n, d_ids.data_ptr(), d_pos.data_ptr(), cap, check=False)
    torch.cuda.synchronize()
    ids, pos = d_ids.cpu().numpy(), d_pos.cpu().numpy()
    assert np.all(ids[cap:] == -5) and np.all(pos[cap:] == -5), "wrote behind capacity"
    w = min(cnt, cap)
    return st, cnt, pos[:w], ids[:w]


def check_list(got_pos, got_ids, want_pos, want_ids, what):
    assert got_pos.size == want_pos.size, f"{what}: {got_pos.size} pairs, want {want_pos.size}"
    if not (np.array_equal(got_pos, want_pos) and np.array_equal(got_ids, want_ids)):
        bad = np.nonzero((got_pos != want_pos) | (got_ids != want_ids))[0]
        raise AssertionError(f"{what}: {bad.size} pairs differ, first at {bad[0]}: got ({got_pos[bad[0]]}, {got_ids[bad[0]]}) "
                             f"want ({want_pos[bad[0]]}, {want_ids[bad[0]]})")


@pytest.fixture(scope="module")
def small_sets(workdir):
    return _small_sets(workdir)


@pytest.fixture(scope="module")
def nested_sets(workloads, workdir):
    """C5 / C6-style sets with nested prefixes: the small C3 / C5 workloads plus prefixes of some of their patterns"""
    out = {}
    for name in ("c3", "c5"):
        w = workloads[name]
        pats = [ln for ln in open(w.pattern_file, "rb").read().split(b"\n")[:-1]]
        extra = [p[:k] for p in pats[:300] for k in (1, 3, 6, 12) if k < len(p)]
        allp = list(dict.fromkeys(pats + extra))
        pf = write_patterns(os.path.join(workdir, "allgpu_" + name + ".pat"), allp)
        data = w.data[:(1 << 20)]
        want = ref.expand_longest(allp, oracle_match(pf, data))
        out[name] = (pf, allp, data, want)
    return out


@pytest.mark.parametrize("perf,tex,mode_name", MODES)
@pytest.mark.parametrize("variant,vname", VARIANTS)
@pytest.mark.parametrize("name", ["c3", "c5"])
def test_all_from_device_every_variant_and_mode(nested_sets, name, variant, vname, perf, tex, mode_name):
    pf, pats, data, (want_pos, want_ids) = nested_sets[name]
    h = make_handle(pf, perf, tex, variant)
    try:
        assert h.info().maxMatchesPerPosition > 1
        st, n, pos, ids = device_all(h, data)
        assert st == api.STATUS.SUCCESS and n == want_pos.size
        check_list(pos, ids, want_pos, want_ids, f"{name}/{vname}/{mode_name}")
    finally:
        h.destroy()


@pytest.mark.parametrize("walker", [api.PFACX_WALKER_AUTO, api.PFACX_WALKER_WINDOW, api.PFACX_WALKER_STAGE, api.PFACX_WALKER_VETO])
def test_all_from_device_every_walker(nested_sets, walker):
    for name in ("c3", "c5"):
        pf, pats, data, (want_pos, want_ids) = nested_sets[name]
        h = make_handle(pf, api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
        try:
            h.setWalker(walker)
            _, _, pos, ids = device_all(h, data)
            check_list(pos, ids, want_pos, want_ids, f"{name}/walker {walker}")
        finally:
            h.destroy()


@pytest.mark.parametrize("name", ["c2-nested", "c5", "a-run", "get-admin", "one-byte", "bytes-00-ff", "duplicates", "whole-input"])
def test_small_sets_equal_brute_force(small_sets, name):
    pf, pats, data = small_sets[name]
    want_pos, want_ids = ref.brute_all(pats, data)
    for perf, tex, mode_name in MODES:
        h = make_handle(pf, perf, tex, api.PFACX_KERNEL_AUTO)
        try:
            st, n, pos, ids = device_all(h, data)
            assert st == api.STATUS.SUCCESS
            check_list(pos, ids, want_pos, want_ids, f"{name}/{mode_name}")
            _, _, pos, ids = device_all(h, data, in_offset=3)                       # misaligned input
            check_list(pos, ids, want_pos, want_ids, f"{name}/{mode_name}/misaligned")
            _, _, pos, ids = device_all(h, data[:1])                                # one byte
            w1 = ref.brute_all(pats, data[:1])
            check_list(pos, ids, w1[0], w1[1], f"{name}/{mode_name}/1 byte")
        finally:
            h.destroy()


@pytest.mark.parametrize("size_mib", [8, 48])
def test_both_sides_of_the_small_call_switch(nested_sets, size_mib):
    pf, pats, _, _ = nested_sets["c3"]
    n = size_mib << 20
    data = wl.http_stream(n, wl.http_message_pool(wl.snort_patterns(3000), pool_size=512, embed_fraction=0.2))
    want_pos, want_ids = ref.expand_longest(pats, oracle_match(pf, data, omp=True))
    h = make_handle(pf, api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        st, cnt, pos, ids = device_all(h, data, capacity=n)
        assert st == api.STATUS.SUCCESS and cnt == want_pos.size
        check_list(pos, ids, want_pos, want_ids, f"c3-nested/{size_mib} MiB")
    finally:
        h.destroy()


def test_hostile_input_truncated_then_exact(workdir):
    """a..a x 8 over runs of a: up to 8 pairs per position, capacity == size truncates"""
    pf = write_patterns(os.path.join(workdir, "allgpu_arun.pat"), A_RUN)
    n = 1 << 20
    rng = np.random.Generator(np.random.PCG64(9))
    data = np.full(n, ord("a"), dtype=np.uint8)
    data[rng.integers(0, n, n // 50)] = ord("b")
    want_pos, want_ids = ref.expand_longest(A_RUN, oracle_match(pf, data, omp=True))
    assert want_pos.size > 4 * n
    h = make_handle(pf, api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        st, cnt, pos, ids = device_all(h, data, capacity=n)
        assert st == api.STATUS.OUTPUT_TRUNCATED and cnt == want_pos.size
        check_list(pos, ids, want_pos[:n], want_ids[:n], "a-run/truncated")
        st, cnt, pos, ids = device_all(h, data, capacity=cnt)
        assert st == api.STATUS.SUCCESS and cnt == want_pos.size
        check_list(pos, ids, want_pos, want_ids, "a-run/exact")
    finally:
        h.destroy()


def test_c3_set_at_64_mib_equals_the_oracle_expanded(workdir):
    pats = wl.snort_patterns(30000)
    pf = wl.write_pattern_file(os.path.join(workdir, "allgpu_c3_30k.pat"), pats)
    n = 64 << 20
    data = wl.http_stream(n, wl.http_message_pool(pats))
    want_pos, want_ids = ref.expand_longest(pats, oracle_match(pf, data, omp=True))
    h = make_handle(pf, api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        assert h.info().maxMatchesPerPosition >= 2
        st, cnt, pos, ids = device_all(h, data, capacity=n)
        assert st == api.STATUS.SUCCESS
        check_list(pos, ids, want_pos, want_ids, "c3/64 MiB")
    finally:
        h.destroy()


def test_fast_path_equals_the_compacted_call(workloads):
    """C2 has no nested prefixes: the all-match list is the longest-match list"""
    w = workloads["c2"]
    h = make_handle(w.pattern_file, api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        assert h.info().maxMatchesPerPosition == 1
        n = w.data.size
        d_in = torch.from_numpy(w.data.copy()).to("cuda:0")
        d_ids = torch.full((n,), -5, dtype=torch.int32, device="cuda:0")
        d_pos = torch.full((n,), -5, dtype=torch.int32, device="cuda:0")
        _, k = h.matchFromDeviceReduce(d_in.data_ptr(), n, d_ids.data_ptr(), d_pos.data_ptr())
        st, cnt, pos, ids = device_all(h, w.data, capacity=n)
        assert st == api.STATUS.SUCCESS and cnt == k
        check_list(pos, ids, d_pos.cpu().numpy()[:k], d_ids.cpu().numpy()[:k], "c2 fast path")
    finally:
        h.destroy()


def test_all_from_host_on_the_gpu_platform_in_several_pieces(nested_sets):
    pf, pats, _, _ = nested_sets["c3"]
    n = (40 << 20) + 17                                   # more than one 16 Mi / 32 Mi host piece
    data = wl.http_stream(n, wl.http_message_pool(wl.snort_patterns(3000), pool_size=512, embed_fraction=0.2))
    want_pos, want_ids = ref.expand_longest(pats, oracle_match(pf, data, omp=True))
    h = make_handle(pf, api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        h.setPlatform(api.PFAC_PLATFORM_GPU)
        pos, ids = h.match_all_host_array(data)
        check_list(pos, ids, want_pos, want_ids, "host path, GPU platform")
    finally:
        h.destroy()


def _batch_shapes(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = rng.integers(0, 40, n // 10 + 16)
    offs = np.concatenate([[0], np.cumsum(lens)])
    offs = offs[offs < n]
    return {
        "random-0..40": np.concatenate([offs, [n]]).astype(np.uint64),
        "1-byte": np.arange(n + 1, dtype=np.uint64),
        "empty-ends": np.array([0, 0, 0, n // 3, n // 3, n, n], dtype=np.uint64),
        "one": np.array([0, n], dtype=np.uint64),
    }


def device_all_batch(h, data, offs, capacity=None):
    n = int(data.size)
    cap = n * max(1, h.info().maxMatchesPerPosition) if capacity is None else int(capacity)
    d_in = torch.from_numpy(np.ascontiguousarray(data)).to("cuda:0")
    d_offs = torch.from_numpy(offs.astype(np.int64)).to("cuda:0")
    d_ids = torch.full((cap + GUARD,), -5, dtype=torch.int32, device="cuda:0")
    d_pos = torch.full((cap + GUARD,), -5, dtype=torch.int32, device="cuda:0")
    d_seg = torch.full((offs.size + 4,), -5, dtype=torch.int64, device="cuda:0")
    st, cnt = h.matchAllBatchFromDevice(d_in.data_ptr(), n, d_offs.data_ptr(), offs.size - 1, d_ids.data_ptr(), d_pos.data_ptr(), cap,
                                        d_seg.data_ptr(), check=False)
    torch.cuda.synchronize()
    ids, pos, seg = d_ids.cpu().numpy(), d_pos.cpu().numpy(), d_seg.cpu().numpy()
    assert np.all(ids[cap:] == -5) and np.all(pos[cap:] == -5) and np.all(seg[offs.size:] == -5)
    w = min(cnt, cap)
    return st, cnt, pos[:w], ids[:w], seg[:offs.size]


def batch_reference(pats, data, offs):
    pos, ids, first = [], [], [0]
    for k in range(offs.size - 1):
        s, e = int(offs[k]), int(offs[k + 1])
        p, i = ref.brute_all(pats, data[s:e]) if e > s else (np.zeros(0, np.int32), np.zeros(0, np.int32))
        pos.append(p + s)
        ids.append(i)
        first.append(first[-1] + p.size)
    return np.concatenate(pos).astype(np.int32), np.concatenate(ids).astype(np.int32), np.array(first, dtype=np.int64)


@pytest.mark.parametrize("name", ["c2-nested", "a-run", "one-byte", "get-admin", "c2"])
def test_batch_equals_brute_force_per_segment(small_sets, name):
    pf, pats, data = small_sets[name]
    data = data[:6000]
    for perf, tex, mode_name in MODES[::3]:
        h = make_handle(pf, perf, tex, api.PFACX_KERNEL_AUTO)
        try:
            for shape, offs in _batch_shapes(data.size, seed=3).items():
                want_pos, want_ids, want_first = batch_reference(pats, data, offs)
                st, cnt, pos, ids, seg = device_all_batch(h, data, offs)
                assert st == api.STATUS.SUCCESS and cnt == want_pos.size, f"{name}/{shape}"
                check_list(pos, ids, want_pos, want_ids, f"{name}/{mode_name}/{shape}")
                assert np.array_equal(seg, want_first), f"{name}/{mode_name}/{shape}: segFirst"
        finally:
            h.destroy()


@pytest.fixture(scope="module")
def token_handle(workdir):
    """a, ab, abc: the input of tests/allmatch_ref.py: nested_tokens gives a known number of longest pairs with chains of 3, 2 and 1"""
    pf = write_patterns(os.path.join(workdir, "allgpu_tokens.pat"), ref.NESTED_TOKEN_PATTERNS)
    h = make_handle(pf, api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    yield h
    h.destroy()


def device_all_poisoned(h, data, capacity, room):
    """matchAllFromDevice into poisoned arrays of `room` entries, of which the call may write `capacity` -> (status, count, pos, ids), whole arrays"""
    d_in = torch.from_numpy(np.ascontiguousarray(data)).to("cuda:0")
    d_ids = torch.full((room,), -5, dtype=torch.int32, device="cuda:0")
    d_pos = torch.full((room,), -5, dtype=torch.int32, device="cuda:0")
    st, cnt = h.matchAllFromDevice(d_in.data_ptr(), int(data.size), d_ids.data_ptr(), d_pos.data_ptr(), int(capacity), check=False)
    torch.cuda.synchronize()
    return st, cnt, d_pos.cpu().numpy(), d_ids.cpu().numpy()


@pytest.mark.parametrize("pairs", [63, 64, 65, 255, 256, 257])
def test_pair_counts_around_the_wave_and_the_block(token_handle, pairs):
    """the expansion's block of 256 pairs, its waves of 64, and a capacity that cuts inside a chain"""
    data, want_pos, want_ids, _, pair_first = ref.nested_tokens(pairs)
    total = int(pair_first[-1])
    st, cnt, pos, ids = device_all(token_handle, data)
    assert st == api.STATUS.SUCCESS and cnt == total
    check_list(pos, ids, want_pos, want_ids, f"{pairs} pairs")


@pytest.mark.parametrize("pairs,cut_pair", [(63, None), (64, None), (65, None), (255, None), (256, None), (257, None), (258, 256), (384, 256)])
def test_capacity_cuts_inside_a_chain(workdir, pairs, cut_pair):
    """The call takes no capacity below the input's size, and a, ab, abc never list more entries than the input has bytes.  a, aa, aaa over
    "aaax" tokens (and a last "a" or "aa": exactly `pairs` longest pairs) have the same chains of 3, 2, 1 and list 6 entries per 4 bytes.
    The capacity is one entry into the chain of cut_pair -- pair 256: the first chain of the expansion's second block -- or, without one, the
    smallest capacity >= size that is not the first entry of a pair.  The slots below it are exact, the rest stay poison, the full length
    is returned"""
    pats = [b"a", b"aa", b"aaa"]
    data = np.frombuffer(b"aaax" * (pairs // 3) + b"aa"[:pairs % 3], dtype=np.uint8).copy()
    want_pos, want_ids = ref.brute_all(pats, data)
    total = want_pos.size
    first_of_pair = np.concatenate([[True], want_pos[1:] != want_pos[:-1]])
    assert int(first_of_pair.sum()) == pairs
    if cut_pair is None:
        cap = int(data.size)
        while first_of_pair[cap]:
            cap += 1
    else:
        cap = int(np.nonzero(first_of_pair)[0][cut_pair]) + 1
        assert not first_of_pair[cap]
    assert data.size <= cap < total
    h = make_handle(write_patterns(os.path.join(workdir, "allgpu_arun3.pat"), pats), api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        st, cnt, pos, ids = device_all_poisoned(h, data, cap, total + GUARD)
    finally:
        h.destroy()
    assert st == api.STATUS.OUTPUT_TRUNCATED and cnt == total
    check_list(pos[:cap], ids[:cap], want_pos[:cap], want_ids[:cap], f"{pairs} pairs, capacity {cap}")
    assert np.all(pos[cap:] == -5) and np.all(ids[cap:] == -5), "wrote at or behind capacity"


def test_batch_cut_at_the_block_edge_with_empty_segments(token_handle):
    """257 pairs; segments that start at pairs 0, 255 (three times: two empty segments), 256 and end at 257: segFirst against the
    offsets of the constructed list"""
    data, want_pos, want_ids, start, pair_first = ref.nested_tokens(257)
    first_pairs = [0, 255, 255, 255, 256]
    offs = np.array([int(start[k]) for k in first_pairs] + [data.size], dtype=np.uint64)
    st, cnt, pos, ids, seg = device_all_batch(token_handle, data, offs)
    assert st == api.STATUS.SUCCESS and cnt == want_pos.size
    check_list(pos, ids, want_pos, want_ids, "batch of 257 pairs")
    assert np.array_equal(seg, pair_first[first_pairs + [257]]), f"segFirst {seg}"


def test_more_pairs_than_one_grid_pass(token_handle):
    """600 000 longest pairs: more than eight blocks per compute unit of 256 take a pair each (524 288 on 256 compute units), so a block's
    range is 512 pairs and it makes two trips"""
    pairs = 600000
    data, want_pos, want_ids, _, pair_first = ref.nested_tokens(pairs)
    total = int(pair_first[-1])
    assert total == 1200000 and data.size == 1800000
    st, cnt, pos, ids = device_all_poisoned(token_handle, data, data.size, data.size + GUARD)       # (the call takes no capacity below the size)
    assert st == api.STATUS.SUCCESS and cnt == total
    assert np.all(pos[total:] == -5) and np.all(ids[total:] == -5), "wrote behind the list"
    pos, ids = pos[:total], ids[:total]
    check_list(pos[:1000], ids[:1000], want_pos[:1000], want_ids[:1000], "first 1000")
    check_list(pos[-1000:], ids[-1000:], want_pos[-1000:], want_ids[-1000:], "last 1000")
    digest = lambda a: hashlib.sha256(np.ascontiguousarray(a, dtype=np.int32).tobytes()).hexdigest()     # noqa: E731
    assert digest(pos) == digest(want_pos) and digest(ids) == digest(want_ids)


def test_scratch_reuse_and_trim(nested_sets, small_sets):
    pf, pats, data, (want_pos, want_ids) = nested_sets["c3"]
    h = make_handle(pf, api.PFAC_TIME_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO)
    try:
        _, _, pos, ids = device_all(h, data)
        check_list(pos, ids, want_pos, want_ids, "first call")
        small = data[:5000]
        w = ref.expand_longest(pats, oracle_match(pf, small))
        _, _, pos, ids = device_all(h, small)
        check_list(pos, ids, w[0], w[1], "smaller call")
        before = h.info().deviceScratchBytes
        h.trim()
        assert h.info().deviceScratchBytes < before
        _, _, pos, ids = device_all(h, data)
        check_list(pos, ids, want_pos, want_ids, "after trim")
    finally:
        h.destroy()


def test_example_program_prints_both_rules():
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "match_all_example"], check=True, stdout=subprocess.PIPE)
    p = subprocess.run([os.path.join(ROOT, "examples", "match_all_example")], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0, p.stderr.decode()
    assert "position 0: rule B (GET /admin)" in out and "position 0: rule A (GET)" in out
    assert out.index("position 0: rule B") < out.index("position 0: rule A")
