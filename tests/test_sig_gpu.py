"""PFACX_sigMatchFromDevice / PFACX_sigPairsFromDevice / PFACX_sigMatchFromHost (GPU platform) against the models of tests/sig_ref.py: the table of
the host file (the compare edges at lengths 1 .. 64 with a mismatch only in the last byte and only in byte 0, wildcards first, last and everywhere
but the anchor, half bytes, the anchor in the middle, 0x0A outside the anchor, chains, identical signatures), the start and end bounds with the
buffer a slice of a larger tensor at every offset and length mod 4 between guard bytes that would complete a match, a class of 300, pair counts
around the frame's block, one list past a single grid pass, truncation, pair lists with ids and positions that must be ignored, overlapping
arrays, and a seeded random set of 200 signatures over 64 KiB.  All arrays are poisoned and carry guard words on both sides."""

import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import sig_ref as ref  # noqa: E402
from tests.sig_ref import test_the_models_agree_on_every_case  # noqa: E402,F401  (runs here too: sig_ref.py is not collected)

BLOCK = api.PFACX_SIG_BLOCK                     # scan_sig.hip: kSigBlock
PER_CU = api.PFACX_SIG_BLOCKS_PER_CU            # scan_passes.h: offsetBlocks takes eight blocks per compute unit at most
GUARD = 64
POISON = -5
INVALID, TRUNCATED = api.STATUS.INVALID_PARAMETER, api.STATUS.OUTPUT_TRUNCATED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def as_array(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)


def out_arrays(cap):
    return tuple(torch.full((GUARD + cap + GUARD,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))


def check_guards(arrays, cap, clean_from):
    """nothing in front of the arrays, at or behind capacity, or in [clean_from, capacity)"""
    for a in arrays:
        assert bool((a[:GUARD] == POISON).all()) and bool((a[GUARD + cap:] == POISON).all()), "wrote outside the arrays"
        assert bool((a[GUARD + clean_from:GUARD + cap] == POISON).all()), "wrote behind the list"


def device_input(data, in_offset=0, front=b"", behind=b""):
    """the input as a slice of a larger tensor: `front` right in front of it, `behind` right behind it, its first byte in_offset bytes behind a
    256-byte boundary (torch allocations are 256-byte aligned); without `behind` the tensor ENDS with the input's last byte -> (tensor, address)"""
    data = as_array(data)
    lead = 16 * ((len(front) + 15) // 16) + in_offset
    assert lead >= len(front)
    host = np.full(lead + data.size + len(behind), 0x2E, dtype=np.uint8)
    host[lead - len(front):lead] = as_array(front)
    host[lead:lead + data.size] = data
    host[lead + data.size:] = as_array(behind)
    d = torch.from_numpy(host).to("cuda:0")
    assert d.data_ptr() % 256 == 0
    return d, d.data_ptr() + lead


def device_sig(sg, d_in, address, n, capacity):
    """match_device -> (status, (pos, ids) of the entries written, the full length).  The arrays take the scan's unordered list below `size`; behind
    max(size, the list) and outside the arrays nothing may be written, and the input must stay untouched"""
    before = d_in.clone()
    d_ids, d_pos = out_arrays(capacity)
    st, total = sg.match_device(address, n, d_ids.data_ptr() + 4 * GUARD, d_pos.data_ptr() + 4 * GUARD, capacity, check=False)
    torch.cuda.synchronize()
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > capacity), (st, total, capacity)
    k = min(total, capacity)
    check_guards((d_ids, d_pos), capacity, min(capacity, max(k, n)))
    assert torch.equal(d_in, before), "the caller's input, or what lies around it, was modified"
    return st, (d_pos[GUARD:GUARD + k].cpu().numpy(), d_ids[GUARD:GUARD + k].cpu().numpy()), total


def device_pairs(sg, address, n, pair_ids, pair_pos, capacity):
    """pairs_device over a pair list on the host, guard words around the pair arrays too -> (status, (pos, ids), the full length)"""
    lists = []
    for a in (pair_ids, pair_pos):
        t = torch.full((GUARD + len(a) + GUARD,), POISON, dtype=torch.int32, device="cuda:0")
        t[GUARD:GUARD + len(a)] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
        lists.append(t)
    before = [t.clone() for t in lists]
    d_ids, d_pos = out_arrays(capacity)
    st, total = sg.pairs_device(address, n, lists[0].data_ptr() + 4 * GUARD, lists[1].data_ptr() + 4 * GUARD, len(pair_ids),
                                d_ids.data_ptr() + 4 * GUARD if capacity else None, d_pos.data_ptr() + 4 * GUARD if capacity else None, capacity,
                                check=False)
    torch.cuda.synchronize()
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > capacity), (st, total, capacity)
    k = min(total, capacity)
    check_guards((d_ids, d_pos), capacity, k)
    assert all(torch.equal(t, b) for t, b in zip(lists, before)), "the caller's pair list, or what lies around it, was modified"
    return st, (d_pos[GUARD:GUARD + k].cpu().numpy(), d_ids[GUARD:GUARD + k].cpu().numpy()), total


def longest_pairs(h, address, n):
    """the ordered longest pairs of the handle's anchors: what the pairs form takes"""
    d_ids, d_pos = (torch.full((n,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
    _, count = h.matchFromDeviceReduce(address, n, d_ids.data_ptr(), d_pos.data_ptr())
    torch.cuda.synchronize()
    return d_ids[:count].cpu().numpy(), d_pos[:count].cpu().numpy()


class Opened:
    """a GPU handle with a signature object over `sigs` ([(values, masks)]) and what the getter says"""

    def __init__(self, sigs, max_len=0):
        self.sigs = sigs
        self.h = api.PFAC.create()
        self.sg = self.h.sigOpen(*ref.csr_of(sigs), max_len)
        self.anchor_id, self.off, self.len = self.sg.anchors()
        want, _ = ref.model_anchors(sigs, max_len)
        assert all(g.tolist() == w.tolist() for g, w in zip((self.anchor_id, self.off, self.len), want))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.sg.close(check=False)
        self.h.destroy()

    def model(self, data, what):
        return ref.check_models(self.sigs, data, self.off, self.len, what)

    def all_forms(self, data, what, in_offset=0, front=b"", behind=b"", host_form=True):
        """the device form, the pairs form over the handle's own reduce list and the host form against the model -> the model's list"""
        data = as_array(data)
        n = int(data.size)
        want = self.model(data, what)
        d_in, address = device_input(data, in_offset, front, behind)
        st, got, total = device_sig(self.sg, d_in, address, n, max(n, int(want[0].size)) + 3)
        assert st == 0 and total == want[0].size, (what, total, want[0].size)
        ref.same(got, want, f"{what}/device")
        pair_ids, pair_pos = longest_pairs(self.h, address, n)
        st, got, total = device_pairs(self.sg, address, n, pair_ids, pair_pos, int(want[0].size) + 3)
        assert st == 0
        ref.same(got, want, f"{what}/pairs")
        if host_form:
            ref.same(self.sg.match_host_array(data), want, f"{what}/host form")             # the GPU platform: the pipelined pairs path
        return want


# ---------------------------------------------------------------- the table of the host file: the compare edges, wildcards, half bytes, chains


@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_in_all_three_forms(case):
    name, data = case[0], case[2]
    with Opened(ref.parse_lines(ref.case_lines(case))) as o:
        want = o.all_forms(data, name)
        if name in ref.WANT:
            ids, pos = ref.WANT[name]
            ref.same(want, (pos, ids), f"{name}: against the list worked out by hand")


@pytest.mark.parametrize("in_offset", [1, 2, 3])
def test_the_compare_edges_with_the_pointer_off_alignment(in_offset):
    """lengths 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 64 in every wildcard kind, a mismatch only in the last byte and only in byte 0 of each, the
    occurrences at every residue mod 4, the last one as the buffer's last bytes: the aligned dwords in front of in[0] and behind in[n - 1] must
    not be loaded whole"""
    with Opened(ref.parse_lines(ref.edge_lines())) as o:
        want = o.all_forms(ref.edge_input(), f"edges/offset {in_offset}", in_offset=in_offset, host_form=False)
        assert want[0].size >= 6 * len(ref.EDGE_LENGTHS)


# ---------------------------------------------------------------- start and end bounds

BOUND_LINES = [
    "5? 52 61 62 63 64",                                        # 1: anchor Rabcd at offset 1: at p = 0 it would start at -1
    "?? ?? 61 62 63 ?? ??",                                     # 2: anchor abc at offset 2, p = 1: -1 again, under wildcards
    "?? 61 62 63 64 ?? 2E",                                     # 3: starts at 0: the dword in front of in[0]
    "70 71 72 73 74 75 76 77 78 79 7A 7B 7? 65 66 67 68 ??",     # 4: ends exactly at n
    "65 66 67 68 ?? 6?",                                        # 5: would end at n + 1
    "65 66 67 68 ??",                                           # 6: ends exactly at n
]


def bound_input(n_mod_4):
    fill = next(f for f in range(4) if (26 + f) % 4 == n_mod_4)
    data = b"Rabcd" + b"." * (3 + fill) + b"pqrstuvwxyz{" + b"\x7c" + b"efgh" + b"X"
    assert len(data) % 4 == n_mod_4
    return data


@pytest.mark.parametrize("n_mod_4", [0, 1, 2, 3])
@pytest.mark.parametrize("in_offset", [0, 1, 2, 3])
def test_start_and_end_bounds_in_a_slice_between_guards(in_offset, n_mod_4):
    """guard bytes in front (..Q: it would complete signatures 1 and 2 at start -1) and behind (j: it would complete signature 5) must not count"""
    data = bound_input(n_mod_4)
    n = len(data)
    with Opened(ref.parse_lines(BOUND_LINES)) as o:
        assert o.off.tolist() == [0, 1, 2, 1, 0, 0, 0]
        want = o.all_forms(data, f"bounds/offset {in_offset}/n mod 4 = {n_mod_4}", in_offset=in_offset, front=b"..Q", behind=b"j...")
        assert sorted(zip(want[1].tolist(), want[0].tolist())) == [(3, 0), (4, n - 18), (6, n - 5)]
        # with the guards inside the buffer the three others occur: the guards are what the bounds keep out
        whole = b"..Q" + data + b"j..."
        ids = o.model(whole, "with the guards inside")[1].tolist()
        assert sorted(ids) == [1, 2, 3, 4, 5, 6]


# ---------------------------------------------------------------- classes and chains


def test_300_signatures_share_one_anchor_at_different_offsets():
    key = [0x4B, 0x45, 0x59, 0x21]
    sigs = [(np.array([0] * k + key + [0], dtype=np.uint8), np.array([0] * k + [0xFF] * 4 + [0], dtype=np.uint8)) for k in range(300)]
    rng = np.random.default_rng(7)
    data = rng.integers(0x61, 0x7B, 1024, dtype=np.uint8)
    for at in (5, 150, 400, 1020):
        data[at:at + 4] = key
    with Opened(sigs) as o:
        assert set(o.anchor_id[1:].tolist()) == {1} and o.off[1:].tolist() == list(range(300))
        want = o.all_forms(data, "a class of 300")
        assert want[0].size == 6 + 151 + 300 + 0, "the starts that fit: offsets 0 .. 5, 0 .. 150, all 300, none (the tail byte lies behind n)"
        assert want[1][:6].tolist() == [6, 5, 4, 3, 2, 1], "within one anchor ids descend"


def test_both_members_of_a_chain_fire_at_one_position():
    lines = ["61 62 ?? 64", "61 62 63 ?? 65", "61 62 ??", "61 62 63", "61 62 63 ?? 65"]
    with Opened(ref.parse_lines(lines)) as o:
        assert o.anchor_id.tolist() == [0, 1, 2, 1, 2, 2] and o.len.tolist() == [0, 2, 3, 2, 3, 3]
        want = o.all_forms(b"abcde abxd abc", "a chain of two")
        assert (want[1][:5].tolist(), want[0][:5].tolist()) == ([5, 4, 2, 3, 1], [0, 0, 0, 0, 0]), "the longer anchor first, ids descending, twins both"


# ---------------------------------------------------------------- block and grid edges

RUN_LINES = ["61 ?? 61", "61 ?? ?? 62"]                          # every 'a' is a pair; the second one never holds


@pytest.mark.parametrize("pairs", [BLOCK - 1, BLOCK, BLOCK + 1])
def test_pair_counts_around_one_block(pairs):
    with Opened(ref.parse_lines(RUN_LINES)) as o:
        want = o.all_forms(b"a" * pairs, f"{pairs} pairs")
        assert want[0].size == pairs - 2


def test_one_pair_more_than_a_single_grid_pass():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pairs = PER_CU * cus * BLOCK + 1
    data = np.full(pairs, 0x61, dtype=np.uint8)
    with Opened(ref.parse_lines(RUN_LINES)) as o:
        d_in, address = device_input(data)
        st, (pos, ids), total = device_sig(o.sg, d_in, address, pairs, pairs)
        assert st == 0 and total == pairs - 2
        assert np.array_equal(pos, np.arange(pairs - 2)) and bool((ids == 1).all())
        pair_ids, pair_pos = longest_pairs(o.h, address, pairs)
        assert pair_ids.size == pairs
        st, (pos, ids), total = device_pairs(o.sg, address, pairs, pair_ids, pair_pos, pairs)
        assert st == 0 and total == pairs - 2
        assert np.array_equal(pos, np.arange(pairs - 2)) and bool((ids == 1).all())


# ---------------------------------------------------------------- capacity


def test_truncation_in_the_pairs_form_and_the_host_form():
    case = next(c for c in ref.CASES if c[0] == "an-anchor-is-a-prefix-of-another")
    data = as_array(case[2])
    n = int(data.size)
    with Opened(ref.parse_lines(case[1])) as o:
        want = o.model(data, case[0])
        total = int(want[0].size)
        assert total > 3
        d_in, address = device_input(data)
        pair_ids, pair_pos = longest_pairs(o.h, address, n)
        for cap in (0, total - 1, total):
            st, got, full = device_pairs(o.sg, address, n, pair_ids, pair_pos, cap)            # (the helper checks the guard words)
            assert (st, full) == (TRUNCATED if cap < total else 0, total)
            ref.same(got, (want[0][:cap], want[1][:cap]), f"pairs/capacity {cap}")
            ids, pos = (np.full(GUARD + cap + GUARD, -7, dtype=np.int32) for _ in range(2))
            st, full = o.sg.match_host(data.ctypes.data, n, ids.ctypes.data + 4 * GUARD if cap else None, pos.ctypes.data + 4 * GUARD if cap else None,
                                       cap, check=False)
            assert (st, full) == (TRUNCATED if cap < total else 0, total)
            ref.same((pos[GUARD:GUARD + cap], ids[GUARD:GUARD + cap]), (want[0][:cap], want[1][:cap]), f"host/capacity {cap}")
            assert all(bool((a[:GUARD] == -7).all()) and bool((a[GUARD + cap:] == -7).all()) for a in (ids, pos)), "wrote at or behind capacity"
        # the device form takes the scan's list first: it refuses capacity < size
        d_ids, d_pos = out_arrays(n)
        st, _ = o.sg.match_device(address, n, d_ids.data_ptr() + 4 * GUARD, d_pos.data_ptr() + 4 * GUARD, n - 1, check=False)
        assert st == INVALID
        check_guards((d_ids, d_pos), n, 0)


# ---------------------------------------------------------------- the pairs form: the caller's list


def test_pairs_with_ids_and_positions_that_give_nothing_and_overlapping_arrays():
    lines = ["61 62 ?? 64", "?? 63 64 65"]
    data = as_array(b"abcde abcd")
    n = int(data.size)
    with Opened(ref.parse_lines(lines)) as o:
        want = o.model(data, "pairs")
        d_in, address = device_input(data)
        good_ids, good_pos = longest_pairs(o.h, address, n)
        F = int(o.anchor_id.max())
        assert F == 2 and good_ids.size >= 3
        # between the good pairs: id 0, id F + 1, position -1, position size; each gives nothing
        pair_ids = np.concatenate([[0, F + 1, 1, 1], good_ids, [0, F + 1, 2]]).astype(np.int32)
        pair_pos = np.concatenate([[0, 0, -1, -1], good_pos, [n - 1, n - 1, n]]).astype(np.int32)
        st, got, total = device_pairs(o.sg, address, n, pair_ids, pair_pos, int(want[0].size) + 3)
        assert st == 0
        ref.same(got, want, "a list with pairs that give nothing")
        # output arrays that overlap the list are refused, and nothing is written
        t = torch.full((4 * n,), POISON, dtype=torch.int32, device="cuda:0")
        t[:good_ids.size] = torch.from_numpy(good_ids)
        t[n:n + good_pos.size] = torch.from_numpy(good_pos)
        before = t.clone()
        base, count = t.data_ptr(), int(good_ids.size)
        for d_ids, d_pos in ((base, base + 8 * n), (base + 8 * n, base + 4 * n), (base + 4 * (count - 1), base + 8 * n), (base + 8 * n, base + 4 * (n + count - 1))):
            st, _ = o.sg.pairs_device(address, n, base, base + 4 * n, count, d_ids, d_pos, n, check=False)
            assert st == INVALID
        torch.cuda.synchronize()
        assert torch.equal(t, before)
        st, total = o.sg.pairs_device(address, n, base, base + 4 * n, count, base + 8 * n, base + 12 * n, n, check=False)
        assert (st, total) == (0, want[0].size), "arrays that only touch are fine"
        st, total = o.sg.pairs_device(address, n, None, None, 0, None, None, 0, check=False)
        assert (st, total) == (0, 0), "no pairs"


def test_the_tables_are_counted_and_freed_with_the_object():
    sigs = ref.parse_lines(["61 62 ?? 64", "?? 63 64 65 66"])
    h = api.PFAC.create()
    try:
        before = h.info().deviceTableBytes
        sg = h.sigOpen(*ref.csr_of(sigs))
        loaded = h.info().deviceTableBytes                       # the anchors' own tables
        data = as_array(b"abcd")
        d_in, address = device_input(data)
        device_sig(sg, d_in, address, 4, 8)
        mine = 16 * 2 + 4 * (2 + 2) + 4 * 2 * (1 + 2)            # 16 bytes per signature, sigOff[F + 2], value and mask dwords
        assert h.info().deviceTableBytes - loaded >= mine
        h.trim()
        assert h.info().deviceTableBytes - loaded >= mine, "PFACX_trim keeps the tables of an object"
        sg.close()
        assert h.info().deviceTableBytes == loaded and loaded >= before
    finally:
        h.destroy()


# ---------------------------------------------------------------- the seeded random case


def test_200_random_signatures_over_64_kib():
    sigs, data = ref.random_case()
    with Opened(sigs) as o:
        want = o.all_forms(data, "random")
        assert 100 <= want[0].size <= 50000


# ---------------------------------------------------------------- the example


def test_sig_example_builds_and_runs():
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "sig_example"], check=True, stdout=subprocess.PIPE)
    p = subprocess.run([os.path.join(ROOT, "examples", "sig_example")], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    assert b"self-check passed" in p.stdout and b"signature 2 starts at 21" in p.stdout
