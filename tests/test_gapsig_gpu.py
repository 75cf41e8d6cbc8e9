"""PFACX_gapsigMatchFromDevice / PFACX_gapsigPairsFromDevice / PFACX_gapsigMatchFromHost (GPU platform) against the models of
tests/gapsig_ref.py: the table of the host file (gap widths up to slack 63 over 1, 2, 3 and 63 gaps, the anchor in every part, a class of 300,
the owner rule, the smallest end, part lengths 1 .. 20, half bytes, 0x0A), the buffer a slice of a larger tensor at every pointer offset mod 4
between guard bytes that would complete an embedding, pair counts around the frame's block, one pairs list past a single grid pass over a small
input, truncation with and without the end array, pair lists with ids and positions that must be ignored, overlapping arrays, and a seeded
random set of 200 signatures over 64 KiB.  All arrays are poisoned and carry guard words on both sides; the input must stay untouched."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import gapsig_ref as ref  # noqa: E402
from tests.gapsig_ref import test_the_models_agree_on_every_case  # noqa: E402,F401  (runs here too: gapsig_ref.py is not collected)

BLOCK = api.PFACX_GAPSIG_BLOCK                  # scan_gapsig.hip: kGapSigBlock
PER_CU = api.PFACX_GAPSIG_BLOCKS_PER_CU         # scan_passes.h: offsetBlocks takes eight blocks per compute unit at most
GUARD = 64
POISON = -5
INVALID, TRUNCATED = api.STATUS.INVALID_PARAMETER, api.STATUS.OUTPUT_TRUNCATED


def as_array(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)


def out_arrays(cap):
    return tuple(torch.full((GUARD + cap + GUARD,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(3))


def check_guards(arrays, cap, clean_from):
    """nothing in front of the arrays, at or behind capacity, or in [clean_from, capacity)"""
    for a in arrays:
        assert bool((a[:GUARD] == POISON).all()) and bool((a[GUARD + cap:] == POISON).all()), "wrote outside the arrays"
        assert bool((a[GUARD + clean_from:GUARD + cap] == POISON).all()), "wrote behind the list"


def device_input(data, in_offset=0, front=b"", behind=b""):
    """the input as a slice of a larger tensor: `front` right in front of it, `behind` right behind it, its first byte in_offset bytes behind a
    256-byte boundary; without `behind` the tensor ENDS with the input's last byte -> (tensor, address)"""
    data = as_array(data)
    lead = 16 * ((len(front) + 15) // 16) + in_offset
    host = np.full(lead + data.size + len(behind), 0x2E, dtype=np.uint8)
    host[lead - len(front):lead] = as_array(front)
    host[lead:lead + data.size] = data
    host[lead + data.size:] = as_array(behind)
    d = torch.from_numpy(host).to("cuda:0")
    assert d.data_ptr() % 256 == 0
    return d, d.data_ptr() + lead


def taken(arrays, k):
    d_ids, d_pos, d_end = arrays
    return tuple(a[GUARD:GUARD + k].cpu().numpy() for a in (d_pos, d_ids, d_end))


def device_gapsig(sg, d_in, address, n, capacity, with_end=True):
    """match_device -> (status, (pos, ids, end) written, the full length).  d_ids / d_pos take the scan's unordered list below `size`; d_end is
    only ever written below the list; outside the arrays nothing may be written, and the input must stay untouched"""
    before = d_in.clone()
    arrays = out_arrays(capacity)
    ptr = [a.data_ptr() + 4 * GUARD for a in arrays]
    st, total = sg.match_device(address, n, ptr[0], ptr[1], ptr[2] if with_end else None, capacity, check=False)
    torch.cuda.synchronize()
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > capacity), (st, total, capacity)
    k = min(total, capacity)
    check_guards(arrays[:2], capacity, min(capacity, max(k, n)))
    check_guards(arrays[2:], capacity, k if with_end else 0)
    assert torch.equal(d_in, before), "the caller's input, or what lies around it, was modified"
    return st, taken(arrays, k), total


def device_pairs(sg, address, n, pair_ids, pair_pos, capacity, with_end=True):
    """pairs_device over a pair list on the host, guard words around the pair arrays too -> (status, (pos, ids, end), the full length)"""
    lists = []
    for a in (pair_ids, pair_pos):
        t = torch.full((GUARD + len(a) + GUARD,), POISON, dtype=torch.int32, device="cuda:0")
        t[GUARD:GUARD + len(a)] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
        lists.append(t)
    before = [t.clone() for t in lists]
    arrays = out_arrays(capacity)
    ptr = [a.data_ptr() + 4 * GUARD if capacity else None for a in arrays]
    st, total = sg.pairs_device(address, n, lists[0].data_ptr() + 4 * GUARD, lists[1].data_ptr() + 4 * GUARD, len(pair_ids),
                                ptr[0], ptr[1], ptr[2] if with_end else None, capacity, check=False)
    torch.cuda.synchronize()
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > capacity), (st, total, capacity)
    k = min(total, capacity)
    check_guards(arrays[:2], capacity, k)
    check_guards(arrays[2:], capacity, k if with_end else 0)
    assert all(torch.equal(t, b) for t, b in zip(lists, before)), "the caller's pair list, or what lies around it, was modified"
    return st, taken(arrays, k), total


def longest_pairs(h, address, n):
    """the ordered longest pairs of the handle's anchors: what the pairs form takes"""
    d_ids, d_pos = (torch.full((n,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
    _, count = h.matchFromDeviceReduce(address, n, d_ids.data_ptr(), d_pos.data_ptr())
    torch.cuda.synchronize()
    return d_ids[:count].cpu().numpy(), d_pos[:count].cpu().numpy()


class Opened:
    """a GPU handle with a gapped-signature object over `sigs` and what the getter says"""

    def __init__(self, sigs, max_len=0):
        self.sigs = sigs
        self.h = api.PFAC.create()
        self.sg = self.h.gapsigOpen(*ref.csr_of(sigs), max_len)
        self.anchors = self.sg.anchors()
        want, _ = ref.model_anchors(sigs, max_len)
        assert all(g.tolist() == w.tolist() for g, w in zip(self.anchors, want))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.sg.close(check=False)
        self.h.destroy()

    def model(self, data, what):
        return ref.check_models(self.sigs, data, self.anchors, what)

    def all_forms(self, data, what, in_offset=0, front=b"", behind=b"", host_form=True, want=None):
        """the device form, the pairs form over the handle's own reduce list and the host form against the model -> the model's list"""
        data = as_array(data)
        n = int(data.size)
        want = self.model(data, what) if want is None else want
        d_in, address = device_input(data, in_offset, front, behind)
        st, got, total = device_gapsig(self.sg, d_in, address, n, max(n, int(want[0].size)) + 3)
        assert st == 0 and total == want[0].size, (what, total, want[0].size)
        ref.same(got, want, f"{what}/device")
        pair_ids, pair_pos = longest_pairs(self.h, address, n)
        st, got, total = device_pairs(self.sg, address, n, pair_ids, pair_pos, int(want[0].size) + 3)
        assert st == 0
        ref.same(got, want, f"{what}/pairs")
        if host_form:
            ref.same(self.sg.match_host_array(data), want, f"{what}/host form")             # the GPU platform: the pipelined pairs path
        return want


# ---------------------------------------------------------------- the table of the host file


@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_in_all_three_forms(case):
    name, lines, data, cut = case
    with Opened(ref.parse_lines(lines), cut) as o:
        want = o.all_forms(data, name)
        if name in ref.WANT:
            ids, pos, end = ref.WANT[name]
            ref.same(want, (pos, ids, end), f"{name}: against the list worked out by hand")


@pytest.mark.parametrize("in_offset", [1, 2, 3])
def test_the_part_compare_with_the_pointer_off_alignment(in_offset):
    """part lengths 1 .. 20 behind a gap, a mismatch only in the last and only in the first byte of each: the parts start at every residue mod 4"""
    name, lines, data, cut = next(c for c in ref.CASES if c[0] == "tail-lengths")
    with Opened(ref.parse_lines(lines)) as o:
        want = o.all_forms(data, f"{name}/offset {in_offset}", in_offset=in_offset, host_form=False)
        assert sorted(want[1].tolist()) == list(range(1, 21))


def test_one_part_signatures_equal_the_sig_calls_on_the_device():
    """the same lines through PFACX_sigMatchFromDevice and PFACX_gapsigMatchFromDevice: the same (id, start), end = start + len"""
    lines = ["61 ?? 63", "4D 5A ?? ?? 50 45", "6? 62", "61 ?? 63"]
    data = as_array(b"abc axc MZ..PE MZ.PE ab cb aXc")
    n = int(data.size)
    d_in, address = device_input(data, in_offset=1)
    h = api.PFAC.create()
    try:
        with h.sigOpenText(ref.sig_ref.text_of(lines)) as sg:
            d_ids, d_pos = (torch.full((n,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
            st, total = sg.match_device(address, n, d_ids.data_ptr(), d_pos.data_ptr(), n)
            torch.cuda.synchronize()
            ids, pos = d_ids[:total].cpu().numpy(), d_pos[:total].cpu().numpy()
        assert st == 0 and total >= 8
        lens = [0] + [len(v) for v, _ in ref.sig_ref.parse_lines(lines)]
        with h.gapsigOpenText(ref.text_of(lines)) as gs:
            st, got, full = device_gapsig(gs, d_in, address, n, n + 3)
        assert st == 0 and full == total
        ref.same(got, (pos, ids, [int(p) + lens[int(i)] for p, i in zip(pos, ids)]), "one part against PFACX_sigMatchFromDevice")
    finally:
        h.destroy()


# ---------------------------------------------------------------- start and end bounds

BOUND_LINES = [
    "51 {0-2} 52 61 62 63",                  # 1: anchor Rabc in part 1 at 0: part 0 would lie at -1 .. -3, where the guard Q stands
    "?? {0-1} 61 62 63 {0-1} 64 ??",         # 2: starts at 0 (the choice that starts at -1 must not count); ends inside
    "77 78 79 7A {0-2} 65 66 {0-1} 67 ??",   # 3: ends exactly at n
    "77 78 79 7A {0-2} 65 66 {2-3} 67",      # 4: needs byte n (the guard g), whatever the first gap
    "77 78 79 7A {1-3} 66 {0-2} 67 68",      # 5: its widest choice needs bytes n and n + 1 (the guard gh), the narrowest fits: listed, with that end
    "77 78 79 7A {2} 66 {1-2} 68 67",        # 6: only over byte n
]


def bound_input(n_mod_4):
    fill = next(f for f in range(4) if (19 + f) % 4 == n_mod_4)
    data = b"Rabcd!" + b"." * (4 + fill) + b"wxyz.efgh"
    assert len(data) % 4 == n_mod_4
    return data


@pytest.mark.parametrize("n_mod_4", [0, 1, 2, 3])
@pytest.mark.parametrize("in_offset", [0, 1, 2, 3])
def test_start_and_end_bounds_in_a_slice_between_guards(in_offset, n_mod_4):
    """guard bytes in front (Q.: Q would be part 0 of signature 1) and behind (gh: they would complete signatures 4 and 6) must not count"""
    data = bound_input(n_mod_4)
    n = len(data)
    with Opened(ref.parse_lines(BOUND_LINES)) as o:
        want = o.all_forms(data, f"bounds/offset {in_offset}/n mod 4 = {n_mod_4}", in_offset=in_offset, front=b"Q.", behind=b"gh.j")
        got = sorted(zip(want[1].tolist(), want[0].tolist(), want[2].tolist()))
        assert got == [(2, 0, 6), (3, n - 9, n), (5, n - 9, n)], got
        # with the guards inside the buffer the others occur too: the guards are what the bounds keep out
        ids = o.model(b"Q." + data + b"gh.j", "with the guards inside")[1].tolist()
        assert sorted(set(ids)) == [1, 2, 3, 4, 5, 6]


# ---------------------------------------------------------------- block and grid edges

RUN_LINES = ["61 {0-1} 61 {1-2} 61", "61 {0-3} 62"]                # every 'a' is a pair; the second one never holds


@pytest.mark.parametrize("pairs", [BLOCK - 1, BLOCK, BLOCK + 1])
def test_pair_counts_around_one_block(pairs):
    with Opened(ref.parse_lines(RUN_LINES)) as o:
        want = o.all_forms(b"a" * pairs, f"{pairs} pairs")
        assert want[0].size == pairs - 3 and want[2].tolist() == list(range(4, pairs + 1))


def test_one_pairs_list_past_a_single_grid_pass_over_a_small_input():
    """every pair decides on its own, so a list that names each position of a 4 KiB input many times gives each entry that many times"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pairs, n = PER_CU * cus * BLOCK + 1, 4096
    data = np.full(n, 0x61, dtype=np.uint8)
    with Opened(ref.parse_lines(RUN_LINES)) as o:
        d_in, address = device_input(data)
        pair_pos = (np.arange(pairs, dtype=np.int64) * n // pairs).astype(np.int32)
        st, (pos, ids, end), total = device_pairs(o.sg, address, n, np.ones(pairs, dtype=np.int32), pair_pos, pairs)
        keep = pair_pos <= n - 4                                   # the owner is part 0 itself: the start is the pair's position
        assert st == 0 and total == int(keep.sum())
        assert np.array_equal(pos, pair_pos[keep]) and bool((ids == 1).all()) and np.array_equal(end, pair_pos[keep] + 4)


# ---------------------------------------------------------------- capacity


def test_truncation_and_a_null_end_array_in_every_form():
    name, lines, data, cut = next(c for c in ref.CASES if c[0] == "a-shared-anchor-at-different-parts")
    data = as_array(data)
    n = int(data.size)
    with Opened(ref.parse_lines(lines)) as o:
        want = o.model(data, name)
        total = int(want[0].size)
        assert total > 3
        d_in, address = device_input(data)
        pair_ids, pair_pos = longest_pairs(o.h, address, n)
        for cap in (0, total - 1, total):
            for with_end in (True, False):
                st, got, full = device_pairs(o.sg, address, n, pair_ids, pair_pos, cap, with_end)    # (the helper checks the guard words)
                assert (st, full) == (TRUNCATED if cap < total else 0, total)
                ref.same(got[:2], (want[0][:cap], want[1][:cap]), f"pairs/capacity {cap}")
                assert not with_end or got[2].tolist() == want[2][:cap].tolist()
            ids, pos, end = (np.full(GUARD + cap + GUARD, -7, dtype=np.int32) for _ in range(3))
            ptr = [a.ctypes.data + 4 * GUARD if cap else None for a in (ids, pos, end)]
            st, full = o.sg.match_host(data.ctypes.data, n, *ptr, cap, check=False)
            assert (st, full) == (TRUNCATED if cap < total else 0, total)
            ref.same(tuple(a[GUARD:GUARD + cap] for a in (pos, ids, end)), tuple(w[:cap] for w in want), f"host/capacity {cap}")
            assert all(bool((a[:GUARD] == -7).all()) and bool((a[GUARD + cap:] == -7).all()) for a in (ids, pos, end)), "wrote at or behind capacity"
        # the device form without an end array, and its refusal of capacity < size
        st, got, full = device_gapsig(o.sg, d_in, address, n, n + 3, with_end=False)
        assert st == 0 and full == total
        ref.same(got[:2], want[:2], "device/no end array")
        arrays = out_arrays(n)
        st, _ = o.sg.match_device(address, n, *[a.data_ptr() + 4 * GUARD for a in arrays], n - 1, check=False)
        assert st == INVALID
        check_guards(arrays, n, 0)


# ---------------------------------------------------------------- the pairs form: the caller's list


def test_pairs_with_ids_and_positions_that_give_nothing_and_overlapping_arrays():
    lines = ["61 62 {0-1} 64", "?? {1-2} 63 64 65"]
    data = as_array(b"abcde abd ab.d")
    n = int(data.size)
    with Opened(ref.parse_lines(lines)) as o:
        want = o.model(data, "pairs")
        d_in, address = device_input(data)
        good_ids, good_pos = longest_pairs(o.h, address, n)
        F = int(o.anchors[0].max())
        assert F == 2 and good_ids.size >= 3
        # between the good pairs: id 0, id F + 1, position -1, position size; each gives nothing
        pair_ids = np.concatenate([[0, F + 1, 1, 1], good_ids, [0, F + 1, 2]]).astype(np.int32)
        pair_pos = np.concatenate([[0, 0, -1, -1], good_pos, [n - 1, n - 1, n]]).astype(np.int32)
        st, got, total = device_pairs(o.sg, address, n, pair_ids, pair_pos, int(want[0].size) + 3)
        assert st == 0
        ref.same(got, want, "a list with pairs that give nothing")
        # output arrays that overlap the list are refused, the end array among them, and nothing is written
        t = torch.full((5 * n,), POISON, dtype=torch.int32, device="cuda:0")
        t[:good_ids.size] = torch.from_numpy(good_ids)
        t[n:n + good_pos.size] = torch.from_numpy(good_pos)
        before = t.clone()
        base, count = t.data_ptr(), int(good_ids.size)
        free = [base + 8 * n, base + 12 * n, base + 16 * n]
        for k in range(3):
            for inside in (base, base + 4 * (count - 1), base + 4 * n, base + 4 * (n + count - 1)):
                arrays = list(free)
                arrays[k] = inside
                st, _ = o.sg.pairs_device(address, n, base, base + 4 * n, count, *arrays, n, check=False)
                assert st == INVALID
        torch.cuda.synchronize()
        assert torch.equal(t, before)
        st, total = o.sg.pairs_device(address, n, base, base + 4 * n, count, *free, n, check=False)
        assert (st, total) == (0, want[0].size), "arrays that only touch are fine"
        st, total = o.sg.pairs_device(address, n, None, None, 0, None, None, None, 0, check=False)
        assert (st, total) == (0, 0), "no pairs"


def test_the_tables_are_counted_and_freed_with_the_object():
    sigs = ref.parse_lines(["61 62 {0-1} 64", "?? {1-2} 63 64 65 66"])
    h = api.PFAC.create()
    try:
        sg = h.gapsigOpen(*ref.csr_of(sigs))
        loaded = h.info().deviceTableBytes                       # the anchors' own tables
        d_in, address = device_input(as_array(b"abcd"))
        device_gapsig(sg, d_in, address, 4, 8)
        mine = 16 * 2 + 16 * 4 + 4 * (2 + 2) + 4 * 2 * 4         # 16 bytes per signature and per part, sigOff[F + 2], value and mask dwords
        assert h.info().deviceTableBytes - loaded >= mine
        h.trim()
        assert h.info().deviceTableBytes - loaded >= mine, "PFACX_trim keeps the tables of an object"
        sg.close()
        assert h.info().deviceTableBytes == loaded
    finally:
        h.destroy()


# ---------------------------------------------------------------- the seeded random case


def test_200_random_signatures_over_64_kib():
    sigs, data = ref.random_case()
    with Opened(sigs) as o:
        want, figures = ref.random_case_figures(sigs, data, o.anchors)
        print(figures)
        assert figures["entries"] >= 200 and figures["deep"] >= 20 and figures["late_owner"] >= 10 and figures["multi_start"] >= 10, figures
        o.all_forms(data, "random", want=want)
