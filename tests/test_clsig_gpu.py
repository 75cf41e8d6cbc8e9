"""PFACX_clsigMatchFromDevice / PFACX_clsigPairsFromDevice / PFACX_clsigMatchFromHost (GPU platform) against the models of tests/clsig_ref.py:
the table of the host file, the buffer a slice of a larger tensor at every pointer offset mod 4 and every n mod 4 between guard bytes that would
complete an embedding or forbid one, pair counts around the frame's block, one pairs list past a single grid pass over a small input, one class
more than the kernel stages in LDS, a fixed run of 65 535 bytes, class windows that cross the mask's top bit on both sides of the anchor, the
same set through PFACX_gapsig* and PFACX_sig*, truncation with and without the end array, pair lists with ids and positions that must be ignored,
overlapping arrays, the tables' bytes, and a seeded random set of 200 signatures over 64 KiB.  All arrays are poisoned and carry guard words on
both sides; the input must stay untouched."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import clsig_ref as ref  # noqa: E402
from tests.clsig_ref import test_the_models_agree_on_every_case  # noqa: E402,F401  (runs here too: clsig_ref.py is not collected)

BLOCK = api.PFACX_CLSIG_BLOCK                   # scan_clsig.hip: kClSigBlock
PER_CU = api.PFACX_CLSIG_BLOCKS_PER_CU          # scan_passes.h: offsetBlocks takes eight blocks per compute unit at most
STAGED = api.PFACX_CLSIG_STAGED_CLASSES         # scan_clsig.hip: kClSigStaged
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


def device_clsig(sg, d_in, address, n, capacity, with_end=True):
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
    """a GPU handle with a class-signature object over `sigs` (or the text `lines`) and what the getter says"""

    def __init__(self, sigs, max_len=0, flags=0, lines=None):
        self.sigs, self.flags, self.lines = sigs, flags, lines
        self.h = api.PFAC.create()
        self.sg = self.h.clsigOpenText(ref.text_of(lines), max_len, flags) if lines is not None else self.h.clsigOpen(*ref.csr_of(sigs), max_len, flags)
        self.anchors = self.sg.anchors()
        want, _ = ref.model_anchors(sigs, max_len)
        assert all(g.tolist() == w.tolist() for g, w in zip(self.anchors, want))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.sg.close(check=False)
        self.h.destroy()

    def model(self, data, what):
        return ref.check_models(self.sigs, data, self.anchors, what, self.flags, self.lines)

    def all_forms(self, data, what, in_offset=0, front=b"", behind=b"", host_form=True, want=None):
        """the device form, the pairs form over the handle's own reduce list and the host form against the model -> the model's list"""
        data = as_array(data)
        n = int(data.size)
        want = self.model(data, what) if want is None else want
        d_in, address = device_input(data, in_offset, front, behind)
        st, got, total = device_clsig(self.sg, d_in, address, n, max(n, int(want[0].size)) + 3)
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
    name, lines, data, cut, flags = case
    with Opened(ref.parse_lines(lines), cut, flags, lines) as o:
        want = o.all_forms(data, name)
        if name in ref.WANT:
            ids, pos, end = ref.WANT[name]
            ref.same(want, (pos, ids, end), f"{name}: against the list worked out by hand")


# ---------------------------------------------------------------- start and end bounds, every alignment

BOUND_LINES = [
    "[Q]?Rabc",                              # 1: anchor Rabc at 0: the optional Q would lie at -1, where the guard Q stands: start 0, never -1
    "(?<![Q.])Rab",                          # 2: a start at 0 is valid whatever stands in front of the buffer (the guard Q would forbid it)
    "(?<![R])abc",                           # 3: notBefore in front of a member byte: refused at 1
    "wxyz[a-z.]{2,9}",                       # 4: a class run that would run past n into the guard `gh`: cut at n
    "wxyz.efgh(?![g])",                      # 5: ends exactly at n: valid whatever stands behind the buffer (the guard g would forbid it)
    "wxyz.efgh[g]{1,2}",                     # 6: needs byte n
    "wxyz[.e]{1,3}fghg",                     # 7: its literal would leave the buffer
    "[!.]{0,5}wxyz",                         # 8: a run backwards
]


def bound_input(n_mod_4):
    fill = next(f for f in range(4) if (19 + f) % 4 == n_mod_4)
    data = b"Rabcd!" + b"." * (4 + fill) + b"wxyz.efgh"
    assert len(data) % 4 == n_mod_4
    return data


@pytest.mark.parametrize("n_mod_4", [0, 1, 2, 3])
@pytest.mark.parametrize("in_offset", [0, 1, 2, 3])
def test_start_and_end_bounds_in_a_slice_between_guards(in_offset, n_mod_4):
    data = bound_input(n_mod_4)
    n = len(data)
    with Opened(ref.parse_lines(BOUND_LINES), lines=BOUND_LINES) as o:
        want = o.all_forms(data, f"bounds/offset {in_offset}/n mod 4 = {n_mod_4}", in_offset=in_offset, front=b".Q", behind=b"gh.j")
        got = sorted(zip(want[1].tolist(), want[0].tolist(), want[2].tolist()))
        assert [g for g in got if g[0] != 8] == [(1, 0, 4), (2, 0, 3), (4, n - 9, n), (5, n - 9, n)], got
        assert [g[1] for g in got if g[0] == 8] == list(range(n - 14, n - 8)), got
        # with the guards inside the buffer it is another list: the guards are what the bounds keep out
        ids = o.model(b".Q" + data + b"gh.j", "with the guards inside")[1].tolist()
        assert sorted(set(ids)) == [1, 4, 6, 7, 8] and ids.count(1) == 2


# ---------------------------------------------------------------- block and grid edges

RUN_LINES = ["a[a]{0,1}a[b-z]?", "a[0-9]{1,3}b"]                   # every 'a' is a pair; the second one never holds


@pytest.mark.parametrize("pairs", [BLOCK - 1, BLOCK, BLOCK + 1])
def test_pair_counts_around_one_block(pairs):
    with Opened(ref.parse_lines(RUN_LINES), lines=RUN_LINES) as o:
        want = o.all_forms(b"a" * pairs, f"{pairs} pairs")
        assert want[0].size == pairs - 1 and want[2].tolist() == list(range(3, pairs + 1)) + [pairs]


def test_one_pairs_list_past_a_single_grid_pass_over_a_small_input():
    """every pair decides on its own, so a list that names each position of a 4 KiB input many times gives each entry that many times"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pairs, n = PER_CU * cus * BLOCK + 1, 4096
    data = np.full(n, 0x61, dtype=np.uint8)
    with Opened(ref.parse_lines(RUN_LINES)) as o:
        d_in, address = device_input(data)
        pair_pos = (np.arange(pairs, dtype=np.int64) * n // pairs).astype(np.int32)
        st, (pos, ids, end), total = device_pairs(o.sg, address, n, np.ones(pairs, dtype=np.int32), pair_pos, pairs)
        keep = pair_pos <= n - 2                                   # the owner is part 0 itself: the start is the pair's position
        assert st == 0 and total == int(keep.sum())
        assert np.array_equal(pos, pair_pos[keep]) and bool((ids == 1).all()) and np.array_equal(end, np.minimum(pair_pos[keep] + 3, n))


# ---------------------------------------------------------------- the class table past what LDS stages, long runs, the mask's top bit


def test_one_class_more_than_the_kernel_stages_in_lds():
    """STAGED + 1 distinct classes: the last staged one and the first unstaged one are both used, in parts and as boundaries"""
    sets = [frozenset([0x30 + k, 0x80 + k]) for k in range(STAGED - 1)]
    k_byte = (frozenset(b"k"), 1, 1)
    sigs = [([k_byte, (frozenset(b"="), 1, 1)] + [(s, 1, 1) for s in sets[:STAGED - 2]], None, None),        # classes 0 .. STAGED - 1, 63 parts
            ([k_byte, (sets[STAGED - 3], 1, 2), (sets[STAGED - 2], 0, 2)], sets[STAGED - 3], sets[STAGED - 2])]
    table = ref.csr_of(sigs)
    assert table[0].shape[0] == STAGED + 1 and table[1][STAGED - 1] == STAGED - 1
    assert table[1][STAGED:].tolist() == [0, STAGED - 1, STAGED] and table[5].tolist() == [-1, STAGED - 1] and table[6].tolist() == [-1, STAGED]
    body = bytes(0x30 + k for k in range(STAGED - 2))
    last, first = bytes([0x30 + STAGED - 3]), bytes([0x30 + STAGED - 2])
    data = (b"k=" + body + b" k=" + body[:-1] + bytes([0x80 + STAGED - 3]) + b" k=" + body[:-1] + b"! k" + last + first + b" " + last + b"k" + last +
            b" k" + last + last + first + first + first + b" k" + last + b"~ k" + first)
    with Opened(sigs) as o:
        want = o.all_forms(data, "staged + 1 classes")
        assert want[1].tolist().count(1) == 2 and want[1].tolist().count(2) >= 2


def test_a_fixed_run_of_65535_bytes_just_long_enough_and_one_byte_too_short():
    lines = ["key[a]{65535}", "key[a]{65535}[b]?"]
    sigs = ref.parse_lines(lines)
    assert [kind for kind, _, _ in ref.fuse(sigs[0])] == ["lit"]           # a one-byte class with lo == hi is literal: one part of 65 538 bytes?
    data = np.frombuffer(b"key" + b"a" * 65535, dtype=np.uint8)
    h = api.PFAC.create()
    try:
        assert h.clsigOpenText(ref.text_of(lines), check=False).bad == 1     # ... refused: a literal part has at most 65 535 bytes
        lines = ["key[ab]{65535}", "xkey[ab]{65534}[c]?"]
        with h.clsigOpenText(ref.text_of(lines)) as sg:
            for n, want in ((65538, ([0], [1], [65538])), (65537, ([], [], []))):
                d_in, address = device_input(data[:n], in_offset=1)
                st, got, total = device_clsig(sg, d_in, address, n, n + 3)
                assert st == 0
                ref.same(got, want, f"{n} bytes")
    finally:
        h.destroy()


def test_class_windows_that_cross_the_top_bit_of_the_mask_on_both_sides_of_the_anchor():
    lines = ["[0-9]{0,63}KEY", "KEY[0-9]{0,63};", "x[0-9]{0,40}KEY[a-f]{0,23}z", "(?<![0-9])[0-9]{1,64}KEY"]
    runs = (0, 1, 62, 63, 64, 70)
    data = ref.SEP.join(b"x" + b"7" * d + b"KEY" + b"5" * d + b";" for d in runs) + ref.SEP + b"x" + b"1" * 40 + b"KEY" + b"abcdef" * 3 + b"abcdez"
    with Opened(ref.parse_lines(lines), lines=lines) as o:
        want = o.all_forms(data, "top bit", in_offset=3)
        ids = want[1].tolist()
        assert ids.count(1) > 3 * 64 and all(ids.count(i) >= 1 for i in (2, 3, 4)), "64 starts from one anchor occurrence, more than once"


def test_the_same_set_through_the_gapsig_and_sig_calls():
    """full classes (??), nibble classes (5?, ?A) and gaps: (id, start, end) equal as sets with SHORTEST_END; one part equals PFACX_sig*"""
    from tests import gapsig_ref, sig_ref
    gap_lines = ["4D 5A {2-6} 50 45 00", "E8 ?? ?? [0-8] 5? C3", "61 62 {0-3} ?A 63 64 {1-2} 65"]
    cls_lines = ["MZ.{2,6}PE\\x00", "\\xe8.{2}.{0,8}[P-_]\\xc3", "ab.{0,3}[\\x0a\\x1a*:JZjz\\x8a\\x9a\\xaa\\xba\\xca\\xda\\xea\\xfa]cd.{1,2}e"]
    data = np.random.default_rng(11).integers(0, 256, 3000, dtype=np.uint8)
    gapsig_ref.embed(gapsig_ref.parse_lines(gap_lines), data, 5, per_sig=6)
    n = int(data.size)
    d_in, address = device_input(data, in_offset=2)
    h = api.PFAC.create()
    try:
        lists = []
        for opened in (lambda: h.gapsigOpenText(gapsig_ref.text_of(gap_lines)), lambda: h.clsigOpenText(ref.text_of(cls_lines), 0, ref.SHORTEST)):
            with opened() as sg:                                     # one after the other: an open call replaces the handle's set
                arrays = out_arrays(n)
                st, total = sg.match_device(address, n, *[a.data_ptr() + 4 * GUARD for a in arrays], n)
                torch.cuda.synchronize()
                pos, ids, end = taken(arrays, total)
                lists.append(sorted(zip(ids.tolist(), pos.tolist(), end.tolist())))
        assert len(lists[0]) >= 12 and lists[0] == lists[1]
        one = ["61 62 63", "4D 5A 00 00 50 45", "61 2E 63"]
        text = as_array(b"abc abd MZ\0\0PE abc a.c")
        d_in, address = device_input(text, in_offset=1)
        with h.sigOpenText(sig_ref.text_of(one)) as sg:
            d_ids, d_pos = (torch.full((text.size,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
            st, total = sg.match_device(address, text.size, d_ids.data_ptr(), d_pos.data_ptr(), text.size)
            torch.cuda.synchronize()
            ids, pos = d_ids[:total].cpu().numpy(), d_pos[:total].cpu().numpy()
        with h.clsigOpenText(ref.text_of(["abc", "MZ\\x00\\x00PE", "a\\.c"])) as cs:
            st, got, full = device_clsig(cs, d_in, address, int(text.size), int(text.size) + 3)
        lens = [0, 3, 6, 3]
        assert full == total >= 4
        ref.same(got, (pos, ids, [int(p) + lens[int(i)] for p, i in zip(pos, ids)]), "one part against PFACX_sigMatchFromDevice")
    finally:
        h.destroy()


# ---------------------------------------------------------------- capacity


def test_truncation_and_a_null_end_array_in_every_form():
    name, lines, data, cut, flags = next(c for c in ref.CASES if c[0] == "a-shared-anchor")
    data = as_array(data)
    n = int(data.size)
    with Opened(ref.parse_lines(lines), lines=lines) as o:
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
        st, got, full = device_clsig(o.sg, d_in, address, n, n + 3, with_end=False)
        assert st == 0 and full == total
        ref.same(got[:2], want[:2], "device/no end array")
        arrays = out_arrays(n)
        st, _ = o.sg.match_device(address, n, *[a.data_ptr() + 4 * GUARD for a in arrays], n - 1, check=False)
        assert st == INVALID
        check_guards(arrays, n, 0)


# ---------------------------------------------------------------- the pairs form: the caller's list


def test_pairs_with_ids_and_positions_that_give_nothing_and_overlapping_arrays():
    lines = ["ab[0-9]?d", "[x-z]{1,2}cde"]
    data = as_array(b"abcde ab1d abd zcde")
    n = int(data.size)
    with Opened(ref.parse_lines(lines), lines=lines) as o:
        want = o.model(data, "pairs")
        d_in, address = device_input(data)
        good_ids, good_pos = longest_pairs(o.h, address, n)
        F = int(o.anchors[0].max())
        assert F == 2 and good_ids.size >= 3 and want[0].size == 3
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
    h = api.PFAC.create()
    try:
        # two signatures, five parts, a blob of two dwords, F = 2, and ONE class: four spellings of it and a boundary are stored once
        sg = h.clsigOpenText(b"ab[0-9]{1,2}\\d{0,1}\n(?<![\\d])xyzw[0123456789]\n")
        loaded = h.info().deviceTableBytes                       # the anchors' own tables
        d_in, address = device_input(as_array(b"ab12"))
        device_clsig(sg, d_in, address, 4, 8)
        mine = 32 * 2 + 16 * 5 + 4 * (2 + 2) + 4 * 2 + 32 * 1
        grown = h.info().deviceTableBytes - loaded
        assert mine <= grown < mine + 32 + 5 * 256, "one class of 32 bytes; more only by what the allocations round up"
        h.trim()
        assert h.info().deviceTableBytes - loaded == grown, "PFACX_trim keeps the tables of an object"
        sg.close()
        assert h.info().deviceTableBytes == loaded
    finally:
        h.destroy()


# ---------------------------------------------------------------- the seeded random case


def test_200_random_signatures_over_64_kib():
    sigs, data = ref.random_case()
    with Opened(sigs) as o:
        want, figures = ref.fast_list(sigs, data, o.anchors)
        print(figures)
        assert figures["entries"] >= 400 and figures["late_owner"] >= 5 and figures["multi_start"] >= 5, figures
        o.all_forms(data, "random", want=want)
