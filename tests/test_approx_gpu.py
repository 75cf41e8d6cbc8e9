"""PFACX_approxMatchFromDevice / PFACX_approxPairsFromDevice / PFACX_approxMatchFromHost (GPU platform) against the models of
tests/approx_ref.py: the table of the host file, the compare edges at lengths (k + 1) .. 64 for k = 0 .. 3 with exactly k and k + 1 substitutions
and the deciding one at byte 0, 15 / 16, 31 / 32, the last whole dword and each tail byte, at every pointer alignment; each occurrence once
whichever pieces are exact; the start and end bounds with the buffer a slice of a larger tensor at every offset and length mod 4 between guard
bytes that would bring a distance down to the budget; a class of 300; pair counts around the frame's block; one list past a single grid pass;
no distance array; truncation; pair lists with ids and positions that must be ignored; overlapping arrays; and two seeded random sets of 100
patterns over 64 KiB.  All arrays are poisoned and carry guard words on both sides."""

import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import approx_ref as ref  # noqa: E402
from tests.approx_ref import test_the_models_agree_on_every_case  # noqa: E402,F401  (runs here too: approx_ref.py is not collected)

BLOCK = api.PFACX_APPROX_BLOCK                  # scan_approx.hip: kApproxBlock
PER_CU = api.PFACX_APPROX_BLOCKS_PER_CU         # scan_passes.h: offsetBlocks takes eight blocks per compute unit at most
GUARD = 64
POISON = -5
INVALID, TRUNCATED = api.STATUS.INVALID_PARAMETER, api.STATUS.OUTPUT_TRUNCATED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

as_array = ref.as_array


def out_arrays(cap):
    return tuple(torch.full((GUARD + cap + GUARD,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(3))


def inner(t, capacity=1):
    """the address of the array between the guard words (None for the count query)"""
    return t.data_ptr() + 4 * GUARD if capacity else None


def check_guards(arrays, cap, clean_from):
    """nothing in front of the arrays, at or behind capacity, or in [clean_from, capacity)"""
    for a in arrays:
        assert bool((a[:GUARD] == POISON).all()) and bool((a[GUARD + cap:] == POISON).all()), "wrote outside the arrays"
        assert bool((a[GUARD + clean_from:GUARD + cap] == POISON).all()), "wrote behind the list"


def written(arrays, k):
    d_ids, d_pos, d_mis = arrays
    return tuple(a[GUARD:GUARD + k].cpu().numpy() for a in (d_pos, d_ids, d_mis))


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


def device_approx(ap, d_in, address, n, capacity, with_mis=True):
    """match_device -> (status, (pos, ids, mis) of the entries written, the full length).  The id and position arrays take the scan's unordered
    list below `size`; behind max(size, the list) and outside the arrays nothing may be written, the distances are only ever written below the
    list, and the input must stay untouched"""
    before = d_in.clone()
    arrays = out_arrays(capacity)
    st, total = ap.match_device(address, n, inner(arrays[0]), inner(arrays[1]), inner(arrays[2]) if with_mis else None, capacity, check=False)
    torch.cuda.synchronize()
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > capacity), (st, total, capacity)
    k = min(total, capacity)
    check_guards(arrays[:2], capacity, min(capacity, max(k, n)))
    check_guards(arrays[2:], capacity, k if with_mis else 0)
    assert torch.equal(d_in, before), "the caller's input, or what lies around it, was modified"
    return st, written(arrays, k), total


def device_pairs(ap, address, n, pair_ids, pair_pos, capacity, with_mis=True):
    """pairs_device over a pair list on the host, guard words around the pair arrays too -> (status, (pos, ids, mis), the full length)"""
    lists = []
    for a in (pair_ids, pair_pos):
        t = torch.full((GUARD + len(a) + GUARD,), POISON, dtype=torch.int32, device="cuda:0")
        t[GUARD:GUARD + len(a)] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
        lists.append(t)
    before = [t.clone() for t in lists]
    arrays = out_arrays(capacity)
    st, total = ap.pairs_device(address, n, inner(lists[0]), inner(lists[1]), len(pair_ids), inner(arrays[0], capacity), inner(arrays[1], capacity),
                                inner(arrays[2], capacity and with_mis), capacity, check=False)
    torch.cuda.synchronize()
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > capacity), (st, total, capacity)
    k = min(total, capacity)
    check_guards(arrays[:2], capacity, k)
    check_guards(arrays[2:], capacity, k if with_mis else 0)
    assert all(torch.equal(t, b) for t, b in zip(lists, before)), "the caller's pair list, or what lies around it, was modified"
    return st, written(arrays, k), total


def longest_pairs(h, address, n):
    """the ordered longest pairs of the handle's pieces: what the pairs form takes"""
    d_ids, d_pos = (torch.full((n,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
    _, count = h.matchFromDeviceReduce(address, n, d_ids.data_ptr(), d_pos.data_ptr())
    torch.cuda.synchronize()
    return d_ids[:count].cpu().numpy(), d_pos[:count].cpu().numpy()


class Opened:
    """a GPU handle with an approximate object over `patterns` / `budgets` whose getter equals the documented cut"""

    def __init__(self, patterns, budgets, min_len=0, max_len=0):
        self.patterns, self.budgets, self.max_len = patterns, budgets, max_len
        self.h = api.PFAC.create()
        self.ap = self.h.approxOpen(patterns, budgets, min_len, max_len)
        want, self.pieces = ref.model_pieces(patterns, budgets, min_len, max_len)
        assert all(g.tolist() == w.tolist() for g, w in zip(self.ap.pieces(), want)), "PFACX_approxGetPieces against model_pieces"

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ap.close(check=False)
        self.h.destroy()

    def model(self, data, what):
        return ref.check_models(self.patterns, self.budgets, data, what, self.max_len)

    def all_forms(self, data, what, want=None, in_offset=0, front=b"", behind=b"", host_form=True):
        """the device form, the pairs form over the handle's own reduce list and the host form against the models -> the models' list"""
        data = as_array(data)
        n = int(data.size)
        want = self.model(data, what) if want is None else want
        d_in, address = device_input(data, in_offset, front, behind)
        st, got, total = device_approx(self.ap, d_in, address, n, max(n, int(want[0].size)) + 3)
        assert st == 0 and total == want[0].size, (what, total, want[0].size)
        ref.same(got, want, f"{what}/device")
        pair_ids, pair_pos = longest_pairs(self.h, address, n)
        st, got, total = device_pairs(self.ap, address, n, pair_ids, pair_pos, int(want[0].size) + 3)
        assert st == 0
        ref.same(got, want, f"{what}/pairs")
        if host_form:
            ref.same(self.ap.match_host_array(data), want, f"{what}/host form")            # the GPU platform: the pipelined pairs path
        return want


# ---------------------------------------------------------------- the table of the host file: each occurrence once, shared pieces, chains


@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_in_all_three_forms(case):
    name, patterns, budgets, min_len, max_len, data = ref.case_of(case)
    with Opened(patterns, budgets, min_len, max_len) as o:
        want = o.all_forms(data, name)
        if name in ref.WANT:
            ids, pos, mis = ref.WANT[name]
            ref.same(want, (pos, ids, mis), f"{name}: against the list worked out by hand")


@pytest.mark.parametrize("exact", [(0,), (1,), (2,), (3,), (0, 1, 2, 3), (1, 3), (0, 2), (2, 3)], ids=lambda e: "pieces-" + "".join(map(str, e)))
def test_an_occurrence_is_listed_once_whichever_pieces_are_exact(exact):
    """k = 3, 32 bytes, four pieces of 8: one substitution in every part that is not named; the entry comes from the lowest exact piece"""
    data = b"...." + ref.mutate(ref.P32, [8 * j + 5 for j in range(4) if j not in exact]) + b"...."
    with Opened([ref.P32], [3]) as o:
        want = o.all_forms(data, f"exact pieces {exact}")
        assert (want[1].tolist(), want[0].tolist(), want[2].tolist()) == ([1], [4], [4 - len(exact)])
        d_in, address = device_input(data)                            # (d_in keeps the bytes alive)
        pair_ids, pair_pos = longest_pairs(o.h, address, len(data))
        assert pair_pos.tolist() == [4 + 8 * j for j in exact], "a candidate per exact piece"


# ---------------------------------------------------------------- the compare edges


@pytest.mark.parametrize("in_offset", [0, 1, 2, 3])
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_the_compare_edges_at_every_pointer_alignment(k, in_offset):
    """lengths (k + 1) .. 64 with minPieceLen 1: exactly k substitutions are accepted and k + 1 rejected, the deciding one at byte 0, 15 / 16,
    31 / 32, the last whole dword and each tail byte; occurrences start at every residue mod 4 and the last one ends the tensor, so with the
    pointer off alignment the aligned dwords in front of in[0] and behind in[n - 1] must not be loaded whole"""
    patterns, budgets, data, _ = ref.edge_case(k)
    want = ref.check_edge_case(k)
    with Opened(patterns, budgets, 1) as o:
        o.all_forms(data, f"edges k = {k}/offset {in_offset}", want=want, in_offset=in_offset, host_form=in_offset == 0)


# ---------------------------------------------------------------- start and end bounds

FRONT_GUARD, BEHIND_GUARD = b"WXYZ", b"jklm"
BOUND_HEAD, BOUND_TAIL = b"Rabcdefghijk", b"pqrStuvwxyzefgh"
BOUND_PATTERNS = (
    # 1 .. 4: 12 bytes, k = 1, the last t = 1 .. 4 guard bytes and then the head of the input: piece 1 (bytes 6 .. 11) stands at p = 6 - t, so the
    # pattern would start at -t, and with the guards read its distance would be 0
    [FRONT_GUARD[4 - t:] + BOUND_HEAD[:12 - t] for t in (1, 2, 3, 4)]
    + [b"Rabcdefg",                               # 5: k = 1: starts at 0 with d = 0: the dword in front of in[0]
       b"pqrstuvwxyzefgh"]                        # 6: k = 2, 15 bytes: ends exactly at n with d = 1, found through piece 1
    # 7 .. 10: 12 bytes, k = 1, the end of the input and then the first t = 1 .. 4 guard bytes: piece 0 stands at p = n - 12 + t, so the pattern
    # would end at n + t, and with the guards read its distance would be 0
    + [BOUND_TAIL[t - 12:] + BEHIND_GUARD[:t] for t in (1, 2, 3, 4)]
    + [b"wxyZefgh"])                              # 11: k = 1: ends exactly at n with d = 1, found through piece 1
BOUND_BUDGETS = [1, 1, 1, 1, 1, 2, 1, 1, 1, 1, 1]


def bound_input(n_mod_4):
    data = BOUND_HEAD + b"." * (4 + (n_mod_4 - 31) % 4) + BOUND_TAIL
    assert len(data) % 4 == n_mod_4
    return data


@pytest.mark.parametrize("n_mod_4", [0, 1, 2, 3])
@pytest.mark.parametrize("in_offset", [0, 1, 2, 3])
def test_start_and_end_bounds_in_a_slice_between_guards(in_offset, n_mod_4):
    """candidates that would start at -1 .. -4 and end at n + 1 .. n + 4 (every s & 3), at every pointer offset and n & 3; the guard bytes right
    in front of and right behind the buffer would bring each of their distances down to 0 if they were read"""
    data = bound_input(n_mod_4)
    n = len(data)
    with Opened(BOUND_PATTERNS, BOUND_BUDGETS) as o:
        d_in, address = device_input(data, in_offset, FRONT_GUARD, BEHIND_GUARD)
        _, pair_pos = longest_pairs(o.h, address, n)
        assert {2, 3, 4, 5} <= set(pair_pos.tolist()) and {n - 11, n - 10, n - 9, n - 8} <= set(pair_pos.tolist()), "the candidates are there"
        want = o.all_forms(data, f"bounds/offset {in_offset}/n mod 4 = {n_mod_4}", in_offset=in_offset, front=FRONT_GUARD, behind=BEHIND_GUARD)
        assert sorted(zip(want[1].tolist(), want[0].tolist(), want[2].tolist())) == [(5, 0, 0), (6, n - 15, 1), (11, n - 8, 1)]
        # with the guards inside the buffer the eight others occur: the guards are what the bounds keep out
        inside = o.model(FRONT_GUARD + data + BEHIND_GUARD, "with the guards inside")
        assert sorted(zip(inside[1].tolist(), inside[0].tolist(), inside[2].tolist())) == (
            [(t, 4 - t, 0) for t in (1, 2, 3, 4)] + [(5, 4, 0), (6, n - 11, 1)] + [(6 + t, n - 8 + t, 0) for t in (1, 2, 3, 4)] + [(11, n - 4, 1)])


def test_a_pattern_that_ends_exactly_at_n_and_one_a_byte_longer():
    with Opened([b"abcdefgh", b"abcdefghi"], [1, 1]) as o:
        for n_mod_4 in range(4):
            data = b"." * (4 + n_mod_4) + b"abcdXfgh"
            want = o.all_forms(data, f"the end at n, n mod 4 = {n_mod_4}", in_offset=1, behind=b"i...")
            assert (want[1].tolist(), want[0].tolist(), want[2].tolist()) == ([1], [4 + n_mod_4], [1])


# ---------------------------------------------------------------- classes and chains


def test_300_patterns_share_one_piece_string():
    """the piece KEY! is piece 0 of 150 patterns and piece 1 of 150 others: one class of 300 entries"""
    tails = [b"%04d" % i for i in range(150)]
    patterns = [b"KEY!" + t for t in tails] + [t + b"KEY!" for t in tails]
    budgets = [1] * 300
    data = bytearray(b"." * 600)
    for at, text in ((2, b"KEY!0007"), (101, b"0007KEY!"), (203, b"0140KEY!014x"), (330, b"xxxxKEY!xxxx"), (596, b"KEY!")):
        data[at:at + len(text)] = text
    with Opened(patterns, budgets) as o:
        (off, piece_id, _, _) = o.ap.pieces()
        assert np.count_nonzero(piece_id == 1) == 300
        want = o.all_forms(bytes(data), "a class of 300")
        got = list(zip(want[1].tolist(), want[0].tolist(), want[2].tolist()))
        # KEY!0007 at 2: pattern 8 exact, and KEY!000x, KEY!00x7 (nine each) and KEY!0107 with d = 1 through piece 0 (the tails end at 0149)
        assert (8, 2, 0) in got and (1, 2, 1) in got and (158, 101, 0) in got and (151 + 140, 203, 0) in got and (141, 207, 1) in got
        assert not any(s in (326, 330, 596) for _, s, _ in got)
        at_2 = [i for i, s, _ in got if s == 2]
        assert at_2 == sorted(at_2, reverse=True) and len(at_2) == 1 + 9 + 9 + 1, "within one piece string ids descend"


def test_the_longer_piece_comes_first_at_one_candidate_position():
    patterns, budgets = [b"abcdefgh", b"abcdWXYZ", b"abcdefXY", b"abcdefgh0123"], [1, 1, 0, 0]
    with Opened(patterns, budgets) as o:
        assert o.pieces == [b"abcd", b"efgh", b"WXYZ", b"abcdefXY", b"abcdefgh0123"]
        want = o.all_forms(b"abcdefgh0123 abcdefXY", "chain order")
        assert (want[1].tolist(), want[0].tolist(), want[2].tolist()) == ([4, 1, 3], [0, 0, 13], [0, 0, 0]), "abcdefgh0123 in front of abcd's class"


# ---------------------------------------------------------------- block and grid edges

RUN_PATTERNS, RUN_BUDGETS = [b"aaaaaaaa", b"aaaaaaab"], [1, 1]            # every 'a' is a pair; the second one holds only where d = 1 fits


@pytest.mark.parametrize("pairs", [BLOCK - 1, BLOCK, BLOCK + 1])
def test_pair_counts_around_one_block(pairs):
    with Opened(RUN_PATTERNS, RUN_BUDGETS) as o:
        data = b"a" * (pairs + 3)                                     # a pair wherever aaaa fits
        d_in, address = device_input(data)                            # (d_in keeps the bytes alive)
        pair_ids, _ = longest_pairs(o.h, address, len(data))
        assert pair_ids.size == pairs, "the passes see exactly this many pairs"
        want = o.all_forms(data, f"{pairs} pairs")
        assert want[0].size == 2 * (pairs - 4), "both patterns at every start, each once although both pieces are exact"


def test_one_pair_more_than_a_single_grid_pass():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pairs = PER_CU * cus * BLOCK + 1
    n = pairs + 3
    data = np.full(n, 0x61, dtype=np.uint8)
    with Opened(RUN_PATTERNS[:1], RUN_BUDGETS[:1]) as o:
        d_in, address = device_input(data)
        st, (pos, ids, mis), total = device_approx(o.ap, d_in, address, n, n)
        assert st == 0 and total == n - 7
        assert np.array_equal(pos, np.arange(n - 7)) and bool((ids == 1).all()) and bool((mis == 0).all())
        pair_ids, pair_pos = longest_pairs(o.h, address, n)
        assert pair_ids.size == pairs
        st, (pos, ids, mis), total = device_pairs(o.ap, address, n, pair_ids, pair_pos, n)
        assert st == 0 and total == n - 7
        assert np.array_equal(pos, np.arange(n - 7)) and bool((ids == 1).all()) and bool((mis == 0).all())


# ---------------------------------------------------------------- capacity, no distance array


def test_truncation_and_no_distance_array():
    name = "keywords-with-typos"
    _, patterns, budgets, min_len, max_len, raw = ref.case_of(next(c for c in ref.CASES if c[0] == name))
    data = as_array(raw)
    n = int(data.size)
    with Opened(patterns, budgets, min_len, max_len) as o:
        want = o.model(data, name)
        total = int(want[0].size)
        assert total > 3
        d_in, address = device_input(data)
        pair_ids, pair_pos = longest_pairs(o.h, address, n)
        for cap in (0, 1, total - 1, total):
            st, got, full = device_pairs(o.ap, address, n, pair_ids, pair_pos, cap)            # (the helper checks the guard words)
            assert (st, full) == (TRUNCATED if cap < total else 0, total)
            ref.same(got, tuple(w[:cap] for w in want), f"pairs/capacity {cap}")
            ids, pos, mis = (np.full(GUARD + cap + GUARD, -7, dtype=np.int32) for _ in range(3))
            st, full = o.ap.match_host(data.ctypes.data, n, *(a.ctypes.data + 4 * GUARD if cap else None for a in (ids, pos, mis)), cap, check=False)
            assert (st, full) == (TRUNCATED if cap < total else 0, total)
            ref.same(tuple(a[GUARD:GUARD + cap] for a in (pos, ids, mis)), tuple(w[:cap] for w in want), f"host/capacity {cap}")
            assert all(bool((a[:GUARD] == -7).all()) and bool((a[GUARD + cap:] == -7).all()) for a in (ids, pos, mis)), "wrote at or behind capacity"
        # d_mis == NULL: the two other arrays as before, the third untouched
        st, got, full = device_approx(o.ap, d_in, address, n, n + 3, with_mis=False)
        assert (st, full) == (0, total)
        ref.same(got[:2], want[:2], "device/no distances")
        st, got, full = device_pairs(o.ap, address, n, pair_ids, pair_pos, total, with_mis=False)
        assert (st, full) == (0, total)
        ref.same(got[:2], want[:2], "pairs/no distances")
        # the device form takes the scan's list first: it refuses capacity < size
        arrays = out_arrays(n)
        st, _ = o.ap.match_device(address, n, inner(arrays[0]), inner(arrays[1]), inner(arrays[2]), n - 1, check=False)
        assert st == INVALID
        check_guards(arrays, n, 0)


# ---------------------------------------------------------------- the pairs form: the caller's list


def test_pairs_with_ids_and_positions_that_give_nothing_and_overlapping_arrays():
    patterns, budgets = [b"abcdefgh", b"efghabcd"], [1, 1]
    data = as_array(b"abcdefgh abcdefgx efghabcd")
    n = int(data.size)
    with Opened(patterns, budgets) as o:
        want = o.model(data, "pairs")
        d_in, address = device_input(data)
        good_ids, good_pos = longest_pairs(o.h, address, n)
        F = len(o.pieces)
        assert F == 2 and good_ids.size >= 3
        # between the good pairs: id 0, id F + 1, a negative id, position -1, position size; each gives nothing
        pair_ids = np.concatenate([[0, F + 1, -1, 1, 1], good_ids, [0, F + 1, -(1 << 31), 2]]).astype(np.int32)
        pair_pos = np.concatenate([[0, 0, 0, -1, -1], good_pos, [n - 1, n - 1, n - 1, n]]).astype(np.int32)
        st, got, total = device_pairs(o.ap, address, n, pair_ids, pair_pos, int(want[0].size) + 3)
        assert st == 0
        ref.same(got, want, "a list with pairs that give nothing")
        # output arrays that overlap the list are refused, and nothing is written
        t = torch.full((5 * n,), POISON, dtype=torch.int32, device="cuda:0")
        t[:good_ids.size] = torch.from_numpy(good_ids)
        t[n:n + good_pos.size] = torch.from_numpy(good_pos)
        before = t.clone()
        base, count = t.data_ptr(), int(good_ids.size)
        free = [base + 8 * n, base + 12 * n, base + 16 * n]
        for slot in range(3):                                        # each of the three output arrays over each of the two pair arrays
            for over in (base, base + 4 * (count - 1), base + 4 * n, base + 4 * (n + count - 1)):
                out = list(free)
                out[slot] = over
                st, _ = o.ap.pairs_device(address, n, base, base + 4 * n, count, out[0], out[1], out[2], n, check=False)
                assert st == INVALID, (slot, over - base)
        torch.cuda.synchronize()
        assert torch.equal(t, before)
        st, total = o.ap.pairs_device(address, n, base, base + 4 * n, count, free[0], free[1], free[2], n, check=False)
        assert (st, total) == (0, want[0].size), "arrays that only touch are fine"
        st, total = o.ap.pairs_device(address, n, None, None, 0, None, None, None, 0, check=False)
        assert (st, total) == (0, 0), "no pairs"


def test_the_tables_are_counted_and_freed_with_the_object():
    h = api.PFAC.create()
    try:
        before = h.info().deviceTableBytes
        ap = h.approxOpen([b"abcdefgh", b"abcdWXYZ0"], [1, 1])
        loaded = h.info().deviceTableBytes                       # the pieces' own tables
        data = as_array(b"abcdefgh")
        d_in, address = device_input(data)
        device_approx(ap, d_in, address, 8, 11)
        mine = 16 * 4 + 4 * (3 + 2) + 4 * (2 + 3)                # 16 bytes per piece, entryOff[F + 2], the patterns' dwords
        assert h.info().deviceTableBytes - loaded >= mine
        h.trim()
        assert h.info().deviceTableBytes - loaded >= mine, "PFACX_trim keeps the tables of an object"
        ap.close()
        assert h.info().deviceTableBytes == loaded and loaded >= before
    finally:
        h.destroy()


# ---------------------------------------------------------------- the seeded random cases


@pytest.mark.parametrize("kind", ["acgt", "text"])
def test_100_random_patterns_over_64_kib(kind):
    """budgets 0 .. 4; over ACGT the 4-byte pieces make about 1 position in 256 a false candidate per piece, which is the point"""
    patterns, budgets, data = ref.random_case(kind)
    want = ref.random_want(kind)                                  # both models, as sets
    with Opened(patterns, budgets) as o:
        o.all_forms(data, f"random {kind}", want=want)
        assert 100 <= want[0].size <= 2000 and set(want[2].tolist()) >= {0, 1, 2, 3, 4}


# ---------------------------------------------------------------- the example


def test_approx_example_builds_and_runs():
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "approx_example"], check=True, stdout=subprocess.PIPE)
    p = subprocess.run([os.path.join(ROOT, "examples", "approx_example")], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    assert b"self-check passed" in p.stdout
