"""PFACX_editMatchFromDevice / PFACX_editPairsFromDevice / PFACX_editMatchFromHost (GPU platform) against the models of tests/edit_ref.py: the
case table with and without PFACX_EDIT_BEST_ENDS; the band edges for k = 0 .. 3, 5 and 7 (every budget class of scan_edit.hip) with exactly k and
k + 1 edits, all insertions in front of the exact piece, all behind it, all deletions, mixed; inputs over two letters in which best alignments
miss the candidate's piece and the neighbours of the covered range decide the flag; the early exit with the deciding edit on either side of
every fourth row; starts in front of 0 and ends behind n in a slice of a larger tensor at every pointer offset and n & 3 between guard bytes that
would bring the distance down; each occurrence once whichever pieces are exact and in periodic input; a class of 300; pair counts around one
block and one pair more than a single grid pass; capacities, NULL arrays, overlapping arrays, pairs that give nothing; the tables' memory; the
example; and two seeded random sets of 100 patterns over 32 KiB.  All arrays are poisoned and carry guard words on both sides."""

import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import edit_ref as ref  # noqa: E402

BLOCK = api.PFACX_EDIT_BLOCK                    # scan_edit.hip: kEditBlock
PER_CU = api.PFACX_EDIT_BLOCKS_PER_CU           # scan_passes.h: offsetBlocks takes eight blocks per compute unit at most
BEST = api.PFACX_EDIT_BEST_ENDS
GUARD = 64
POISON = -5
INVALID, TRUNCATED = api.STATUS.INVALID_PARAMETER, api.STATUS.OUTPUT_TRUNCATED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

as_array = ref.as_array


def out_arrays(cap):
    return tuple(torch.full((GUARD + cap + GUARD,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(4))


def inner(t, wanted=1):
    """the address of the array between the guard words (None for an array that is not given)"""
    return t.data_ptr() + 4 * GUARD if wanted else None


def check_guards(arrays, cap, clean_from):
    """nothing in front of the arrays, at or behind capacity, or in [clean_from, capacity)"""
    for a in arrays:
        assert bool((a[:GUARD] == POISON).all()) and bool((a[GUARD + cap:] == POISON).all()), "wrote outside the arrays"
        assert bool((a[GUARD + clean_from:GUARD + cap] == POISON).all()), "wrote behind the list"


def written(arrays, k):
    return tuple(a[GUARD:GUARD + k].cpu().numpy() for a in arrays)          # (ids, start, end, dist)


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


def device_edit(ed, d_in, address, n, capacity, with_end=True, with_dist=True):
    """match_device -> (status, (ids, start, end, dist) of the entries written, the full length).  The id and start arrays take the scan's
    unordered list below `size`; end and dist are only ever written below the list; the input must stay untouched"""
    before = d_in.clone()
    arrays = out_arrays(capacity)
    st, total = ed.match_device(address, n, inner(arrays[0]), inner(arrays[1]), inner(arrays[2], with_end), inner(arrays[3], with_dist), capacity,
                                check=False)
    torch.cuda.synchronize()
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > capacity), (st, total, capacity)
    k = min(total, capacity)
    check_guards(arrays[:2], capacity, min(capacity, max(k, n)))
    check_guards(arrays[2:3], capacity, k if with_end else 0)
    check_guards(arrays[3:], capacity, k if with_dist else 0)
    assert torch.equal(d_in, before), "the caller's input, or what lies around it, was modified"
    return st, written(arrays, k), total


def device_pairs(ed, address, n, pair_ids, pair_pos, capacity, with_end=True, with_dist=True):
    """pairs_device over a pair list on the host, guard words around the pair arrays too -> (status, (ids, start, end, dist), the full length)"""
    lists = []
    for a in (pair_ids, pair_pos):
        t = torch.full((GUARD + len(a) + GUARD,), POISON, dtype=torch.int32, device="cuda:0")
        t[GUARD:GUARD + len(a)] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
        lists.append(t)
    before = [t.clone() for t in lists]
    arrays = out_arrays(capacity)
    st, total = ed.pairs_device(address, n, inner(lists[0]), inner(lists[1]), len(pair_ids), inner(arrays[0], capacity), inner(arrays[1], capacity),
                                inner(arrays[2], capacity and with_end), inner(arrays[3], capacity and with_dist), capacity, check=False)
    torch.cuda.synchronize()
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > capacity), (st, total, capacity)
    k = min(total, capacity)
    check_guards(arrays[:2], capacity, k)
    check_guards(arrays[2:3], capacity, k if with_end else 0)
    check_guards(arrays[3:], capacity, k if with_dist else 0)
    assert all(torch.equal(t, b) for t, b in zip(lists, before)), "the caller's pair list, or what lies around it, was modified"
    return st, written(arrays, k), total


def longest_pairs(h, address, n):
    """the ordered longest pairs of the handle's pieces: what the pairs form takes"""
    d_ids, d_pos = (torch.full((n,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(2))
    _, count = h.matchFromDeviceReduce(address, n, d_ids.data_ptr(), d_pos.data_ptr())
    torch.cuda.synchronize()
    return d_ids[:count].cpu().numpy(), d_pos[:count].cpu().numpy()


class Opened:
    """a GPU handle with an edit object over `patterns` / `budgets` whose getter equals the documented cut"""

    def __init__(self, patterns, budgets, min_len=0, max_len=0, flags=0):
        self.patterns, self.budgets, self.max_len, self.flags = patterns, budgets, max_len, flags
        self.h = api.PFAC.create()
        self.ed = self.h.editOpen(patterns, budgets, min_len, max_len, flags)
        want, self.pieces = ref.model_pieces(patterns, budgets, min_len, max_len)
        assert all(g.tolist() == w.tolist() for g, w in zip(self.ed.pieces(), want)), "PFACX_editGetPieces against model_pieces"

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ed.close(check=False)
        self.h.destroy()

    def model(self, data, what):
        return ref.check_models(self.patterns, self.budgets, data, what, self.flags, self.max_len)

    def all_forms(self, data, what, want=None, in_offset=0, front=b"", behind=b"", host_form=True):
        """the device form, the pairs form over the handle's own reduce list and the host form against the models -> the models' list"""
        data = as_array(data)
        n = int(data.size)
        want = self.model(data, what) if want is None else want
        d_in, address = device_input(data, in_offset, front, behind)
        st, got, total = device_edit(self.ed, d_in, address, n, max(n, int(want[0].size)) + 3)
        assert st == 0 and total == want[0].size, (what, total, want[0].size)
        ref.same(got, want, f"{what}/device")
        pair_ids, pair_pos = longest_pairs(self.h, address, n)
        st, got, total = device_pairs(self.ed, address, n, pair_ids, pair_pos, int(want[0].size) + 3)
        assert st == 0
        ref.same(got, want, f"{what}/pairs")
        if host_form:
            ref.same(self.ed.match_host_array(data), want, f"{what}/host form")            # the GPU platform: the pipelined pairs path
        return want


# ---------------------------------------------------------------- the case table


@pytest.mark.parametrize("flags", [0, BEST], ids=["all-ends", "best-ends"])
@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_in_all_three_forms(case, flags):
    name, patterns, budgets, min_len, max_len, data = ref.case_of(case)
    with Opened(patterns, budgets, min_len, max_len, flags) as o:
        want = o.all_forms(data, name)
        if name in ref.WANT:
            ref.same(want, ref.want_of(name, flags), f"{name}: against the list worked out by hand")


# ---------------------------------------------------------------- the band edges


@pytest.mark.parametrize("flags", [0, BEST], ids=["all-ends", "best-ends"])
@pytest.mark.parametrize("k,length", ref.BAND, ids=[f"k{k}-L{n}" for k, n in ref.BAND])
def test_band_edges_with_k_and_k_plus_1_edits(k, length, flags):
    pattern = ref.edge_pattern(length)
    data = ref.band_input(pattern, k)
    with Opened([pattern], [k], 1, 0, flags) as o:
        want = o.all_forms(data, f"band k={k} L={length}")
        assert (want[3] == k).sum() >= (4 if k and length > 2 * k else 1), "the variants with exactly k edits are occurrences"


@pytest.mark.parametrize("flags", [0, BEST], ids=["all-ends", "best-ends"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_two_letter_inputs_where_best_alignments_miss_the_piece(seed, flags):
    """over {a, b} every piece is exact all over the place: most candidates' best alignments at a covered end do not pass through the candidate's
    piece, and D(e - 1) / D(e + 1) next to the covered range decide the flag; the distances must be the true ones"""
    rng = np.random.default_rng(seed)
    patterns = [bytes(rng.choice(np.frombuffer(b"ab", dtype=np.uint8), int(rng.integers(8, 17)))) for _ in range(6)]
    budgets = [1, 2, 3, 1, 2, 3]
    budgets = [min(k, len(p) // 2 - 1) for p, k in zip(patterns, budgets)]
    data = rng.choice(np.frombuffer(b"ab", dtype=np.uint8), 203)
    with Opened(patterns, budgets, 2, 0, flags) as o:
        want = o.all_forms(data, f"two letters {seed}")
        assert want[0].size > 20


# ---------------------------------------------------------------- the early exit (tested where r & 3 == 0)


@pytest.mark.parametrize("row", [4, 8, 12])
def test_the_deciding_edit_on_either_side_of_a_row_at_which_the_exit_is_tested(row):
    """24 bytes, k = 1, the second half exact: one substitution at pattern byte x is an occurrence, with another at byte 0 it is none; x is the
    byte of row - 1, row and row + 1"""
    pattern = ref.edge_pattern(24)
    rows = [row - 1, row, row + 1]
    texts = [ref.apply_edits(pattern, [("s", r - 1)]) for r in rows] + [ref.apply_edits(pattern, [("s", 0), ("s", r - 1)]) for r in rows if r > 1]
    data = b"....." + b"....".join(texts) + b"....."
    with Opened([pattern], [1]) as o:
        want = o.all_forms(data, f"early exit at row {row}")
        assert want[0].size == 3 and want[3].tolist() == [1, 1, 1]


# ---------------------------------------------------------------- bounds


@pytest.mark.parametrize("in_offset", [0, 1, 2, 3])
def test_starts_in_front_of_0_and_ends_behind_n_between_guard_bytes(in_offset):
    """12 bytes, k = 2: the input begins with the pattern less its first c bytes and ends with it less its last c, c = 1 .. 4; the missing bytes
    lie right outside the buffer and would bring the distance down to 0 if they were read; every n & 3"""
    pattern = ref.edge_pattern(12)
    for c in (1, 2, 3, 4):
        for pad in range(4):
            data = pattern[c:] + b"." * (8 + pad) + pattern[:12 - c]
            with Opened([pattern], [2]) as o:
                want = o.all_forms(data, f"bounds c={c} pad={pad}", in_offset=in_offset, front=pattern[:c], behind=pattern[12 - c:],
                                   host_form=pad == 0)
                rows = set(zip(*[w.tolist() for w in want]))
                assert ((1, 0, 12 - c, c) in rows) == (c <= 2), "an occurrence that starts at 0"
                assert ((1, len(data) - (12 - c), len(data), c) in rows) == (c <= 2), "an occurrence that ends exactly at n"


# ---------------------------------------------------------------- ownership


P32 = ref.edge_pattern(32)


@pytest.mark.parametrize("exact", [(0,), (1,), (2,), (3,), (0, 1, 2, 3), (1, 3), (0, 2), (2, 3)], ids=lambda e: "pieces-" + "".join(map(str, e)))
def test_an_occurrence_is_listed_once_whichever_pieces_are_exact(exact):
    """k = 3, 32 bytes, four pieces of 8: one substitution in every part that is not named"""
    data = b"...." + ref.apply_edits(P32, [("s", 8 * j + 5) for j in range(4) if j not in exact]) + b"...."
    with Opened([P32], [3]) as o:
        want = o.all_forms(data, f"exact pieces {exact}")
        rows = list(zip(*[w.tolist() for w in want]))
        assert (1, 4, 36, 4 - len(exact)) in rows
        assert len({(r[0], r[2]) for r in rows}) == len(rows), "an (id, end) is listed once"


def test_a_periodic_input_in_which_one_piece_covers_an_end_from_two_positions():
    data = b".." + b"abc" * 7 + b".."
    with Opened([b"abcabcabcabc"], [2]) as o:
        want = o.all_forms(data, "periodic")
        rows = list(zip(*[w.tolist() for w in want]))
        assert len({(r[0], r[2]) for r in rows}) == len(rows) and len(rows) > 5


# ---------------------------------------------------------------- classes and chains


def test_300_patterns_share_one_piece_string():
    patterns = [b"qrstuvwx" + bytes([0x41 + i % 26, 0x41 + i // 26, 0x61 + i % 7, 0x30 + i % 10]) * 2 for i in range(300)]
    data = b"..".join(patterns[i] for i in (0, 7, 299, 150)) + b"..qrstuvwxAA.0AAa0.."
    with Opened(patterns, [1] * 300) as o:
        want = o.all_forms(data, "a class of 300")
        assert want[0].size >= 5


def test_the_longer_piece_comes_first_at_one_candidate_position():
    with Opened([b"abcd", b"abcdefgh", b"abcdef"], [0, 0, 0]) as o:
        want = o.all_forms(b"..abcdefgh..", "chain")
        assert want[0].tolist() == [2, 3, 1]


# ---------------------------------------------------------------- block and grid edges

RUN = [b"aaaaaaaa"]


def run_want(n):
    start = np.arange(n - 7, dtype=np.int32)
    return (np.ones(n - 7, dtype=np.int32), start, start + 8, np.zeros(n - 7, dtype=np.int32))


@pytest.mark.parametrize("pairs", [BLOCK - 1, BLOCK, BLOCK + 1])
def test_pair_counts_around_one_block(pairs):
    n = pairs + 7
    with Opened(RUN, [0]) as o:
        o.all_forms(np.full(n, 0x61, dtype=np.uint8), f"{pairs} pairs", want=run_want(n))


def test_one_pair_more_than_a_single_grid_pass():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pairs = PER_CU * cus * BLOCK + 1
    n = pairs + 7
    data = np.full(n, 0x61, dtype=np.uint8)
    want = run_want(n)
    with Opened(RUN, [0]) as o:
        d_in, address = device_input(data)
        st, got, total = device_edit(o.ed, d_in, address, n, n)
        assert st == 0 and total == n - 7
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        pair_ids, pair_pos = longest_pairs(o.h, address, n)
        assert pair_ids.size == pairs
        st, got, total = device_pairs(o.ed, address, n, pair_ids, pair_pos, n)
        assert st == 0 and total == n - 7
        assert all(np.array_equal(g, w) for g, w in zip(got, want))


# ---------------------------------------------------------------- arrays and capacity


def test_capacities_and_null_arrays():
    name = "exact-copy-k2"
    _, patterns, budgets, min_len, max_len, raw = ref.case_of(next(c for c in ref.CASES if c[0] == name))
    data = as_array(raw)
    n = int(data.size)
    with Opened(patterns, budgets, min_len, max_len) as o:
        want = o.model(data, name)
        total = int(want[0].size)
        assert total == 5
        d_in, address = device_input(data)
        pair_ids, pair_pos = longest_pairs(o.h, address, n)
        for cap in (0, 1, total - 1, total):
            st, got, full = device_pairs(o.ed, address, n, pair_ids, pair_pos, cap)              # (the helper checks the guard words)
            assert (st, full) == (TRUNCATED if cap < total else 0, total)
            ref.same(got, tuple(w[:cap] for w in want), f"pairs/capacity {cap}")
            arrays = [np.full(GUARD + cap + GUARD, -7, dtype=np.int32) for _ in range(4)]
            st, full = o.ed.match_host(data.ctypes.data, n, *(a.ctypes.data + 4 * GUARD if cap else None for a in arrays), cap, check=False)
            assert (st, full) == (TRUNCATED if cap < total else 0, total)
            ref.same(tuple(a[GUARD:GUARD + cap] for a in arrays), tuple(w[:cap] for w in want), f"host/capacity {cap}")
            assert all(bool((a[:GUARD] == -7).all()) and bool((a[GUARD + cap:] == -7).all()) for a in arrays), "wrote at or behind capacity"
        for with_end, with_dist in ((False, True), (True, False), (False, False)):
            st, got, full = device_edit(o.ed, d_in, address, n, n + 3, with_end, with_dist)      # (the helper: a NULL array's stand-in is untouched)
            assert (st, full) == (0, total)
            ref.same(got[:2], want[:2], "device/NULL arrays")
            st, got, full = device_pairs(o.ed, address, n, pair_ids, pair_pos, total, with_end, with_dist)
            assert (st, full) == (0, total)
            ref.same(got[:2], want[:2], "pairs/NULL arrays")
            if with_end:
                assert got[2].tolist() == want[2].tolist()
            if with_dist:
                assert got[3].tolist() == want[3].tolist()
        arrays = out_arrays(n)                                        # the device form takes the scan's list first: it refuses capacity < size
        st, _ = o.ed.match_device(address, n, inner(arrays[0]), inner(arrays[1]), inner(arrays[2]), inner(arrays[3]), n - 1, check=False)
        assert st == INVALID
        check_guards(arrays, n, 0)


def test_pairs_that_give_nothing_and_overlapping_arrays():
    patterns, budgets = [b"abcdefgh", b"efghabcd"], [1, 1]
    data = as_array(b"abcdefgh abcdefgx efghabcd")
    n = int(data.size)
    with Opened(patterns, budgets) as o:
        want = o.model(data, "pairs")
        d_in, address = device_input(data)
        good_ids, good_pos = longest_pairs(o.h, address, n)
        F = len(o.pieces)
        assert F == 2 and good_ids.size >= 3
        pair_ids = np.concatenate([[0, F + 1, -1, 1, 1], good_ids, [0, F + 1, -(1 << 31), 2, 1]]).astype(np.int32)
        pair_pos = np.concatenate([[0, 0, 0, -1, -(1 << 31)], good_pos, [n - 1, n - 1, n - 1, n, (1 << 31) - 1]]).astype(np.int32)
        st, got, total = device_pairs(o.ed, address, n, pair_ids, pair_pos, int(want[0].size) + 3)
        assert st == 0
        ref.same(got, want, "a list with pairs that give nothing")
        t = torch.full((6 * n,), POISON, dtype=torch.int32, device="cuda:0")
        t[:good_ids.size] = torch.from_numpy(good_ids)
        t[n:n + good_pos.size] = torch.from_numpy(good_pos)
        before = t.clone()
        base, count = t.data_ptr(), int(good_ids.size)
        free = [base + 8 * n, base + 12 * n, base + 16 * n, base + 20 * n]
        for slot in range(4):                                        # each of the four output arrays over each of the two pair arrays
            for over in (base, base + 4 * (count - 1), base + 4 * n, base + 4 * (n + count - 1)):
                out = list(free)
                out[slot] = over
                st, _ = o.ed.pairs_device(address, n, base, base + 4 * n, count, out[0], out[1], out[2], out[3], n, check=False)
                assert st == INVALID, (slot, over - base)
        torch.cuda.synchronize()
        assert torch.equal(t, before)
        st, total = o.ed.pairs_device(address, n, base, base + 4 * n, count, free[0], free[1], free[2], free[3], n, check=False)
        assert (st, total) == (0, want[0].size), "arrays that only touch are fine"
        st, total = o.ed.pairs_device(address, n, None, None, 0, None, None, None, None, 0, check=False)
        assert (st, total) == (0, 0), "no pairs"


def test_the_tables_are_counted_and_freed_with_the_object():
    h = api.PFAC.create()
    try:
        before = h.info().deviceTableBytes
        ed = h.editOpen([b"abcdefgh", b"abcdWXYZ0"], [1, 1])
        loaded = h.info().deviceTableBytes                       # the pieces' own tables
        data = as_array(b"abcdefgh")
        d_in, address = device_input(data)
        device_edit(ed, d_in, address, 8, 11)
        mine = 16 * 4 + 4 * (3 + 2) + 4 * (2 + 3)                # 16 bytes per piece, entryOff[F + 2], the patterns' dwords
        assert h.info().deviceTableBytes - loaded >= mine
        h.trim()
        assert h.info().deviceTableBytes - loaded >= mine, "PFACX_trim keeps the tables of an object"
        ed.close()
        assert h.info().deviceTableBytes == loaded and loaded >= before
    finally:
        h.destroy()


# ---------------------------------------------------------------- the seeded random cases


@pytest.mark.parametrize("kind", ["acgt", "text"])
def test_100_random_patterns_over_32_kib(kind):
    patterns, budgets, min_len, data, want = ref.random_case(kind)       # both models, as sets; the list has 100 .. 20 000 entries, d = 0 .. 3
    with Opened(patterns, budgets, min_len) as o:
        o.all_forms(data, f"random {kind}", want=want)


# ---------------------------------------------------------------- the example


def test_edit_example_builds_and_runs():
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "edit_example"], check=True, stdout=subprocess.PIPE)
    p = subprocess.run([os.path.join(ROOT, "examples", "edit_example")], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    assert b"self-check passed" in p.stdout
