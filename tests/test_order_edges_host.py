"""The cases of tests/test_order_edges_gpu.py (tests/order_edges.py), checked without a device: the model of PairOrder::plan against a table written
out by hand, and that every case is what it claims to be -- the kernels do not report which path a bin or a wave took, so the histograms here are the
evidence that the GPU test reaches each."""
import numpy as np
import pytest

from tests import order_edges as oe

OTHER_CUS = 304                                  # the list is built from the device's CU count: a second count, for the cases that depend on it


def test_plan_model_against_a_table_written_by_hand():
    """n -> (shift, bins, words, per).  Shift 6 up to 2^22 (2^16 bins of 64 positions), then one more per doubling; bins = ceil(n / 2^shift);
    words = 2^shift / 32; a thread of the rank pass takes words / 256 consecutive words where there are more than 256: 2 only at shift 14, 4 at 15."""
    table = {
        1: (6, 1, 2, 1), 2: (6, 1, 2, 1), 63: (6, 1, 2, 1), 64: (6, 1, 2, 1), 65: (6, 2, 2, 1),
        65536: (6, 1024, 2, 1), 65537: (6, 1025, 2, 1), 524289: (6, 8193, 2, 1),
        3178857: (6, 49670, 2, 1), 4194303: (6, 65536, 2, 1), 4194304: (6, 65536, 2, 1),
        4194305: (7, 32769, 4, 1), 6357731: (7, 49670, 4, 1), 8388608: (7, 65536, 4, 1),
        8388609: (8, 32769, 8, 1), 12715491: (8, 49670, 8, 1), 16777216: (8, 65536, 8, 1),
        16777217: (9, 32769, 16, 1), 25431011: (9, 49670, 16, 1), 33554432: (9, 65536, 16, 1),
        33554433: (10, 32769, 32, 1), 50862051: (10, 49670, 32, 1), 67108864: (10, 65536, 32, 1),
        67108865: (11, 32769, 64, 1), 101724131: (11, 49670, 64, 1), 134217728: (11, 65536, 64, 1),
        134217729: (12, 32769, 128, 1), 203448291: (12, 49670, 128, 1), 268435456: (12, 65536, 128, 1),
        268435457: (13, 32769, 256, 1), 406896611: (13, 49670, 256, 1), 536870912: (13, 65536, 256, 1),
        536870913: (14, 32769, 512, 2), 813793251: (14, 49670, 512, 2), 1073741824: (14, 65536, 512, 2),
        1073741825: (15, 32769, 1024, 4), 1627586531: (15, 49670, 1024, 4), 2147483647: (15, 65536, 1024, 4),
    }
    listed = sorted({n for s in oe.SHIFTS for n in oe.sizes(s)})
    assert listed == sorted(table), set(listed) ^ set(table)
    for n, (shift, bins, words, per) in table.items():
        p = oe.plan(n)
        assert (p["shift"], p["bins"], p["words"], p["per"]) == (shift, bins, words, per), (n, p)
        assert p["padded"] % 1024 == 0 and 0 <= p["padded"] - bins < 1024
    assert [s for s in oe.SHIFTS if oe.plan(oe.mid_n(s))["per"] == 2] == [14] and [s for s in oe.SHIFTS if oe.plan(oe.mid_n(s))["per"] == 4] == [15]
    assert [oe.shift_id(s) for s in (6, 13, 14, 15)] == ["shift6", "shift13", "shift14-per2", "shift15-per4"]
    for s in oe.SHIFTS:
        first, mid, last = oe.first_n(s), oe.mid_n(s), oe.last_n(s)
        assert {oe.plan(n)["shift"] for n in (first, mid, last)} == {s}
        assert s == 15 or oe.plan(last + 1)["shift"] == s + 1
        assert s == 6 or oe.plan(first - 1)["shift"] == s - 1
        assert (mid - 1) % (1 << s) != 0 and first < mid < last, "a ragged last bin"


def test_scratch_model():
    """capacity_fresh by hand for n = 100 000, 65536 pairs: 1563 bins, 2048 counters -> 8448 + 8192 + 6400 = 23040 fixed bytes; need 23040 + 2 * 262144 =
    547328, reserved 820992; each array (820992 - 23040) / 2 = 398976 bytes, down to a multiple of 256: 398848 = 99712 pairs; 256 bytes more of scratch are
    128 more per array, which reach the next multiple."""
    assert oe.fixed_bytes(100_000) == 23040 and oe.reserve_bytes(100_000, 65536) == 820992 and oe.capacity_fresh(100_000, 65536) == 99712
    assert oe.capacity_of(100_000, 820992 + 255) == 99712 and oe.capacity_of(100_000, 820992 + 256) == 99776
    n = oe.capacity_edge()
    assert oe.capacity_fresh(n, 65536) == n and oe.capacity_fresh(n + 1, 65536) < n + 1 and 65536 < n < (1 << 20)
    assert oe.reserve_bytes(n + 1, n + 1) > oe.reserve_bytes(n + 1, 65536) + (1 << 18), "the second round grows the scratch by far more than anything else on the handle takes"
    assert [oe.grid_for(256, k) for k in (0, 1, 256, 257, 2048 * 256, 1 << 30)] == [1, 1, 1, 2, 2048, 2048] and oe.grid_for(0, 1 << 30) == 2048


def test_the_front_of_block_8_is_the_first_eight_deep_one():
    assert [oe.front_is_eight_deep(b) for b in (0, 1, 7, 8, 9, 63)] == [False, False, False, True, True, True]
    assert oe.first_eight_deep_block() * oe.kOrderBlockBins == 8192
    for s in oe.SHIFTS:
        named = oe.named_bins(oe.mid_n(s))
        assert named == {"bin 0": 0, "bin 1": 1, "bin 1023": 1023, "bin 1024": 1024, "bin 1025": 1025, "bin 8191": 8191, "bin 8192": 8192, "bin 8193": 8193,
                         "last bin": 49669, "last bin of the last whole block": 49151}
        assert oe.bin_width(oe.mid_n(s), 49669) == (41 if s == 6 else (1 << s) - 29) and oe.bin_width(oe.mid_n(s), 49668) == 1 << s


@pytest.mark.parametrize("cus", [oe.NOMINAL_CUS, OTHER_CUS])
def test_number_of_cases_and_their_cost(cus):
    grid = 8 * cus
    cases = oe.cases(grid)
    by_group = {g: len(oe.group(g, grid)) for g in ("size", "bins", "crowded", "pairs", "waves", "fresh")}
    assert by_group == {"size": 58, "bins": 87, "crowded": 5, "pairs": 12, "waves": 20, "fresh": 2} and len(cases) == 184
    assert max(c.count for c in cases) == 2 * grid * 256 + 77 <= oe.MAX_PAIRS
    # the "pairs" group: 5 grid 256 and a thousand; "crowded": 65 (5 grid + 4) and the background; every other group together: 0.6 M
    assert sum(c.count for c in cases) < 5 * grid * 256 + 65 * 5 * grid + 700_000
    assert sum(c.count for c in cases if c.group not in ("pairs", "crowded")) < 600_000
    for s in oe.SHIFTS:
        assert len(oe.group("size", grid, s)) == (13 if s == 6 else 5) and len(oe.group("bins", grid, s)) == (6 if s == 6 else 9)
        assert len(oe.group("waves", grid, s)) == 2
        assert {c.order for c in oe.group("bins", grid, s)} == {"ascending", "descending", "random"}
    assert {c.shift for c in cases} == set(oe.SHIFTS)
    assert {c.order for c in cases} == set(oe.ORDERS)


def test_every_case_has_distinct_positions_below_n_and_a_permutation_of_them():
    for c in oe.cases():
        assert c.pos.dtype == np.int64 and np.all(np.diff(c.pos) > 0), c
        assert c.count == 0 or (0 <= c.pos[0] and c.pos[-1] < c.n), c
        assert 0 < c.n < 1 << 31 and c.count <= c.n
        perm = c.perm()
        assert np.array_equal(np.sort(perm), np.arange(c.count)), c
        assert np.array_equal(perm, c.perm()), "deterministic"
        if c.order == "ascending":
            assert np.all(np.diff(c.pos[perm]) > 0)
        if c.order == "descending":
            assert np.all(np.diff(c.pos[perm]) < 0)
        if c.order == "random" and c.count > 100:
            assert 0.3 < np.mean(np.diff(c.pos[perm]) > 0) < 0.7
    ids = oe.ids_of(np.array([0, 1, 128, (1 << 31) - 2]))
    assert ids.tolist() == [1 + (p * 2654435761 >> 7) % 1000003 for p in (0, 1, 128, (1 << 31) - 2)] and ids.dtype == np.int32
    many = oe.ids_of(oe.cases()[-2].pos)
    assert np.unique(many).size > 0.97 * many.size and many.min() >= 1


def test_size_cases():
    for s in oe.SHIFTS:
        got = oe.group("size", shift=s)
        spread = [c for c in got if c.count > 1 or c.n <= 2]
        assert sorted(c.n for c in spread if not c.name.endswith(("position 0", "position n - 1"))) == sorted(oe.sizes(s))
        for c in spread:
            assert c.pos[0] == 0 and c.pos[-1] == c.n - 1 and c.count == min(c.n, 2000 + 2) or c.count in range(1990, 2003), c
        only = [c for c in got if c.name.endswith(("position 0", "position n - 1"))]
        assert [(c.count, int(c.pos[0])) for c in only] == [(1, 0), (1, oe.last_n(s) - 1)]
        assert oe.plan(only[1].n)["bins"] == 65536 and int(only[1].pos[0]) >> s == 65535, "... in the last of 2^16 bins"


@pytest.mark.parametrize("shift", oe.SHIFTS, ids=oe.shift_id)
def test_bins_cases_place_every_occupancy_in_every_named_bin(shift):
    n = oe.mid_n(shift)
    w = 1 << shift
    occ = oe.occupancies(shift)
    labels = [label for label, _ in occ]
    assert labels == (["0", "1", "2", "63", "64=full", "first+last"] if shift == 6 else
                      ["0", "1", "2", "63", "64", "65", "min(2^s,4096)", "full" if shift <= 12 else "33+33+every 97th", "first+last"])
    ends97 = np.unique(np.r_[np.arange(33), np.arange(w - 33, w), np.arange(0, w, 97)])
    seen = set()
    got = oe.group("bins", shift=shift)
    assert len(got) == len(occ)
    for r, c in enumerate(got):
        assert c.n == n and c.shift == shift
        hist = c.histogram()
        layout = oe.bins_layout(shift, r)
        assert {b for b, _, _ in layout.values()} == set(oe.named_bins(n).values())
        for name, (b, label, what) in layout.items():
            width = oe.bin_width(n, b)
            inside = c.pos[c.pos >> shift == b] - (b << shift)
            assert (width == w) == (name != "last bin")
            if what == "ends":
                assert inside.tolist() == [0, width - 1], (c, name)
            elif what == "ends97":
                assert width < w or np.array_equal(inside, ends97), (c, name)
                assert np.array_equal(inside[:33], np.arange(33)) and np.array_equal(inside[-33:], np.arange(width - 33, width)) and inside.size > 66 + width // 97 - 2
            else:
                assert hist[b] == min(int(what), width), (c, name, label)
                if int(what) == w:
                    assert np.array_equal(inside, np.arange(width)), "a full bin"
            seen.add((name, label))
        # the threshold: 64 pairs are ranked by the pair loop, 65 through the bitmap -- and the crowded bins' positions reach the bitmap's last words
        if shift > 6:
            assert 64 in hist[list(oe.named_bins(n).values())] and 65 in hist[list(oe.named_bins(n).values())]
            crowded = [b for b in oe.named_bins(n).values() if hist[b] > oe.kOrderCrowded and oe.bin_width(n, b) == w]
            assert crowded and all(((c.pos[c.pos >> shift == b] & (w - 1)) >> 5).max() >= oe.plan(n)["words"] * 3 // 4 for b in crowded)
        assert c.count - sum(hist[b] for b in oe.named_bins(n).values()) > 1400, "background pairs in front of, between and behind the named bins"
        assert hist[2:1023].sum() > 10 and hist[1026:8191].sum() > 100 and hist[8194:49151].sum() > 500
    assert seen == {(name, label) for name in oe.named_bins(n) for label in labels}


@pytest.mark.parametrize("cus", [oe.NOMINAL_CUS, OTHER_CUS])
def test_crowded_and_pairs_cases_follow_the_grid(cus):
    grid = 8 * cus
    assert oe.grid_for(cus, oe.capacity_fresh(oe.CROWDED_N, 2 * grid * 256 + 77)) == grid, "the scratch that holds the largest case gives the full grid"
    assert oe.plan(oe.CROWDED_N)["shift"] == 7
    want = [1, grid - 1, grid, grid + 1, 2 * grid + 3]
    for c, k in zip(oe.group("crowded", grid), want):
        hist = c.histogram()
        assert int(np.sum(hist > oe.kOrderCrowded)) == k and set(hist[hist > oe.kOrderCrowded].tolist()) == {65}, c
        assert hist.max() == 65 and c.count - 65 * k > 1000
    assert [c.count for c in oe.group("pairs", grid)] == [0, 1, 63, 64, 65, 255, 256, 257, grid * 256 - 1, grid * 256, grid * 256 + 1, 2 * grid * 256 + 77]
    for c in oe.group("pairs", grid):
        assert c.n == oe.CROWDED_N and (c.count < 2 or np.diff(c.pos).max() - np.diff(c.pos).min() <= 1), "spread evenly"
    # on a handle of its own the grid follows the scratch of that one call: fewer blocks than crowded bins, whatever the device
    crowded, plain = oe.group("fresh", grid)
    assert int(np.sum(crowded.histogram() > oe.kOrderCrowded)) == oe.FRESH_CROWDED_BINS
    for some_cus in (64, 256, 304):
        assert oe.grid_for(some_cus, oe.capacity_fresh(crowded.n, crowded.count)) < oe.FRESH_CROWDED_BINS


@pytest.mark.parametrize("shift", oe.SHIFTS, ids=oe.shift_id)
def test_waves_cases_have_the_property_stated(shift):
    striped, clumped = oe.group("waves", shift=shift)
    assert (striped.order, clumped.order) == ("striped", "clumped") and striped.count == 384 and clumped.count == 40 * (64 if shift == 6 else 128)
    for c, distinct in ((striped, 64), (clumped, 1)):
        bins = (c.pos[c.perm()] >> shift).reshape(-1, 64)          # the waves of the count and the scatter pass: aligned runs of 64 list entries
        assert all(np.unique(row).size == distinct for row in bins), c
    by_bin = (clumped.pos[clumped.perm()] >> shift).reshape(-1, 64)[:, 0]
    assert np.mean(np.diff(by_bin) > 0) < 0.8, "the clumps are shuffled"
    inside = clumped.pos[clumped.perm()].reshape(-1, 64)
    assert np.mean(np.diff(inside, axis=1) > 0) < 0.7, "... and so is each clump"


@pytest.mark.parametrize("n", oe.REAL_SIZES + (oe.REAL_BIG,))
def test_inputs_of_the_real_scans_hold_their_plants(n):
    """The oracle is run on these inputs by the GPU test, which checks the histogram of its result; here: the bytes."""
    p = oe.plan(n)
    s = p["shift"]
    assert s == {(1 << 22) - 1: 6, 1 << 22: 6, (1 << 22) + 1: 7, (1 << 23) + 1: 8, (1 << 24) + 1: 9}[n]
    data = oe.real_input(n)
    assert data.size == n and data.dtype == np.uint8
    starts = {p[0] for p in oe.PATTERNS}
    assert not any(b in starts for b in oe.FILLER)
    h = np.flatnonzero(data == ord("h"))
    hist = np.bincount(h >> s, minlength=p["bins"])
    plants = oe.real_plants(n)
    for what in ("64", "65", "full"):
        b, k = plants[what]
        assert hist[b] == k, (what, hist[b])
    assert plants["64"][1] + 1 == plants["65"][1] and plants["65"][0] == plants["64"][0] + 1 and plants["full"][1] == 1 << s
    assert (plants["64"][1], plants["65"][1]) == ((63, 64) if s == 6 else (64, 65))
    assert bytes(data[:3]) == b"abc" and data[n - 1] == ord("h") and bytes(data[(1024 << s) - 1:(1024 << s) + 5]) == b"abmnop"
