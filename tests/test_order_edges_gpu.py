"""The four ordering launches behind every compacted-output call (pfac_amd/csrc/scan_order.inc: pfac_order_count, _offsets, _scatter, _rank, driven by
PairOrder) at every bin width and bin edge.  The launches need the pairs and the claimed input size only, so most of this file hands lists of a few
thousand pairs to PFACX_orderPairsProbe (include/pfac_module.h), which runs them as a call over n bytes would: shifts 6 to 15, the bitmap of a crowded
bin with one, two and four words per thread, bins of 64 and of 65 pairs, full bins, pairs on a bin's first and last position, the bins on either side
of a block of 1024 counters and of the first block whose front sum takes the loop with eight loads in flight, more crowded bins than the rank launch
has blocks, more pairs than one pass of the grid takes, waves whose 64 pairs share a bin or lie in 64 bins (tests/order_edges.py;
tests/test_order_edges_host.py proves that the cases are what they claim).

Expected values of the probe tests are numpy's: the sorted positions, each with the id mixed from it, 64 poisoned ints untouched on either side of both
arrays.  The tests of real calls (counter hygiene, the capacity edge, the scans at the smallest sizes of shifts 6 to 9) expect the oracle's result on
the same bytes.  One handle serves the file, so that calls of every layout follow each other on the same scratch; its scratch is first grown to hold
the largest case, which makes the grid of every later call the full one (8 blocks per compute unit) -- the case list is built from that number."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from pfac_amd import workloads as wl  # noqa: E402
from tests import order_edges as oe  # noqa: E402
from tests.gpu_helpers import assert_pairs, device_reduce, make_handle  # noqa: E402

SHIFT_PARAMS = [pytest.param(s, id=oe.shift_id(s)) for s in oe.SHIFTS]


@functools.lru_cache(maxsize=None)
def pattern_file(workdir, name="order_edges", patterns=tuple(oe.PATTERNS)):
    return wl.write_pattern_file(os.path.join(workdir, name + ".pat"), list(patterns))


def new_handle(workdir, variant=api.PFACX_KERNEL_AUTO):
    return make_handle(pattern_file(workdir), api.PFAC_SPACE_DRIVEN, api.PFAC_AUTOMATIC, variant)


def run_probe(h, c, verify=True):
    """case c through PFACX_orderPairsProbe: positions and ids against numpy, the poison around both arrays intact"""
    P = oe.POISON
    perm = c.perm()
    want_ids = oe.ids_of(c.pos)
    host_pos = np.full(c.count + 2 * P, -5, dtype=np.int32)
    host_ids = np.full(c.count + 2 * P, -5, dtype=np.int32)
    host_pos[P:P + c.count] = c.pos[perm]
    host_ids[P:P + c.count] = want_ids[perm]
    d_pos = torch.from_numpy(host_pos).to("cuda:0")
    d_ids = torch.from_numpy(host_ids).to("cuda:0")
    api.order_pairs_probe(h, d_ids.data_ptr() + 4 * P, d_pos.data_ptr() + 4 * P, c.count, c.n)
    torch.cuda.synchronize()
    if not verify:
        return
    got_pos, got_ids = d_pos.cpu().numpy(), d_ids.cpu().numpy()
    for a in (got_pos, got_ids):
        assert np.all(a[:P] == -5) and np.all(a[P + c.count:] == -5), f"{c}: wrote outside the {c.count} pairs"
    got_pos, got_ids = got_pos[P:P + c.count], got_ids[P:P + c.count]
    if not np.array_equal(got_pos, c.pos):
        bad = np.flatnonzero(got_pos != c.pos)
        k = int(bad[0])
        raise AssertionError(f"{c} (n {c.n}, shift {c.shift}, {c.count} pairs): {bad.size} positions out of place; first at {k} (bin {int(c.pos[k]) >> c.shift}): "
                             f"got {int(got_pos[k])} want {int(c.pos[k])}")
    if not np.array_equal(got_ids, want_ids):
        bad = np.flatnonzero(got_ids != want_ids)
        raise AssertionError(f"{c}: {bad.size} ids not those of their positions; first at {int(bad[0])}")


@pytest.fixture(scope="module")
def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def shared(workdir, cus):
    """the file's handle, its scratch grown by the largest case: from here on capacity >= 8 * CUs * 256 at every n, the grid is 8 * CUs"""
    h = new_handle(workdir)
    grid = 8 * cus
    assert int(h.info().multiProcessorCount) == cus
    largest = oe.group("pairs", grid)[-1]
    assert largest.count == 2 * grid * 256 + 77
    run_probe(h, largest, verify=False)            # (test_more_pairs_than_one_grid_pass checks this case like every other)
    scratch = oe.reserve_bytes(largest.n, largest.count)
    assert h.info().deviceScratchBytes >= scratch
    assert all(oe.grid_for(cus, oe.capacity_of(c.n, scratch)) == grid for c in oe.cases(grid))
    yield h
    h.destroy()


# ---------------------------------------------------------------------------------------------------------------------- the probe

@pytest.mark.parametrize("shift", SHIFT_PARAMS)
def test_first_middle_and_last_size_of_every_shift(shared, cus, shift):
    """The first n of the shift, one with a ragged last bin, the last (shift 6: n = 1, 2, 63, 64, 65, one block of counters exactly, one bin more, 8193
    bins too): 2000 random pairs with positions 0 and n - 1 among them; and the only pair of an input on position 0, on position n - 1."""
    got = oe.group("size", 8 * cus, shift)
    assert len(got) == (13 if shift == 6 else 5)
    for c in got:
        run_probe(shared, c)


@pytest.mark.parametrize("shift", SHIFT_PARAMS)
def test_bins_of_64_and_65_pairs_full_bins_and_bin_ends_around_a_block_of_counters_and_the_8_deep_front(shared, cus, shift):
    """0, 1, 2, 63, 64, 65, min(2^shift, 4096) pairs, a full bin (from shift 13: its first 33 and last 33 positions and every 97th) and a pair on the first
    and the last position, each in bin 0, 1, 1023, 1024, 1025 (the second block of the offsets pass), 8191, 8192, 8193 (the first block whose front sum runs
    eight loads deep), the last bin of the last whole block and the ragged last bin; ascending, descending and random input.  From shift 14 a thread of
    the rank pass owns two, at 15 four words of the bitmap, and the crowded bins set bits in its last quarter."""
    got = oe.group("bins", 8 * cus, shift)
    assert len(got) == len(oe.occupancies(shift))
    for c in got:
        run_probe(shared, c)


@pytest.mark.parametrize("label", oe.CROWDED_LABELS)
def test_more_crowded_bins_than_blocks(shared, cus, label):
    """1, grid - 1, grid, grid + 1 and 2 grid + 3 bins of 65 pairs at shift 7: a block of the rank pass takes a second and a third crowded bin"""
    grid = 8 * cus
    c = oe.group("crowded", grid)[oe.CROWDED_LABELS.index(label)]
    assert int(np.sum(c.histogram() > oe.kOrderCrowded)) == oe.crowded_counts(grid)[oe.CROWDED_LABELS.index(label)]
    run_probe(shared, c)


@pytest.mark.parametrize("label", oe.PAIRS_LABELS)
def test_more_pairs_than_one_grid_pass(shared, cus, label):
    """0, 1, 63 .. 65, 255 .. 257 pairs (a wave, a block), grid * 256 - 1 .. + 1 and 2 grid * 256 + 77: the count, scatter and rank pass go round their grids"""
    grid = 8 * cus
    c = oe.group("pairs", grid)[oe.PAIRS_LABELS.index(label)]
    assert c.count == oe.pair_counts(grid)[oe.PAIRS_LABELS.index(label)]
    run_probe(shared, c)


@pytest.mark.parametrize("shift", SHIFT_PARAMS)
def test_waves_whose_pairs_share_one_bin_or_lie_in_64_bins(shared, cus, shift):
    """The count and the scatter pass spend one atomic per distinct bin of a wave's 64 list entries: 64 distinct bins, and one"""
    striped, clumped = oe.group("waves", 8 * cus, shift)
    run_probe(shared, striped)
    run_probe(shared, clumped)


@pytest.mark.parametrize("shift", SHIFT_PARAMS)
def test_a_fresh_handle_per_call(workdir, cus, shift):
    """Every size again, each on a handle of its own: the probe's plan makes the scratch, the grid follows the scratch of that one call
    (at shift 7 also 300 crowded bins: more than those blocks)."""
    todo = [c for c in oe.group("size", 8 * cus, shift) if c.count > 1 or c.n <= 2]
    if shift == 7:
        todo += oe.group("fresh", 8 * cus)
        assert oe.grid_for(cus, oe.capacity_fresh(todo[-2].n, todo[-2].count)) < oe.FRESH_CROWDED_BINS
    assert len(todo) == len(oe.sizes(shift)) + (2 if shift == 7 else 0)
    for c in todo:
        h = new_handle(workdir)
        try:
            run_probe(h, c)
            assert h.info().deviceScratchBytes >= oe.reserve_bytes(c.n, c.count)
        finally:
            h.destroy()


def test_bad_arguments(shared):
    d = torch.full((8,), -5, dtype=torch.int32, device="cuda:0")
    bad = api.STATUS.INVALID_PARAMETER
    assert api.order_pairs_probe(shared, d.data_ptr(), d.data_ptr() + 16, 0, 100) == api.STATUS.SUCCESS
    assert api.order_pairs_probe(shared, None, None, 0, 100) == api.STATUS.SUCCESS
    for args in ((d.data_ptr(), d.data_ptr() + 16, 1, 0), (d.data_ptr(), d.data_ptr() + 16, 1, 1 << 31), (d.data_ptr(), d.data_ptr() + 16, 4, 3),
                 (None, d.data_ptr(), 1, 100), (d.data_ptr(), None, 1, 100)):
        assert api.order_pairs_probe(shared, *args, check=False) == bad, args
    torch.cuda.synchronize()
    assert int(d.min()) == -5 and int(d.max()) == -5


# ---------------------------------------------------------------------------------------------------------------------- real calls

@functools.lru_cache(maxsize=None)
def oracle_result(pf, n):
    """the oracle's result vector of real_input(n) / hygiene_input() (n == 0): once per module"""
    from oracle import binding as ob
    o = ob.Oracle(pf, hashed=False)
    try:
        return o.match(oe.real_input(n) if n else oe.hygiene_input())
    finally:
        o.close()


def test_probe_and_real_calls_alternate_on_one_handle(workdir):
    """Counter hygiene: a real call skips its memset when the call before it left the same layout clean, and calls alternate between two pairs of
    counters; the probe leaves `not clean` behind and does not flip the parity.  real, real (clean layout: no memset), the probe at another n, real, the
    probe at the real call's n, real, real -- every real call's pairs are the oracle's."""
    h = new_handle(workdir)
    try:
        data = oe.hygiene_input()
        want = oracle_result(pattern_file(workdir), 0)
        assert np.count_nonzero(want) > 4000 and np.bincount(np.flatnonzero(want) >> 6).max() == 64
        other = oe.group("bins", shift=9)[5]
        same = oe.Case("hygiene", "the real call's n", data.size, oe._sample(data.size, 3000, oe._rng("hygiene probe")), "random")
        assert oe.plan(data.size)["shift"] == 6 and other.n != data.size
        for step in ("real", "real", other, "real", same, "real", "real"):
            if step == "real":
                assert_pairs(device_reduce(h, data), want, "a real call")
            else:
                run_probe(h, step)
    finally:
        h.destroy()


def test_as_many_pairs_as_a_first_call_s_scratch_holds_and_one_more(workdir):
    """n bytes of `h` under the one pattern `h` are n pairs.  n = capacity_fresh(n, 65536) -- a first call of this size plans for 65536 pairs -- fits in
    one round; n + 1 leaves the launches at once and goes through the second round behind a larger scratch.  Both return positions 0 .. n - 1 in order;
    PFACX_getInfo's deviceScratchBytes (all of the handle's scratch) stays below what the second round reserves in the first call only."""
    pf = pattern_file(workdir, "only_h", (b"h",))
    n0 = oe.capacity_edge()
    assert oe.capacity_fresh(n0, 65536) == n0 and oe.capacity_fresh(n0 + 1, 65536) == n0
    second_round = oe.reserve_bytes(n0 + 1, n0 + 1)
    scratch = []
    for n in (n0, n0 + 1):
        h = make_handle(pf, api.PFAC_SPACE_DRIVEN, api.PFAC_AUTOMATIC, api.PFACX_KERNEL_AUTO)
        try:
            pos, ids = device_reduce(h, np.full(n, ord("h"), dtype=np.uint8))
            assert np.array_equal(pos, np.arange(n)) and np.all(ids == 1), n
            scratch.append(int(h.info().deviceScratchBytes))
        finally:
            h.destroy()
    print("deviceScratchBytes", scratch, "second round reserves", second_round)
    assert oe.reserve_bytes(n0, 65536) <= scratch[0] < second_round <= scratch[1], (scratch, second_round)


def check_real(workdir, n):
    data = oe.real_input(n)
    want = oracle_result(pattern_file(workdir), n)
    p = oe.plan(n)
    nz = np.flatnonzero(want)
    hist = np.bincount(nz >> p["shift"], minlength=p["bins"])
    for what, (b, k) in oe.real_plants(n).items():
        assert hist[b] == k, (what, b, int(hist[b]), k)
    assert nz[0] == 0 and nz[-1] == n - 1 and nz.size > n // 2000
    for variant, name in ((api.PFACX_KERNEL_AUTO, "auto"), (api.PFACX_KERNEL_FILTER, "filter")):
        h = new_handle(workdir, variant)
        try:
            for call in range(2):                    # the second call finds the layout clean
                assert_pairs(device_reduce(h, data), want, f"n {n}/{name}/call {call}")
        finally:
            h.destroy()


@pytest.mark.parametrize("n", oe.REAL_SIZES)
def test_real_scans_at_the_smallest_sizes_of_shifts_6_to_8(workdir, n):
    """2^22 - 1 and 2^22 (shift 6: 2^16 bins), 2^22 + 1 (shift 7), 2^23 + 1 (shift 8) through the scans themselves, which append in the order their walks
    end (the filter kernel far more scrambled than the tiled one): filler with `h`, `ab`, `abc`, `mnop` planted so that one bin holds 64 pairs and its
    neighbour 65 (shift 6: 63 and 64), one bin is full of `h`, positions 0 and n - 1 match, bins 1023, 1024 and the last are occupied -- asserted on the
    oracle's result, which is the expected value."""
    check_real(workdir, n)


def test_real_scan_at_the_smallest_size_of_shift_9(workdir):
    check_real(workdir, oe.REAL_BIG)
