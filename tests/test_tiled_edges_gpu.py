"""pfac_scan_tiled (scan_tiled.hip) at its tile, halo, alignment and density edges, through full-result calls: the kernel of every
PFACX_KERNEL_AUTO call below 32 MiB, of PFACX_KERNEL_NAIVE, of the filter kernel's dense chunks and -- REF >= 0 -- of
PFACX_KERNEL_REFTABLE.  Groups are cut at 16-byte ADDRESSES (positions in front of the first input byte and behind the last owned one
are masked), 128 bytes are staged behind a group, results leave through the LDS tile (one-tile shape), whole zero lines or
per-position stores, a group's survivors are listed plainly (<= 256), `crowded` (> 256: 4 per lane and pass) or not at all (dense:
survivors * 2 >= owned positions), and the shape changes at 8 MiB owned (256 threads and 1 KiB groups; 1024 threads and 4 KiB -- the
reference-layout tables: 2 KiB -- groups).

Every expected value is the oracle's result on exactly the bytes the kernel was given (tests/tiled_edges.py: want), never a slice of
a longer run and never another kernel's.  Every call has poisoned result buffers whose surroundings must stay as they were, and the
device memory around the input holds bytes that would complete a match: a kernel that read them as input reports it.

Each case runs under two pattern sets (tests/tiled_edges.py: SETS).  Under "q" -- a 1-byte pattern in a small set -- the early-out
lets nine positions in ten through and every group is dense; under "qq" only `q` runs are, and the sparse paths run at the same
edges.  The kernel does not report which branch a group took: the survivor counts of the fixtures, pinned against the numpy model
of the early-out in tests/test_tiled_edges_host.py, are the evidence."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import tiled_edges as te  # noqa: E402
from tests.gpu_helpers import MODES, assert_pairs, assert_same, device_match, device_reduce, make_handle  # noqa: E402

NAIVE, AUTO, REFTABLE, FILTER = api.PFACX_KERNEL_NAIVE, api.PFACX_KERNEL_AUTO, api.PFACX_KERNEL_REFTABLE, api.PFACX_KERNEL_FILTER
VARIANT_NAMES = {NAIVE: "naive", AUTO: "auto", REFTABLE: "reftable", FILTER: "filter"}
TILED = [(NAIVE, "naive"), (AUTO, "auto"), (REFTABLE, "reftable")]
PLAIN_LOADS = [MODES[0], MODES[2]]               # dense-global, hash-global: the big shape of the reference-layout kernel has no buffer loads


@pytest.fixture(scope="module")
def handles():
    """handle(set name, variant, mode): one handle per combination for the whole file, as a caller keeps one across calls of every size"""
    made = {}

    def handle(name, variant, mode):
        key = (name, variant, mode[2])
        if key not in made:
            made[key] = make_handle(te.pattern_file(name), mode[0], mode[1], variant)
        return made[key]

    yield handle
    for h in made.values():
        h.destroy()


# ------------------------------------------------------------------------------------------------------------------------------- A

RAGGED_RUNS = [(NAIVE, MODES[1]), (NAIVE, MODES[2]), (AUTO, MODES[1]), (AUTO, MODES[2]),     # time-driven with buffer loads, space-driven without
               (REFTABLE, MODES[0]), (REFTABLE, MODES[3])]


@pytest.mark.parametrize("in_off", range(16))
def test_every_misalignment_at_ragged_sizes(handles, in_off):
    """A.  The input in_off bytes and the result 0..3 ints behind a 16-byte address, n around the 16-byte lane, the 1 KiB group, group
    plus halo and the four waves of a block -- as n, and as in_off + n (n <= 16 - in_off: the launch of scan() for an input that lies
    in front of the first aligned byte).  `q` runs at both ends (under "q" a match at 0 and at n - 1), a 60-byte pattern that needs 4
    bytes beyond n, `q`s in the device memory around the input.  For an aligned result, the compacted call on the same input too."""
    around = dict(front=te.Q, behind=b"q" * 64)
    for name in te.SETS:
        for n in te.ragged_sizes(in_off):
            data = te.ragged(n)
            want = te.want(data, name)
            for variant, mode in RAGGED_RUNS:
                h = handles(name, variant, mode)
                what = f"{name}/{VARIANT_NAMES[variant]}/{mode[2]}/in +{in_off}/n {n}"
                for out_off in range(4):
                    assert_same(device_match(h, data, in_off, out_off, **around), want, f"{what}/out +{out_off}")
                assert_pairs(device_reduce(h, data, in_off, **around), want, f"{what}/compacted")


# ------------------------------------------------------------------------------------------------------------------------------- B

@pytest.mark.parametrize("variant,variant_name", TILED)
@pytest.mark.parametrize("in_off,out_off", [(0, 0), (7, 1)])
def test_walks_across_every_group_and_halo_edge(handles, in_off, out_off, variant, variant_name):
    """B.  Small shape.  60-byte matches, near misses, the diverging twin and prefix-patterns across a 1 KiB group boundary at every
    offset 0..71; the 200- and 600-byte patterns, complete and with a wrong last byte, from 1..199 bytes in front of a group's end
    and ENDING 127, 128 and 129 bytes behind it (the last staged byte, the first from global memory, one further); a 600-byte match
    that ends at n and a pattern cut off by n whose rest lies behind the input.  At in_off 7 the boundaries lie at 1024 k - 7."""
    data, _ = te.walks(te.GROUP_SMALL, in_off)
    for name in te.SETS:
        want = te.want(data, name)
        for mode in MODES:
            got = device_match(handles(name, variant, mode), data, in_off, out_off, front=te.Q, behind=b"ABCDEFGH")
            assert_same(got, want, f"{name}/{variant_name}/{mode[2]}/+{in_off},+{out_off}")


# ------------------------------------------------------------------------------------------------------------------------------- C

@pytest.mark.parametrize("n", te.SWITCH_SIZES)
@pytest.mark.parametrize("in_off,out_off", [(0, 0), (5, 3)])
def test_both_sides_of_the_shape_switch(handles, in_off, out_off, n):
    """C.  8 MiB - 1 (small shape), 8 MiB and 8 MiB + 1 (big: ScanArgs::owned counts the whole input): B's plants relative to the
    4 KiB groups of the chained-table kernel (NAIVE, AUTO) and to the 2 KiB groups of the reference-layout one, dense stretches over
    the first group, the last (partial) one, one between sparse neighbours and ten in a row.  8 MiB + 1 also through
    PFACX_KERNEL_FILTER, whose dense chunks come back to the tiled kernel's list mode (owned 0, n the whole input)."""
    for group, runs in ((te.GROUP_BIG, [(NAIVE, MODES), (AUTO, MODES)] + ([(FILTER, MODES[1:3])] if n > te.BIG_BYTES else [])),
                        (te.GROUP_REF, [(REFTABLE, PLAIN_LOADS)])):
        data = te.shape_switch(group, in_off)[0][:n]
        for name in te.SETS:
            want = te.want(data, name, omp=True)
            for variant, modes in runs:
                for mode in modes:
                    got = device_match(handles(name, variant, mode), data, in_off, out_off, front=te.Q, behind=b"z" * 8)
                    assert_same(got, want, f"{name}/{VARIANT_NAMES[variant]}/{mode[2]}/n {n}/+{in_off},+{out_off}")


# ------------------------------------------------------------------------------------------------------------------------------- D

@pytest.mark.parametrize("variant,variant_name", TILED)
def test_groups_on_either_side_of_the_crowded_and_dense_thresholds(handles, variant, variant_name):
    """D, small shape.  1 KiB groups with exactly 255, 256, 257 (plain | crowded), 511, 512, 513 (crowded | dense) and 1024 survivors
    under "qq", and two crowded groups of ~330: one with 19 lanes that hold all 16 positions of their bytes, one with about 5 in every
    lane.  Which branch a group takes is not reported: the counts -- asserted against the model of the early-out in
    test_tiled_edges_host.py -- are the evidence.  Full and compacted output against the oracle."""
    data, _ = te.thresholds_small()
    for name in te.SETS:
        want = te.want(data, name)
        for mode in MODES:
            h = handles(name, variant, mode)
            assert_same(device_match(h, data, front=te.Q, behind=b"q" * 8), want, f"{name}/{variant_name}/{mode[2]}")
            assert_pairs(device_reduce(h, data, front=te.Q, behind=b"q" * 8), want, f"{name}/{variant_name}/{mode[2]}/compacted")


@pytest.fixture(scope="module")
def big_thresholds():
    data, _ = te.thresholds_big()
    return data, te.want(data, "qq", omp=True)


@pytest.mark.parametrize("variant,variant_name", TILED)
def test_big_shape_groups_on_either_side_of_the_dense_threshold(handles, big_thresholds, variant, variant_name):
    """D, big shape (exactly 8 MiB, aligned).  4 KiB groups with 2047, 2048 and 2049 survivors -- the chained-table kernel's -- and 2 KiB
    groups with 1023, 1024 and 1025 -- the reference-layout kernel's -- under "qq"; full and compacted output against the oracle."""
    data, want = big_thresholds
    for mode in (PLAIN_LOADS if variant == REFTABLE else MODES):
        h = handles("qq", variant, mode)
        assert_same(device_match(h, data), want, f"{variant_name}/{mode[2]}")
        assert_pairs(device_reduce(h, data), want, f"{variant_name}/{mode[2]}/compacted")


# ------------------------------------------------------------------------------------------------------------------------------- E

@pytest.mark.parametrize("seed", range(8))
def test_fuzzed_pattern_sets_through_the_tiled_kernel(workdir, seed):
    """E.  The generator of test_fuzzed_pattern_sets_over_tiny_alphabets (tiny alphabets, 1- and 2-byte patterns, bytes 0x00 and 0xFF,
    almost every position walks) through NAIVE, AUTO and REFTABLE in all four modes, at offset (seed % 16, seed % 4), full and
    compacted."""
    from oracle import binding as ob
    pf, data = te.fuzz_case(workdir, seed)
    o = ob.Oracle(pf, hashed=False)
    want = o.match(data)
    o.close()
    in_off, out_off = seed % 16, seed % 4
    for variant, variant_name in TILED:
        for mode in MODES:
            h = make_handle(pf, mode[0], mode[1], variant)
            try:
                what = f"fuzz seed {seed}/{variant_name}/{mode[2]}"
                assert_same(device_match(h, data, in_off, out_off), want, what)
                assert_pairs(device_reduce(h, data, in_off), want, what + "/compacted")
            finally:
                h.destroy()
