"""tests/count_edges.py without a GPU and without a handle: the constants are the sources'; every case's claims hold for the grid it was
built with, 1, 256 and 304 compute units; the plain Python transcription of pfac_count_hist (hist_model) equals np.bincount in both orders
of the cache's claims and writes nowhere else; and every named off-by-one of the transcription changes the histogram of a case of the
family that claims its edge, or makes the model write outside its words -- but for the five that provably change no count
(count_edges.equivalent_mutants), which are pinned as such, each beside a neighbour that is caught.  The device form runs the same cases in
tests/test_count_edges_gpu.py.

Families C and D are built for a device; here their twins for one compute unit stand in: the same builders, a pass of 2048 ids for
524 288."""
import functools
import os

import numpy as np
import pytest

from pfac_amd import api
from tests import count_edges as ce

CSRC = os.path.join(os.path.dirname(os.path.abspath(api.__file__)), "csrc")
ORDERS = ("ascending", "descending")

# mutant -> the family whose cases must tell it from the kernel, and the cases that do by hand
CAUGHT_BY = {
    "quad_le_plus_1": ("A", {"A-shift0-3", "A-shift3-1020"}),                 # j + 4 == end + 1: the 16-byte load takes the int behind the list
    "quad_ge_minus_1": ("A", {"A-shift1-3", "A-shift1-one-run-1025"}),        # j == shift - 1: ... the int in front of it
    "lane0_not_forced": ("B", {"B-shift%d-run-of-256-fills-a-wave" % s for s in ce.B_SHIFTS}),      # lane 0 all equal: nobody heads the run
    "next_drops_first": ("B", {"B-shift%d-k0-to-next-lane-k%d" % (s, k) for s in ce.B_SHIFTS for k in range(3)}),     # the next head is k + 1 of its lane
    "above_includes_own": ("B", {"B-shift0-k0-to-same-lane-k0", "B-shift3-alternating-ids"}),
    "last_run_63": ("B", {"B-shift%d-%s" % (s, n) for s in ce.B_SHIFTS for n in ("last-run-of-a-wave", "last-run-ends-the-list")}),
    "filter_le": ("E", {"E-F16383-id-F-and-F+1-alternating", "E-F16383-F-1-F-F+1-in-runs"}),        # a stray write: lds[16384]
    "no_second_trip": ("C", {"C-pass+1", "C-3pass+5", "C-pass-2-shift3", "C-id-in-every-trip", "C-one-run"}),
    "loser_dropped": ("D", {"D-F%d-%s" % (f, n) for f in ce.D_SETS for n in (ce.D_LISTS[0], ce.D_LISTS[2], ce.D_LISTS[7])}),
    "filter_le_flush_unchecked": ("D", {"D-F%d-id-F-among-junk" % f for f in ce.D_SETS}),           # a stray write: hist[F + 1]
}


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def built(compute_units):
    return ce.families(compute_units)


@functools.lru_cache(maxsize=None)
def outcome(family, name, order, mutate=None):
    """(the model's histogram as bytes, its stray writes) of a case of the one-unit twin"""
    case = ce.by_name(built(1)[family])[name]
    hist, stray = ce.hist_model(case[1], case[2], case[3], ce.launch_grid(case[1].size, 1), order, mutate)
    return hist.tobytes(), tuple(stray)


def differs(family, case, mutate):
    """the orders in which the mutant's outcome is not the reference's"""
    want = (case.want().tobytes(), ())
    return [order for order in ORDERS if outcome(family, case[0], order, mutate) != want]


# ---------------------------------------------------------------------------------------------------------------- the constants

def test_the_constants_are_the_sources():
    count, passes = source("scan_count.hip"), source("scan_passes.h")
    assert (ce.THREADS, ce.PER, ce.TRIP, ce.WAVE, ce.LDS_WORDS, ce.CACHE_LOG2, ce.SLOTS, ce.BLOCKS_PER_CU) == (256, 4, 1024, 256, 16384, 13, 8192, 2)
    assert api.PFACX_COUNT_LDS_DIRECT == 16384 == ce.LDS_WORDS and 2 * ce.SLOTS == ce.LDS_WORDS
    for text in ("constexpr unsigned int kCountThreads = %d;" % ce.THREADS,
                 "constexpr unsigned int kCountPer = %d;" % ce.PER,
                 "constexpr unsigned int kCountTrip = kCountThreads * kCountPer;",
                 "constexpr unsigned int kCountLdsWords = %d;" % ce.LDS_WORDS,
                 "constexpr unsigned int kCountDirect = kCountLdsWords;",
                 "constexpr unsigned int kCountCacheLog2 = %d;" % ce.CACHE_LOG2,
                 "constexpr unsigned int kCountCacheSlots = 1u << kCountCacheLog2;",
                 "const unsigned int slot = (id * 0x%Xu) >> (32 - kCountCacheLog2);" % ce.MULTIPLIER,
                 # the launch
                 "const size_t trips = (count + 2 * kCountPer + kCountTrip - 1) / kCountTrip;",
                 "const unsigned int grid = (unsigned int)(trips < gridCap(c, %d) ? trips : gridCap(c, %d));" % (ce.BLOCKS_PER_CU, ce.BLOCKS_PER_CU),
                 "if (F + 1 <= kCountDirect) hipLaunchKernelGGL(pfac_count_hist<true>, dim3(grid), dim3(kCountThreads), 0, 0, h);",
                 # loadQuad, as the mutants name it
                 "const size_t j = q * kCountPer, end = (size_t)shift + a.count;",
                 "if (j >= shift && j + kCountPer <= end) {",
                 "v[k] = j + k >= shift && j + k < end ? (unsigned int)aligned[j + k] : 0u;",
                 "v[k] = v[k] - 1u < a.numIds ? v[k] : 0u;",
                 # the wave
                 "for (size_t q0 = (size_t)blockIdx.x * kCountThreads; q0 < quads; q0 += (size_t)gridDim.x * kCountThreads) {",
                 "const unsigned int prev = (unsigned int)__shfl_up((int)v[kCountPer - 1], 1);",
                 "head[0] = lane == 0 || v[0] != prev;",
                 "const unsigned long long above = lane == 63u ? 0ull : any & (~0ull << (lane + 1u));",
                 "const unsigned int nextLane = above ? (unsigned int)__ffsll((long long)above) - 1u : 0u;",
                 "unsigned int next = above ? nextLane * kCountPer + firstThere : 64u * kCountPer;",
                 # the counters
                 "const unsigned int used = DIRECT ? a.numIds + 1u : kCountLdsWords;",
                 "const unsigned int owner = atomicCAS(&lds[slot], 0u, id);",
                 "if (owner == 0u || owner == id) atomicAdd(&lds[kCountCacheSlots + slot], run);",
                 "else atomicAdd(&a.hist[id], run);",
                 "if (c != 0 && id - 1u < a.numIds) atomicAdd(&a.hist[id], c);"):
        assert text in count, text
    assert ("inline unsigned int gridCap(const PFAC_context *c, unsigned int perCu) { return (unsigned int)(c->multiProcessorCount > 0 ? "
            "c->multiProcessorCount : 256) * perCu; }") in passes
    assert set(ce.MUTANTS) == set(CAUGHT_BY) | set(ce.equivalent_mutants())
    assert all(near in CAUGHT_BY for _, near in ce.equivalent_mutants().values()), "the neighbour of an equivalent mutant is one that is caught"


def test_the_names_do_not_depend_on_the_device():
    for units in (1, 256, 304):
        assert {f: tuple(c[0] for c in cases) for f, cases in built(units).items()} == ce.NAMES
    assert ce.NAMES["C"] == ce.C_NAMES
    assert ce.NAMES["D"] == tuple("D-F%d-%s" % (f, n) for f in ce.D_SETS for n in ce.D_LISTS)
    assert ce.NAMES["E"] == tuple("E-F%d-%s" % (f, n) for f in ce.E_SETS for n in ce.E_LISTS)
    assert {f: len(names) for f, names in ce.NAMES.items()} == {"A": 99, "B": 136, "C": 9, "D": 16, "E": 6}
    assert len({n for names in ce.NAMES.values() for n in names}) == 266


# ---------------------------------------------------------------------------------------------------------------- the reference, the slots

def test_the_histogram_by_hand():
    assert ce.histogram([1, 1, 0, -1, 6, 5, ce.INT_MIN, ce.INT_MAX, 5, 2], 5).tolist() == [0, 2, 1, 0, 0, 2]
    assert ce.histogram([16384, 16385, 16383], 16383).tolist()[-2:] == [0, 1] and ce.histogram([0, -1], 5).sum() == 0


def test_the_slots_family_d_relies_on():
    by = ce.check_slots()
    assert sum(len(v) for v in by.values()) == 16384
    assert ce.slot_of(1) == 0x9E3779B1 >> 19 and ce.slot_of(4181) == 0 and ce.slot_of(6765) == 8191
    assert ce.slot_of(16385) not in (0, 8191) and len(ce.slots(16385)[ce.slot_of(16385)]) <= 4
    d = ce.by_name(built(1)["D"])
    four = [c for c in d["D-F16384-a-full-slot-interleaved"].claims if c[0] == "whole_slot"][0]
    assert len(four) == 2 + 4, "a fullest slot: four ids"


# ---------------------------------------------------------------------------------------------------------------- the claims

@pytest.mark.parametrize("compute_units", [256, 1, 304])
@pytest.mark.parametrize("family", sorted(ce.NAMES))
def test_every_claim_holds_for_its_grid(family, compute_units):
    for case in built(compute_units)[family]:
        ce.check_claims(case, compute_units)


def test_a_claim_that_does_not_hold_is_told():
    """claim_holds is no rubber stamp: claims of one case asked of another"""
    b = ce.by_name(built(1)["B"])
    assert not ce.claim_holds(b["B-shift0-k0-to-next-lane-k1"], ("run", ce.B_LANE, 0, ce.B_LANE + 1, 2), 1)
    assert not ce.claim_holds(b["B-shift0-k0-to-next-lane-k1"], ("no_head", ce.B_LANE + 1), 1)
    assert not ce.claim_holds(b["B-shift0-run-over-255|256"], ("spans", 512, "wave"), 1)
    assert not ce.claim_holds(b["B-shift0-run-of-257-from-a-wave's-first"], ("fills_wave",), 1)
    c = ce.by_name(built(1)["C"])
    assert not ce.claim_holds(c["C-pass"], ("trips", 0, 2), 1) and not ce.claim_holds(c["C-pass"], ("no_quad",), 1)
    assert not ce.claim_holds(c["C-3pass+5"], ("in_every_trip", 3, 0, 4), 1)
    d = ce.by_name(built(1)["D"])
    assert not ce.claim_holds(d["D-F16384-two-ids-of-a-slot-alternating"], ("share_slot", 0, 4181, 6765), 1)
    x, y = d["D-F16384-claimed-in-trip-0-hit-in-trip-1"].claims[0][2:]
    assert not ce.claim_holds(d["D-F16384-claimed-in-trip-0-hit-in-trip-1"], ("claimed_then_hit", 0, y, x), 1)
    assert not ce.claim_holds(d["D-F16384-claimed-in-trip-0-hit-in-trip-1"], ("claimed_then_hit", 0, x, y), 256), "built for another grid"


def test_what_the_full_size_cases_reach_on_256_compute_units():
    """by hand, for the device the sizes were chosen for"""
    c, d = ce.by_name(built(256)["C"]), ce.by_name(built(256)["D"])
    one = 524288
    assert [int(c[n][1].size) for n in ce.C_NAMES] == [one - 1, one, one + 1, 3 * one + 5, one - 2, 511 * 1024, 511 * 1024 - 2, 3 * one + 5, 2 * one + 7]
    assert [ce.launch_grid(int(c[n][1].size), 256) for n in ce.C_NAMES] == [512] * 9
    assert max(int(case[1].size) for case in built(256)["C"]) == 1572869, "about 1.6 M ints"
    assert int(d["D-F16385-claimed-in-trip-0-hit-in-trip-1"][1].size) == one + 1024
    assert ce.launch_grid(1024, 1) == 2 and ce.launch_grid(1022, 1) == 2 and ce.launch_grid(1016, 1) == 1, "the alignment's quad: 8 ids of slack"


# ---------------------------------------------------------------------------------------------------------------- the model

@pytest.mark.parametrize("family", sorted(ce.NAMES))
def test_the_model_is_the_bincount_in_both_claim_orders(family):
    for case in built(1)[family]:
        assert not differs(family, case, None), case[0]


def test_the_model_under_other_grids():
    """the trip loop: any number of blocks gives the same counts, one block and more blocks than the list has trips included"""
    for family, name in (("C", "C-3pass+5"), ("C", "C-id-in-every-trip"), ("D", "D-F16385-claimed-in-trip-0-hit-in-trip-1"), ("A", "A-shift3-9")):
        case = ce.by_name(built(1)[family])[name]
        for grid in (1, 3, 16):
            for order in ORDERS:
                hist, stray = ce.hist_model(case[1], case[2], case[3], grid, order)
                assert not stray and np.array_equal(hist, case.want()), (name, grid, order)


def test_the_claim_order_decides_who_owns_a_slot():
    """the race the `order` argument stands for is real in the model: with the loser dropped, the two orders lose DIFFERENT ids"""
    x, y = ce.check_slots()[0][:2]
    name = "D-F16384-two-ids-of-a-slot-alternating"                # lane 0 heads x, lane 1 heads y, both at k = 0
    left = [np.flatnonzero(np.frombuffer(outcome("D", name, order, "loser_dropped")[0], dtype=np.uint64)).tolist() for order in ORDERS]
    assert left == [[x], [y]]
    # ... where the lists of family D put the ids of a slot at different k, k = 3 is first in either order: the same winner
    name = "D-F16384-a-full-slot-interleaved"
    a, b = (np.frombuffer(outcome("D", name, order, "loser_dropped")[0], dtype=np.uint64) for order in ORDERS)
    assert np.flatnonzero(a).tolist() == np.flatnonzero(b).tolist() and np.count_nonzero(a) == 1


@pytest.mark.parametrize("mutant", sorted(CAUGHT_BY))
def test_every_mutant_is_caught_by_the_family_that_claims_its_edge(mutant):
    family, by_hand = CAUGHT_BY[mutant]
    caught = {case[0] for case in built(1)[family] if len(differs(family, case, mutant)) == len(ORDERS)}
    assert caught, "no case of family %s tells %s (%s) from the kernel" % (family, mutant, ce.MUTANTS[mutant])
    assert by_hand <= caught, (mutant, sorted(by_hand - caught))
    if mutant == "filter_le":
        # in cache mode the flush's check catches what the filter let through: no count changes, nothing is written outside
        assert not [case[0] for f in ("D", "E") for case in built(1)[f] if case[3] + 1 > ce.LDS_WORDS and differs(f, case, mutant)]
        stray = outcome("E", "E-F16383-id-F-and-F+1-alternating", "ascending", mutant)[1]
        assert set(stray) == {("lds", ce.LDS_WORDS)}, "id F + 1 is counted behind the last LDS word"
    if mutant == "filter_le_flush_unchecked":
        assert set(outcome("D", "D-F16384-id-F-among-junk", "ascending", mutant)[1]) == {("hist", 16385)}


@pytest.mark.parametrize("mutant", sorted(ce.equivalent_mutants()))
def test_the_equivalent_mutants_change_no_count(mutant):
    """quad_lt, quad_gt, raw_compare, owner_not_accepted and flush_unchecked (count_edges.equivalent_mutants says why): no list can catch
    them, so the claim is turned round and pinned over every family -- family A has the whole quads at either end of a list, family B the
    junk between and inside runs, family D the winners that come back and the tags.  A change to the kernel that makes one of them matter
    fails here and has to bring its case"""
    for family in sorted(ce.NAMES):
        for case in built(1)[family]:
            assert not differs(family, case, mutant), (mutant, case[0])
