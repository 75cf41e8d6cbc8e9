"""PFACX_countPairsFromDevice where pfac_count_hist takes another path: the cases of tests/count_edges.py, families C and D built for this
device's compute units and their claims checked again, through guarded_count -- the list `shift` ints into a 16-byte aligned allocation
with a VALID id in every int around it, poison words on both sides of counts[0, F], with PFACX_COUNT_LONGEST against np.bincount and
without it against count_ref.counts_from_result over the set's prefix table (every set here has chains), each again with
PFACX_COUNT_ACCUMULATE over a preset that carries into the high word, the counts exact, the list and its surroundings unchanged.
tests/test_count_edges_host.py pins what every case reaches.

    A  shift 0 .. 3 x 1 .. 9 and 1020 .. 1029 ids, lists of one run, junk at both ends: the 16-byte load of a quad
    B  runs from every k to every k' of the same lane, the next, two lanes on and lane 63; runs that fill a wave, over a wave and a trip
       boundary, cut by junk; alternating ids
    C  pass - 1 .. pass + 1, 3 pass + 5 (1.6 M ints on 256 compute units, also compared with torch.bincount on the device), the second
       trip of one thread, the block without a quad, the block of the alignment's quad
    D  F = 16384 and 16385: ids of one slot of the tagged cache, slots 0 and 8191, every id, a slot claimed in one trip and hit in the next
    E  F = 16383 and 16384: id F in the last LDS word and through the cache, F + 1 dropped in both

Wall time on an MI355X (256 compute units), one run of the 267 tests together with tests/test_count_gpu.py, 8.4 s with the imports: this
module 1.6 s -- the four handles, the three 16 K sets among them, 1.12 s (the setup of the first case); the cases built for the device and
the claims of families C and D 0.34 s (inside C-pass-1, the slowest case); the test that reuses one handle 0.03 s; the lists of 0.5 M to
1.6 M ints of families C and D 0.01 .. 0.03 s each; every other case below 5 ms.  test_count_gpu's
test_id_lists_at_every_alignment_and_length took 0.02 s in the same run."""
import numpy as np
import pytest
import torch                              # before the library loads its HIP runtime, as in every GPU test module

from pfac_amd import api  # noqa: E402
from pfac_amd import workloads as wl  # noqa: E402
from tests import count_edges as ce  # noqa: E402
from tests import count_ref as ref  # noqa: E402
from tests import scale_sets as ss  # noqa: E402
from tests.gpu_helpers import make_handle  # noqa: E402
from tests.spans_helpers import pattern_file  # noqa: E402
from tests.test_count_gpu import ACCUMULATE, GUARD, LONGEST, counts_tensor, gpu_handle, prefix_of, read_counts  # noqa: E402

pytestmark = pytest.mark.gpu

FIVE_PATTERNS = (b"ab", b"abc", b"abd", b"x", b"abcq")         # chains: abcq -> abc -> ab
BEHIND = 8                                                     # ints behind the list: two quads that a load past `end` would take
ON_DEVICE = 100000                                             # lists from this size on are compared with torch.bincount as well


class Set:
    """a handle and what the reference needs of its patterns"""

    def __init__(self, h, pats):
        self.h, self.f, self.table = h, len(pats), prefix_of(tuple(pats))
        assert int(h.info().numOfPatterns) == self.f
        self.chains = int(np.max(self.table[1])) > 1
        assert int(h.info().maxMatchesPerPosition) == int(np.max(self.table[1]))
        # a preset that carries into the high word with whatever is added; entry 0 is the caller's
        self.preset = np.full(self.f + 1, 0xFFFFFFFF, dtype=np.uint64)
        self.preset[0] = 7


def five_handle(workdir, name):
    return gpu_handle(pattern_file(workdir, name, list(FIVE_PATTERNS)))


@pytest.fixture(scope="module")
def sets(workdir):
    """F -> Set: the five-pattern set and the first 16383, 16384 and 16385 patterns of the 100 000, each built once"""
    out = {ce.FIVE: Set(five_handle(workdir, "count-edges"), FIVE_PATTERNS)}
    for f in ce.SETS[1:]:
        pats = tuple(ss.patterns(ss.S100)[:f])
        pf = wl.write_pattern_file(ss.scratch_path("count_edges_first%d.pat" % f), list(pats))
        out[f] = Set(make_handle(pf, api.PFAC_SPACE_DRIVEN, api.PFAC_TEXTURE_OFF, api.PFACX_KERNEL_AUTO), pats)
    assert all(s.chains for s in out.values()), "every set has a pattern that is a prefix of another: both forms are run"
    yield out
    for s in out.values():
        s.h.destroy()


@pytest.fixture(scope="module")
def cases(sets):
    """family -> name -> case, built for this device"""
    units = int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert units == int(sets[ce.FIVE].h.info().multiProcessorCount), "the library and torch see the same device"
    built = ce.families(units)
    for family in ("C", "D"):
        for case in built[family]:
            ce.check_claims(case, units)
    assert {family: tuple(c[0] for c in members) for family, members in built.items()} == ce.NAMES
    return {family: ce.by_name(members) for family, members in built.items()}


def guarded_count(s, case):
    """every form of the call over one case; asserts everything the module's docstring lists"""
    name, ids, shift, f = case
    assert f == s.f
    count = int(ids.size)
    around = np.concatenate([np.full(shift, ce.OUTSIDE, dtype=np.int32), ids, np.full(BEHIND, ce.OUTSIDE, dtype=np.int32)])
    d_all = torch.from_numpy(around).to("cuda:0")
    d_ids = d_all.data_ptr() + 4 * shift
    assert d_all.data_ptr() % 16 == 0 and (d_ids % 16) // 4 == shift, "the list is as far off a 16-byte boundary as the case says"
    valid = ids[(ids >= 1) & (ids <= f)]
    assert np.array_equal(ref.counts_from_result(valid, s.table, True), case.want()), "the two references of the plain histogram"
    if count >= ON_DEVICE:
        inside = d_all[shift:shift + count]
        on_device = torch.bincount(inside[(inside >= 1) & (inside <= f)], minlength=f + 1)
    for longest in ((True, False) if s.chains else (True,)):
        want = ref.counts_from_result(valid, s.table, longest)
        assert want[0] == 0
        for accumulate in (False, True):
            what = f"{name}/longest {longest}/accumulate {accumulate}"
            d = counts_tensor(f, s.preset if accumulate else None)
            flags = (LONGEST if longest else 0) | (ACCUMULATE if accumulate else 0)
            assert s.h.countPairsFromDevice(d_ids, count, flags, d.data_ptr() + 8 * GUARD, f + 1) == 0, what
            if count >= ON_DEVICE and longest and not accumulate:
                torch.cuda.synchronize()
                assert torch.equal(d[GUARD:GUARD + f + 1], on_device), f"{what}: differs from torch.bincount"
            got = read_counts(d, f)
            if accumulate:
                assert got[0] == s.preset[0], f"{what}: entry 0 is the caller's"
                ref.same(got[1:], s.preset[1:] + want[1:], what)
                assert np.all(got[1:][want[1:] != 0] >> np.uint64(32) == 1), f"{what}: the carry into the high word"
            else:
                ref.same(got, want, what)
    assert np.array_equal(d_all.cpu().numpy(), around), f"{name}: the id list or the ints around it were modified"


def run_family(sets, cases, family, name):
    case = cases[family][name]
    guarded_count(sets[case[3]], case)


@pytest.mark.parametrize("name", ce.NAMES["A"])
def test_quads_cut_on_the_address(sets, cases, name):
    """loadQuad's 16-byte load at the first and at the last quad of a list at every shift: an int outside the list is a valid id"""
    run_family(sets, cases, "A", name)


@pytest.mark.parametrize("name", ce.NAMES["B"])
def test_runs_inside_and_across_waves(sets, cases, name):
    """heads, any, above, nextLane, first, next and run: from every k to every k', over lanes without a head, to a wave's end and past it"""
    run_family(sets, cases, "B", name)


@pytest.mark.parametrize("name", ce.NAMES["C"])
def test_trips_and_the_grid(sets, cases, name):
    """both sides of one pass of the grid, four trips of a block, the trip of one thread, the block without a quad"""
    run_family(sets, cases, "C", name)


@pytest.mark.parametrize("name", ce.NAMES["D"])
def test_ids_by_their_slot_of_the_tagged_cache(sets, cases, name):
    """claim, hit, the loser's global atomic and the flush: two, three and four ids of a slot, slots 0 and 8191, a slot claimed in a block's
    first trip and hit in its second"""
    run_family(sets, cases, "D", name)


@pytest.mark.parametrize("name", ce.NAMES["E"])
def test_the_last_id_on_both_sides_of_the_threshold(sets, cases, name):
    """F + 1 == 16384: id F in lds[16383]; F == 16384: the same list through the cache; id F + 1 is dropped in both"""
    run_family(sets, cases, "E", name)


def test_a_short_list_behind_a_long_one_on_one_handle(workdir, cases):
    """L and the word of the total are the handle's: behind 3 passes and 5 ids a list of nine finds them used; trim() in between; then both
    once more"""
    s = Set(five_handle(workdir, "count-edges-reuse"), FIVE_PATTERNS)
    try:
        big, small = cases["C"]["C-3pass+5"], cases["A"]["A-shift1-9"]
        guarded_count(s, big)
        grown = s.h.info().deviceScratchBytes
        guarded_count(s, small)
        assert s.h.info().deviceScratchBytes == grown, "the shorter list needs no more"
        s.h.trim()
        assert s.h.info().deviceScratchBytes < grown
        for case in (big, small):
            guarded_count(s, case)
        assert s.h.info().deviceScratchBytes == grown, "a second call of the same shape allocates what the first did"
    finally:
        s.h.destroy()
