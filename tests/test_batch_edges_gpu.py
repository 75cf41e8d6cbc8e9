"""The batch fix-up kernels (pfac_amd/csrc/scan_batch.hip) at their group, trip, zone, grid and block edges: PFACX_matchBatchFromDevice and
...FromDeviceReduce over the tables of tests/batch_edges.py against the brute force on every segment alone, exactly, with sentinel-filled
outputs between guard words (the pattern of tests/test_batch_gpu.py).  tests/test_batch_edges_host.py proves that each table reaches the code
its name says."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import batch_edges as be  # noqa: E402
from tests.gpu_helpers import MODES  # noqa: E402
from tests.segcount_ref import brute_seg_result  # noqa: E402
from tests.test_batch_gpu import GUARD, SENTINEL, check, device_batch  # noqa: E402

TWO_MODES = [MODES[0], MODES[3]]                 # dense table without, hashed table with buffer loads: both instantiations of every kernel
FULL_VARIANTS = [(api.PFACX_KERNEL_FILTER, "filter"), (api.PFACX_KERNEL_NAIVE, "naive")]
GROUPS = {
    "width": lambda: [be.width_case(k) for k in range(7)] + [be.width6_long_zone()],
    "trip": lambda: [be.trip_case(n) for n in range(1, 18)],
    "empties": lambda: [be.empties()],
    "long-slots": lambda: [be.long_slots()],
    "nocase": lambda: [be.nocase_case()],
}


def handle_for(case, perf, tex, variant=api.PFACX_KERNEL_AUTO):
    h = api.PFAC.create()
    h.setPerfMode(perf)
    h.setTextureMode(tex)
    h.setKernelVariant(variant)
    if case.nocase:
        h.readPatternFromFileEx(be.pattern_file(case.set), api.PFACX_READ_NOCASE)
    else:
        h.readPatternFromFile(be.pattern_file(case.set))
    return h


def reduce_edges(h, data, offsets):
    """matchBatchFromDeviceReduce -> (count, ids, positions, segFirst): every array sentinel-filled between GUARD ints on either side, the
    input followed by GUARD zero bytes"""
    n, nseg = int(data.size), len(offsets) - 1
    d_in = torch.zeros(n + GUARD, dtype=torch.uint8, device="cuda:0")
    d_in[:n] = torch.from_numpy(np.array(data, dtype=np.uint8)).to("cuda:0")
    d_ids = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    d_pos = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    d_first = torch.full((GUARD + nseg + 1 + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    d_off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64)).to("cuda:0")
    st, count = h.matchBatchFromDeviceReduce(d_in.data_ptr(), n, d_off.data_ptr(), nseg, d_ids.data_ptr() + 4 * GUARD, d_pos.data_ptr() + 4 * GUARD,
                                             d_first.data_ptr() + 4 * GUARD)
    torch.cuda.synchronize()
    assert st == 0
    ids, pos, first = d_ids.cpu().numpy(), d_pos.cpu().numpy(), d_first.cpu().numpy()
    for a, m in ((ids, n), (pos, n), (first, nseg + 1)):
        assert np.all(a[:GUARD] == SENTINEL) and np.all(a[GUARD + m:] == SENTINEL), "a guard word was written"
    assert 0 <= count <= n, count
    return count, ids[GUARD:GUARD + count], pos[GUARD:GUARD + count], first[GUARD:GUARD + nseg + 1]


def check_reduce(h, data, offsets, want, what):
    count, ids, pos, first = reduce_edges(h, data, offsets)
    nz = np.flatnonzero(want)
    assert count == nz.size, f"{what}: count {count} != {nz.size}"
    assert np.array_equal(pos, nz), f"{what}: positions"
    assert np.array_equal(ids, want[nz]), f"{what}: ids"
    want_first = np.searchsorted(nz, np.minimum(offsets, np.uint64(data.size)).astype(np.int64), side="left")
    assert np.array_equal(first, want_first), f"{what}: segFirst differs at segments {np.flatnonzero(first != want_first)[:4].tolist()}"
    return count, first


# ------------------------------------------------------------------------------------------------------------------- full result

@pytest.mark.parametrize("perf,tex,mode_name", MODES)
@pytest.mark.parametrize("variant,vname", FULL_VARIANTS)
@pytest.mark.parametrize("group", list(GROUPS))
def test_full_result(group, variant, vname, perf, tex, mode_name):
    cases = GROUPS[group]()
    handles = {}
    try:
        for case in cases:
            if case.set not in handles:
                handles[case.set] = handle_for(case, perf, tex, variant)
            check(device_batch(handles[case.set], case.data, case.offsets), be.reference(case), f"{case.name}/{vname}/{mode_name}")
    finally:
        for h in handles.values():
            h.destroy()


@pytest.mark.parametrize("perf,tex,mode_name", TWO_MODES)
@pytest.mark.parametrize("name", ["width-3", "long-slots", "empties"])
def test_full_result_misaligned_pointers(name, perf, tex, mode_name):
    case = {"width-3": be.width_case(3), "long-slots": be.long_slots(), "empties": be.empties()}[name]
    h = handle_for(case, perf, tex, api.PFACX_KERNEL_FILTER)
    try:
        for in_offset, out_offset in ((1, 0), (15, 0), (0, 1), (15, 1)):
            got = device_batch(h, case.data, case.offsets, in_offset=in_offset, out_offset=out_offset)
            check(got, be.reference(case), f"{name}/{mode_name}/input + {in_offset}, result + {out_offset} ints")
    finally:
        h.destroy()


@pytest.mark.parametrize("perf,tex,mode_name", TWO_MODES)
def test_grid_pass_more_segments_than_the_grid_takes_in_one_pass(perf, tex, mode_name):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = be.grid_pass(cus)
    assert len(case.offsets) - 1 > be.segments_per_pass(cus, be.case_group_log2(case))
    for k, want in be.brute_on_segments(case, be.sample_segments(case, 200)):
        assert np.array_equal(be.reference(case)[70 * k:70 * k + 70], want), k
    h = handle_for(case, perf, tex)
    try:
        check(device_batch(h, case.data, case.offsets), be.reference(case), f"grid-pass/{cus} compute units/{mode_name}")
    finally:
        h.destroy()


@pytest.mark.parametrize("perf,tex,mode_name", TWO_MODES)
def test_trip_tables_with_the_run_going_on_behind_the_last_offset(perf, tex, mode_name):
    """Under the contract the last segment ends with the input, where the scan itself stops every match: the fix-up of the LAST segment of a
    call -- the lane of a trip whose end offset is offsets[numSegments] -- changes nothing.  Here the buffer goes on for three more `a`
    behind the last offset, so the last segment ends inside a match like every other and needs its fix-up.  The positions behind the last
    offset belong to no segment: only their range is asserted."""
    case = be.trip_case(1)
    h = handle_for(case, perf, tex, api.PFACX_KERNEL_FILTER)
    try:
        for n in range(1, 18):
            case = be.trip_case(n)
            inside = case.data.size
            got = device_batch(h, np.concatenate([case.data, np.frombuffer(b"aaa", dtype=np.uint8)]), case.offsets)
            check(got[:inside], be.reference(case), f"{case.name} + 3 bytes/{mode_name}")
            assert np.all((got[inside:] >= 0) & (got[inside:] <= len(be.ARUN)))
    finally:
        h.destroy()


# -------------------------------------------------------------------------------------------------------------- compacted result

def _compacted_case(name):
    return {"empties": be.empties, "long-slots": be.long_slots, "nocase": be.nocase_case}[name]() if name in ("empties", "long-slots", "nocase") else be.pair_case(name)


@pytest.mark.parametrize("perf,tex,mode_name", TWO_MODES)
@pytest.mark.parametrize("name", list(be.PAIR_TABLES) + ["empties", "long-slots", "nocase"])
def test_compacted_result(name, perf, tex, mode_name):
    case = _compacted_case(name)
    h = handle_for(case, perf, tex)
    try:
        count, first = check_reduce(h, case.data, case.offsets, be.reference(case), f"{name}/{mode_name}")
        if name in be.CLAIMED:
            pairs, drops = be.CLAIMED[name]
            assert count == pairs - len(drops)
        if name in ("all-dropped", "no-pairs"):
            assert count == 0 and not first.any()
        check(device_batch(h, case.data, case.offsets), be.reference(case), f"{name}/{mode_name}/full result")
    finally:
        h.destroy()


# --------------------------------------------------------------------------------------------------- offsets outside the contract

def _in_range(h, case, offsets, what):
    """what include/pfac_ext.h promises for device offsets that break the rules: success, no write outside the arrays (the helpers' guards),
    and values in range"""
    patterns = len(be.SETS[case.set])
    got = device_batch(h, case.data, offsets)
    assert np.all((got >= 0) & (got <= patterns)), f"{what}: a result outside [0, {patterns}]"
    count, ids, pos, first = reduce_edges(h, case.data, offsets)
    assert 0 <= count <= case.data.size, what
    assert np.all((ids >= 0) & (ids <= patterns)) and np.all((pos >= 0) & (pos < case.data.size)), what
    assert np.all((first >= 0) & (first <= count)), f"{what}: segFirst outside [0, {count}]"


@pytest.mark.parametrize("perf,tex,mode_name", TWO_MODES)
def test_offsets_larger_than_the_size_are_clamped(perf, tex, mode_name):
    case = be.width_case(3)
    size = case.data.size
    offsets = case.offsets.copy()
    offsets[-3:] = np.array([size + 1, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)
    clamped = np.minimum(offsets, np.uint64(size))
    want = brute_seg_result(be.ARUN, case.data.tobytes(), clamped)
    h = handle_for(case, perf, tex)
    try:
        check(device_batch(h, case.data, offsets), want, f"offsets above the size/{mode_name}")
        check_reduce(h, case.data, offsets, want, f"offsets above the size/{mode_name}/compacted")
    finally:
        h.destroy()


@pytest.mark.parametrize("perf,tex,mode_name", TWO_MODES)
def test_arbitrary_offsets_stay_inside_the_buffers(perf, tex, mode_name):
    """Asserts a guarantee read off the code first (offsetAt clamps every offset, both binary searches run over [0, numSegments) and
    [0, count], a walk whose end lies in front of its start reads nothing); it is no search for a fault."""
    case = be.width_case(3)
    size = case.data.size
    good = case.offsets
    lens = be.segment_lengths(case)
    k = int(np.flatnonzero((lens[:-1] > 0) & (lens[1:] > 0))[3]) + 1
    bad = {}
    bad["a decreasing pair"] = good.copy()
    bad["a decreasing pair"][[k, k + 1]] = good[[k + 1, k]]
    bad["offsets[0] > 0"] = good.copy()
    bad["offsets[0] > 0"][0] = 5
    bad["last offset below the size"] = good.copy()
    bad["last offset below the size"][-1] = size - 7
    bad["shuffled"] = np.random.Generator(np.random.PCG64(77)).permutation(good)
    h = handle_for(case, perf, tex)
    try:
        for what, offsets in bad.items():
            assert not np.array_equal(offsets, good)
            _in_range(h, case, offsets, f"{what}/{mode_name}")
        check(device_batch(h, case.data, good), be.reference(case), f"well-formed call behind them/{mode_name}")
        check_reduce(h, case.data, good, be.reference(case), f"well-formed call behind them/{mode_name}/compacted")
    finally:
        h.destroy()
