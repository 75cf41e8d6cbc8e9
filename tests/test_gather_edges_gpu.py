"""PFACX_gatherLinesFromDevice where its kernels take another path: the cases of tests/gather_edges.py, built for this device's compute
units, through guarded_gather -- 64 bytes of 0xEE on BOTH sides of d_out, the input tensor ending with the input's last byte, status and
*h_outBytes always, the exact text of gather_edges.gather_text wherever the call is not truncated, only the guards where it is (the header
leaves the contents unspecified), the input and the line arrays unchanged.  tests/test_gather_edges_host.py pins what every case reaches.

    A, B   line starts around both bounds of a tile at three alignments of d_out; tiles that stage 4096 offsets; a tile inside one line
    C      sixteen line changes in one thread, a '\\n' as a thread's last and first byte at every alignment; texts that end inside a thread
    D      255 .. 513 lines and 8 C 256 - 1 .. + 1 lines: per 256 -> 512, two steps of pfac_array_scan (1.5 MiB of text on 256 compute units)
    E      520 lines of 64 KiB on 256 compute units, 32.5 MiB: 128 tiles more than one pass of the copy's grid, compared on the device;
           2^32 bytes of text into no room and into one tile
    F, G   lists out of order and hostile lists at capacities 0, 100 and full; the last line ends with the input's last byte

Wall time on an MI355X, one run of the 124 tests, 3 s with the imports: the first case 0.11 s (the first launches of the handle), family E's
32.5 MiB with its comparison on the device 0.06 s, the three large counts of family D and the test that reuses one handle 0.02 s each, every
other case below 5 ms; test_lines_gpu's test_gather_every_misalignment_of_the_output_and_sizes_around_the_tile took 0.01 s in the same run."""
import numpy as np
import pytest
import torch                              # before the library loads its HIP runtime, as in every GPU test module

from pfac_amd import api  # noqa: E402
from tests import gather_edges as ge  # noqa: E402
from tests import lines_ref as ref  # noqa: E402
from tests.lines_helpers import pattern_file  # noqa: E402
from tests.test_lines_gpu import gpu_handle  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
TRUNCATED = api.STATUS.OUTPUT_TRUNCATED


@pytest.fixture(scope="module")
def handle(workdir):
    h = gpu_handle(pattern_file(workdir, "gather-edges", ref.PATS))
    yield h
    h.destroy()


@pytest.fixture(scope="module")
def cases(handle):
    """family -> name -> case, built for this device"""
    units = int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert units == int(handle.info().multiProcessorCount), "the library and torch see the same device"
    built = ge.families(units)
    for family in ("D", "E"):
        for case in built[family]:
            ge.check_claims(case, units)
    return {family: ge.by_name(members) for family, members in built.items()}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0")


def guarded_gather(h, case, on_device=False):
    """the call of one case -> (status, *h_outBytes).  Asserts everything the module's docstring lists; on_device: the expected text is put
    together from the lines on the device -- every line of the case is the whole input -- and compared there"""
    name, data, start, length, in_offset, out_offset, capacity = case
    n, count = int(data.size), int(start.size)
    total = ge.gather_total(n, start, length)
    cap = total if capacity is None else int(capacity)
    d_in = torch.empty(in_offset + n, dtype=torch.uint8, device="cuda:0")       # no slack: the input's last byte is the tensor's
    d_in[:in_offset] = 0
    d_in[in_offset:] = dev(data)
    d_start, d_len = dev(start), dev(length)
    d_out = torch.full((GUARD + out_offset + cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
    at = GUARD + out_offset
    assert d_in.data_ptr() % 16 == 0 and (d_out.data_ptr() + at) % 16 == out_offset, "the pointers are as far off a 16-byte boundary as the case says"
    st, got = h.gatherLinesFromDevice(d_in.data_ptr() + in_offset, n, d_start.data_ptr(), d_len.data_ptr(), count, d_out.data_ptr() + at, cap, check=False)
    torch.cuda.synchronize()
    assert (st, got) == (TRUNCATED if total > cap else 0, total), f"{name}: status {st}, {got} bytes, want {total}"
    assert bool((d_out[:at] == 0xEE).all()), f"{name}: wrote in front of d_out"
    assert bool((d_out[at + cap:] == 0xEE).all()), f"{name}: wrote at or behind outCapacity"
    if total <= cap:
        if on_device:
            assert bool((d_start == 0).all()) and bool((d_len == n).all())
            want = torch.cat([d_in[in_offset:], torch.full((1,), ge.NL, dtype=torch.uint8, device="cuda:0")]).repeat(count)
            assert torch.equal(d_out[at:at + total], want), f"{name}: gathered text differs"
        else:
            text, want = d_out[at:at + total].cpu().numpy(), ge.gather_text(data, start, length)
            if not np.array_equal(text, want):
                bad = np.flatnonzero(text != want)
                raise AssertionError(f"{name}: {bad.size} bytes differ, first at {bad[0]} (tile {(bad[0] + out_offset) // ge.TILE}, byte "
                                     f"{(bad[0] + out_offset) % ge.TILE}): got {text[bad[0]]} want {want[bad[0]]}")
            assert np.all(d_out[at + total:at + cap].cpu().numpy() == 0xEE), f"{name}: wrote behind the text"
    assert np.array_equal(d_in[in_offset:].cpu().numpy(), data), f"{name}: the input was modified"
    assert np.array_equal(d_start.cpu().numpy(), start) and np.array_equal(d_len.cpu().numpy(), length), f"{name}: the line arrays were modified"
    return st, got


@pytest.mark.parametrize("name", ge.NAMES["A"])
def test_line_starts_around_the_bounds_of_a_tile(handle, cases, name):
    """both binary searches of a tile with a start on, one in front of and one behind oLo and oHi, and on the last thread's first bytes"""
    assert guarded_gather(handle, cases["A"][name]) == (0, ge.A_TOTAL)


@pytest.mark.parametrize("name", ge.NAMES["B"])
def test_tiles_that_stage_4096_offsets_and_one(handle, cases, name):
    """sCount at kOutTile with empty lines only and with a line that is not as the 4096th; cnt == 1: the lo == 0 branch in every thread"""
    assert guarded_gather(handle, cases["B"][name])[0] == 0


@pytest.mark.parametrize("name", ge.NAMES["C"])
def test_line_changes_inside_a_thread(handle, cases, name):
    """next(): sixteen line changes in one thread; a line's newline as byte 15 and as byte 0; the walk that runs off the list"""
    assert guarded_gather(handle, cases["C"][name])[0] == 0


@pytest.mark.parametrize("name", ge.NAMES["D"])
def test_the_cut_of_the_offset_passes(handle, cases, name):
    """lines on both sides of one block, of 8 blocks per compute unit -- per = 256 and 512 -- and of one step of pfac_array_scan"""
    assert guarded_gather(handle, cases["D"][name])[0] == 0


def test_more_tiles_than_one_pass_of_the_grid(handle, cases):
    """32 blocks per compute unit and 128 tiles more: the tile loop's second trip, rel[] rewritten behind the barrier"""
    case = cases["E"][ge.E_NAMES[0]]
    assert guarded_gather(handle, case, on_device=True) == (0, int(case[2].size) << 16)


@pytest.mark.parametrize("name", ge.E_NAMES[1:])
def test_the_size_of_the_text_is_computed_in_64_bits(handle, cases, name):
    assert guarded_gather(handle, cases["E"][name]) == (TRUNCATED, 1 << 32)


@pytest.mark.parametrize("name", ge.NAMES["F"])
def test_lists_in_list_order(handle, cases, name):
    """descending, overlapping, repeated and hostile (start, len): the clamped reference's text, nothing outside d_out[0, outCapacity)"""
    case = cases["F"][name]
    assert guarded_gather(handle, case)[0] == (0 if case[6] is None else TRUNCATED)


@pytest.mark.parametrize("name", ge.NAMES["G"])
def test_the_last_line_ends_with_the_input(handle, cases, name):
    assert guarded_gather(handle, cases["G"][name])[0] == 0


def test_a_small_gather_behind_a_large_one_on_one_handle(workdir, cases):
    """the scratch is grow-only: behind the 8 C 256 + 1 lines of family D (4 MiB of offsets, 4 C + 1 block totals) and the 32.5 MiB of family
    E a case of family A and a list of three lines find stale off[] and blockBase behind their own; trim() between the last two; then each
    once more"""
    h = gpu_handle(pattern_file(workdir, "gather-edges-reuse", ref.PATS))
    try:
        big, mid = cases["E"][ge.E_NAMES[0]], cases["A"]["A-out15-tile1-oLo+0"]
        small = ge.Case("three-lines", mid[1], [7, 0, 300], [5, 0, 40], 3, 9, None)
        base = h.info().deviceScratchBytes
        assert guarded_gather(h, cases["D"]["D-full+1"])[0] == 0
        assert guarded_gather(h, big, on_device=True)[0] == 0
        grown = h.info().deviceScratchBytes
        assert grown > base
        assert guarded_gather(h, mid) == (0, ge.A_TOTAL) and h.info().deviceScratchBytes == grown, "the smaller call keeps the larger scratch"
        h.trim()
        assert h.info().deviceScratchBytes == base
        assert guarded_gather(h, small) == (0, 5 + 0 + 40 + 3)
        for case, on_device in ((big, True), (mid, False), (small, False)):
            assert guarded_gather(h, case, on_device=on_device)[0] == 0
    finally:
        h.destroy()
