"""PFACX_locatePairsFromDevice and PFACX_capturePairsFromDevice (scan_locate.hip, scan_capture.hip, scan_cuts.h) where a block of the pairs kernels
takes a second tile, a thread of the mark kernels a second pair, pfac_locate_carry a third step, a block counts slow pairs in several tiles, and
at n = 2^31 - 1: the cases of tests/cuts_edges.py, built for the grid of the device at hand (8 blocks per compute unit), every answer compared entry
for entry with the model there, the slow count read from the module entry PFACX_captureRun.  tests/test_cuts_edges_host.py checks the model
against the byte-by-byte references and the cases' claims for 256 compute units; the claims are asserted again here, for this device.  Every
call: guard words on both sides of both output arrays, guard bytes around the input, the input and the list unmodified, the pointer at 0 and at
5 mod 16; behind every large case a small call on the same handle."""
import time

import numpy as np
import pytest
import torch                              # before the library loads its HIP runtime, as in every GPU test module

from pfac_amd import api  # noqa: E402
from tests import cuts_edges as ce  # noqa: E402

pytestmark = pytest.mark.gpu

T = ce.T
GUARD = -0x5A5A5A5B                       # no record, no column, no start, no length, not -1
PAD = 4                                   # guard words on each side of an output array
EDGE = 32                                 # bytes in front of and behind the input
FILL = 0x0A
MISALIGNMENTS = (0, 5)
DEV = "cuda:0"


@pytest.fixture(scope="module")
def handle():
    assert torch.cuda.is_available(), "GPU tests need a device; there is no CPU fallback to test"
    torch.cuda.set_device(0)
    h = api.PFAC.create()
    h.readPatternFromMemory(ce.PATTERNS)
    yield h
    h.destroy()


@pytest.fixture(scope="module")
def grid(handle):
    return api.PFACX_GRID_BLOCKS_PER_CU * int(handle.info().multiProcessorCount)


def guarded(n):
    return torch.full((n + 2 * PAD,), GUARD, dtype=torch.int32, device=DEV)


def inner(buf, n):
    got = buf.cpu().numpy()
    assert np.all(got[:PAD] == GUARD) and np.all(got[PAD + n:] == GUARD), "written outside an array"
    return got[PAD:PAD + n].copy()


def same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def a_small_call(h):
    """what a plain call answers on this handle, behind a large one"""
    text = np.frombuffer(b"k= v;key:w;\nab\n\nxyz", dtype=np.uint8)
    d_in = torch.from_numpy(text.copy()).to(DEV)
    d_pos = torch.tensor([0, 5, 12, 15, 16, 18], dtype=torch.int32, device=DEV)
    d_ids = torch.tensor([1, 2, 1, 1, 1, 1], dtype=torch.int32, device=DEV)
    rec, col, start, length = guarded(6), guarded(6), guarded(6), guarded(6)
    st, records = h.locatePairsFromDevice(d_in.data_ptr(), text.size, None, 0, d_pos.data_ptr(), 6, rec.data_ptr() + 4 * PAD, col.data_ptr() + 4 * PAD)
    assert (st, records) == (0, 4) and inner(rec, 6).tolist() == [0, 0, 1, 2, 3, 3] and inner(col, 6).tolist() == [0, 5, 0, 0, 0, 2]
    st = h.capturePairsFromDevice(d_in.data_ptr(), text.size, b" ", b";", 0, 0, d_ids.data_ptr(), d_pos.data_ptr(), 2, start.data_ptr() + 4 * PAD,
                                  length.data_ptr() + 4 * PAD)
    got = inner(start, 6), inner(length, 6)
    assert st == 0 and got[0].tolist() == [3, 9] + [GUARD] * 4 and got[1].tolist() == [1, 1] + [GUARD] * 4


def run(h, case, view, mis):
    """every call of the case over the input at `view`; the list checked behind them"""
    k = case.pos.size
    d_pos = torch.from_numpy(case.pos.copy()).to(DEV)
    d_ids = None if case.ids is None else torch.from_numpy(case.ids.copy()).to(DEV)
    d_lens = torch.from_numpy(ce.LENS.copy()).to(DEV)
    assert view.data_ptr() % 16 == mis
    for cls, flags in case.locate:
        what = (case.name, "locate", cls, flags, mis)
        rec, col = guarded(k), guarded(k)
        st, records = h.locatePairsFromDevice(view.data_ptr(), case.n, cls, flags, d_pos.data_ptr(), k, rec.data_ptr() + 4 * PAD,
                                              col.data_ptr() + 4 * PAD, check=False)
        torch.cuda.synchronize()
        want = case.want_locate(cls, flags)
        assert (st, records) == (api.STATUS.SUCCESS, want[2]), what
        same(inner(rec, k), want[0], what + ("record",))
        same(inner(col, k), want[1], what + ("column",))
    for skip, stop, window, flags in case.capture:
        what = (case.name, "capture", skip, stop, window, flags, mis)
        ids = None if flags & ce.AT_POS else d_ids.data_ptr()
        want = case.want_capture(skip, stop, window, flags)
        start, length = guarded(k), guarded(k)
        st = h.capturePairsFromDevice(view.data_ptr(), case.n, skip, stop, window, flags, ids, d_pos.data_ptr(), k, start.data_ptr() + 4 * PAD,
                                      length.data_ptr() + 4 * PAD, check=False)
        torch.cuda.synchronize()
        assert st == api.STATUS.SUCCESS, what
        same(inner(start, k), want[0], what + ("valStart",))
        same(inner(length, k), want[1], what + ("valLen",))
        start, length = guarded(k), guarded(k)
        st, slow = ce.capture_run(h, view.data_ptr(), case.n, skip, stop, window, flags, ids, d_pos.data_ptr(), k, d_lens.data_ptr(), ce.LENS.size,
                                  start.data_ptr() + 4 * PAD, length.data_ptr() + 4 * PAD)
        torch.cuda.synchronize()
        print("%s: %d slow pairs, the model %d" % (what, slow, int(np.count_nonzero(want[2]))))
        assert st == api.STATUS.SUCCESS, what
        same(inner(start, k), want[0], what + ("valStart of the module entry",))
        same(inner(length, k), want[1], what + ("valLen of the module entry",))
        assert slow == int(np.count_nonzero(want[2])), what + ("the slow pairs",)
    assert np.array_equal(d_pos.cpu().numpy(), case.pos) and (d_ids is None or np.array_equal(d_ids.cpu().numpy(), case.ids)), "the list is never written"


def check(h, case):
    """a case of families A to D: its claims on this device's grid, then every call at both alignments"""
    ce.check_claims(case)
    data = case.text.dense()
    for mis in MISALIGNMENTS:
        t0 = time.perf_counter()
        whole = torch.full((EDGE + 16 + data.size + EDGE,), FILL, dtype=torch.uint8, device=DEV)
        view = whole[EDGE + mis:EDGE + mis + data.size]
        view.copy_(torch.from_numpy(data))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        run(h, case, view, mis)
        print("%s + %d: the input up in %.2f s, %d calls and their checks in %.2f s" % (case.name, mis, t1 - t0, len(case.locate) + 2 * len(case.capture),
                                                                                   time.perf_counter() - t1))
        back = whole.cpu().numpy()
        lo = EDGE + mis
        assert np.array_equal(back[lo:lo + data.size], data) and np.all(back[:lo] == FILL) and np.all(back[lo + data.size:] == FILL), "the input is never written"
        del whole, view
        a_small_call(h)


@pytest.mark.parametrize("variant", sorted(ce.A_VARIANTS))
def test_tiles_beyond_one_pass_of_the_grid(handle, grid, variant):
    """the second trip of pfac_locate_pairs, pfac_capture_pairs and pfac_split_count<., false>, SINGLE and through the table: tiles with pairs in
    both trips, in one, full of delimiters and without any, and the last tile's 5 bytes over a tile that set every bit"""
    check(handle, ce.tiles_beyond_a_pass(grid, variant))


@pytest.mark.parametrize("kind", ce.B_KINDS)
def test_lists_beyond_one_pass_of_the_mark_kernels(handle, grid, kind):
    """the second trip of pfac_locate_mark and pfac_capture_mark: positions outside the input, ids the set does not have and a tile's first pair
    at indices of the second pass; once over family A's tiles"""
    check(handle, ce.lists_beyond_a_pass(grid, kind))


@pytest.mark.parametrize("kind", ce.C_KINDS)
def test_three_steps_of_the_carry(handle, grid, kind):
    """pfac_locate_carry: the last cut survives two step edges, sits on one, opens a step, and never falls back over a step without a cut"""
    check(handle, ce.carry_steps(grid, kind))


@pytest.mark.parametrize("window", ce.D_WINDOWS)
def test_slow_pairs_in_several_tiles_of_a_block(handle, grid, window):
    """slowHere over a block's trips: the values and the exact count, without a window and with one that turns most of them fast"""
    case = ce.slow_pairs(grid, window)
    assert int(np.count_nonzero(case.want_capture(*case.capture[0])[2])) > (0 if window else 12)
    check(handle, case)


@pytest.mark.parametrize("kind", ce.E_KINDS)
def test_the_top_of_the_32_bit_range(handle, kind):
    """n = 2^31 - 1, zeros and a few special bytes written on the device; the model never sees more than those bytes"""
    case = ce.top_of_range(kind)
    ce.check_claims(case)
    n = case.n
    if torch.cuda.mem_get_info()[0] < 3 << 30:
        pytest.skip("needs 3 GiB of free device memory")
    at, by = case.text.sparse()
    assert np.all(by != 0)
    whole = torch.zeros(EDGE + 16 + n + EDGE, dtype=torch.uint8, device=DEV)
    d_at, d_by = torch.from_numpy(at).to(DEV), torch.from_numpy(by).to(DEV)
    for mis in MISALIGNMENTS:
        whole.zero_()
        lo = EDGE + mis
        whole[:lo] = FILL
        whole[lo + n:] = FILL
        view = whole[lo:lo + n]
        view[d_at] = d_by
        run(handle, case, view, mis)
        assert int(torch.count_nonzero(whole)) == at.size + whole.numel() - n and torch.equal(view[d_at], d_by), "the input is never written"
        assert bool(torch.all(whole[:lo] == FILL)) and bool(torch.all(whole[lo + n:] == FILL))
        a_small_call(handle)
    del whole, view
    torch.cuda.empty_cache()
