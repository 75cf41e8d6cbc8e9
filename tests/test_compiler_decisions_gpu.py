"""Every decision of the pattern compiler on both sides of its threshold, on the device: the sets of tests/compiler_sets.py (each asserts which
side it is on) through the kernels that read the decided structures -- the filter kernel under its three walkers, the tiled kernel, the
compacted output -- against the oracle, exact equality of the whole result vector; the form of the veto a set was built to get; the dense
fast table (pfac_api.cpp: uploadChainedHashTable) around both of its thresholds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import compiler_sets as cs  # noqa: E402
from tests.gpu_helpers import MODES, assert_same, device_match, make_handle  # noqa: E402

WINDOW, STAGE, VETO = (api.PFACX_WALKER_WINDOW, "window"), (api.PFACX_WALKER_STAGE, "stage"), (api.PFACX_WALKER_VETO, "veto")


def _modes(name):
    """sets of up to 5000 patterns in all four table modes; the dense tables of the larger ones are hundreds of MB: the two hashed modes"""
    return MODES if cs.get(name).small else MODES[2:]


def _reduce(h, data, want, what):
    n = int(data.size)
    d_in = torch.from_numpy(np.array(data)).to("cuda:0")
    d_ids = torch.full((n,), -3, dtype=torch.int32, device="cuda:0")
    d_pos = torch.full((n,), -3, dtype=torch.int32, device="cuda:0")
    _, count = h.matchFromDeviceReduce(d_in.data_ptr(), n, d_ids.data_ptr(), d_pos.data_ptr())
    nz = np.flatnonzero(want)
    assert count == nz.size, (what, count, nz.size)
    assert np.array_equal(d_pos[:count].cpu().numpy(), nz) and np.array_equal(d_ids[:count].cpu().numpy(), want[nz]), what


@pytest.mark.parametrize("name", cs.NAMES)
def test_every_kernel_that_reads_the_decided_structures_equals_oracle(name):
    sset = cs.get(name)
    data, want = cs.stream(name)
    n = data.size
    cut = data[:n - 2]                                  # the last pattern is cut off by the end of the input
    want_cut = cs.oracle_match(name, cut)
    assert not np.array_equal(want_cut, want[:n - 2])
    for perf, tex, mode_name in _modes(name):
        h = make_handle(sset.pattern_file, perf, tex, api.PFACX_KERNEL_FILTER)
        try:
            walks = {}
            for walker, walker_name in (WINDOW, STAGE, VETO):
                h.setWalker(walker)
                what = f"{name}/{mode_name}/filter-{walker_name}"
                assert_same(device_match(h, data), want, what)
                st = h.scanStats()
                walks[walker_name] = st["walksStarted"]
                if walker == api.PFACX_WALKER_VETO:
                    assert st["veto"] == sset.veto, (what, st["veto"], sset.veto)
                    assert_same(device_match(h, data, in_offset=5, out_offset=3), want, what + "/input +5 B, result +3 ints")
                    assert_same(device_match(h, cut), want_cut, what + "/cut off by the end")
                else:                                   # a table in LDS is asked by every launch but the stage walker's (scan_filter.hip: launchChained)
                    assert st["veto"] == (1 if sset.veto == 1 and walker == api.PFACX_WALKER_WINDOW else 0), (what, st["veto"])
                _reduce(h, data, want, what + "/compacted")
            print(f"{name}/{mode_name}: walks started window {walks['window']} stage {walks['stage']} veto {walks['veto']}")
            if sset.spares_walks:                       # near misses stop at a node that knows the rest of its pattern: the veto spares their walks
                plain = walks["stage"] if sset.veto == 1 else walks["window"]       # the launch that asks no table
                assert walks["veto"] < plain, (name, mode_name, walks)
            assert walks["veto"] <= walks["window"] <= walks["stage"], (name, mode_name, walks)      # (compiler_sets says which sets leave it at that, and why)
            h.setKernelVariant(api.PFACX_KERNEL_NAIVE)
            assert_same(device_match(h, data), want, f"{name}/{mode_name}/tiled")
            _reduce(h, data, want, f"{name}/{mode_name}/tiled/compacted")
        finally:
            h.destroy()


@pytest.mark.parametrize("name", cs.FAST_NAMES)
def test_dense_fast_table_on_both_sides_of_its_thresholds(name):
    """The table exists for a set of at most 8192 states of which less than a quarter lie inside chains, in both perf modes, and for neither
    neighbour.  Witness: PFACX_getInfo's deviceTableBytes.  int[S][256] is numOfStates KiB; everything else such a set keeps on the device --
    the chained tables (32 bytes a slot, a few slots a state), the hashed pair, 200 KiB of bitmaps and counters -- is a fraction of that, so
    the bytes lie above numOfStates x 1024 with the table and below without.  Then 33 MiB of a pattern-dense stream under PFACX_KERNEL_AUTO,
    twice: the second call takes the density route (through the dense table where it exists) -- both equal the oracle."""
    sset = cs.get(name)
    fast = sset.extra["fast"]
    data, want = cs.dense_stream(name)
    for perf, tex, mode_name in (MODES[1], MODES[2]):
        h = make_handle(sset.pattern_file, perf, tex, api.PFACX_KERNEL_AUTO)
        try:
            info = h.info()
            print(f"{name}/{mode_name}: numOfStates {info.numOfStates} deviceTableBytes {info.deviceTableBytes}")
            assert info.numOfStates == sset.extra["states"]
            assert (info.deviceTableBytes >= info.numOfStates * 1024) == fast, (name, info.deviceTableBytes, info.numOfStates)
            assert_same(device_match(h, data), want, f"{name}/{mode_name}/auto, first call")
            assert h.info().streamDense == 1, "the stream is not pattern-dense: the second call would not take the density route"
            assert_same(device_match(h, data), want, f"{name}/{mode_name}/auto, second call")
            assert_same(device_match(h, data, in_offset=16, out_offset=4), want, f"{name}/{mode_name}/auto, third call, other addresses")
        finally:
            h.destroy()
