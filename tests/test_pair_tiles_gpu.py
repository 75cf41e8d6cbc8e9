"""The mark passes of PFACX_locate* and PFACX_capture* (one first-pair rule, scan_cuts.h: firstPairOfItsTile) on one handle, call after call: each
call's answers for the positions outside the input are its own -- (-1, -1) for locate, (-1, 0) for capture -- and no first-pair word of one call
reaches the next."""
import numpy as np
import pytest
import torch                              # before the library loads its HIP runtime, as in every GPU test module

from pfac_amd import api  # noqa: E402
from tests import capture_ref, locate_ref  # noqa: E402
from tests.test_capture_gpu import capture_device  # noqa: E402
from tests.test_capture_host import capture_host  # noqa: E402
from tests.test_locate_gpu import locate_device, on_device, text_with  # noqa: E402
from tests.test_locate_host import locate_host  # noqa: E402

pytestmark = pytest.mark.gpu

T = api.PFACX_SPLIT_TILE
AT_POS = api.PFACX_CAPTURE_AT_POS


def test_locate_capture_locate_keep_their_own_outside_answers():
    assert torch.cuda.is_available(), "GPU tests need a device; there is no CPU fallback to test"
    torch.cuda.set_device(0)
    n = 2 * T + 1
    data = text_with(n, [5, T - 1, T + 7, 2 * T - 1])
    positions = [-1, 0, T - 1, T, T, 2 * T, n - 1, n, 2 ** 31 - 1]     # tile 1: two equal positions; tile 2: two pairs; three entries outside
    outside = np.array([p < 0 or p >= n for p in positions])
    assert outside.sum() == 3

    want_loc = locate_ref.locate(data, positions, None, 0)
    want_cap = capture_ref.capture(data, None, positions, None, None, None, 0, AT_POS)
    # the references give the outside values of the header, and the host forms agree with them
    assert np.all(want_loc[0][outside] == -1) and np.all(want_loc[1][outside] == -1)
    assert np.all(want_cap[0][outside] == -1) and np.all(want_cap[1][outside] == 0)
    host = api.PFAC.createHostOnly()
    st, rec, col, _ = locate_host(host, data, positions, None, 0)
    assert st == api.STATUS.SUCCESS and np.array_equal(rec, want_loc[0]) and np.array_equal(col, want_loc[1])
    st, start, length = capture_host(host, data, None, positions, None, None, 0, AT_POS)
    assert st == api.STATUS.SUCCESS and np.array_equal(start, want_cap[0]) and np.array_equal(length, want_cap[1])
    host.destroy()

    h = api.PFAC.create()                  # one handle for all three calls; no pattern set: neither call needs one here
    _, view = on_device(data)
    first = locate_device(h, view, n, positions, None, 0)              # every helper checks the guard words around its arrays
    captured = capture_device(h, view, n, None, positions, None, None, 0, AT_POS)
    second = locate_device(h, view, n, positions, None, 0)
    h.destroy()
    for st, rec, col, records in (first, second):
        assert st == api.STATUS.SUCCESS and records == want_loc[2]
        assert np.array_equal(rec, want_loc[0]), (rec, want_loc[0])
        assert np.array_equal(col, want_loc[1]), (col, want_loc[1])
    st, start, length = captured
    assert st == api.STATUS.SUCCESS
    assert np.array_equal(start, want_cap[0]), (start, want_cap[0])
    assert np.array_equal(length, want_cap[1]), (length, want_cap[1])
