"""The flows seam and merge kernels (pfac_amd/csrc/scan_flows.hip, seamBlock of scan_passes.h) at their piece, block and M edges, and
pfac_stream_seam (scan_stream.hip) at the same M edges: the cases of tests/flows_edges.py through PFACX_flowsMatchFromDevice and
PFACX_flowsFlush, call by call against the model, with the canaries and the unmodified-input check of tests/test_flows_gpu.py: DeviceFeeder.
tests/test_flows_edges_host.py proves that each case reaches the code its name says."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import flows_edges as fe  # noqa: E402
from tests import flows_ref as fr  # noqa: E402
from tests.test_flows_gpu import DeviceFeeder  # noqa: E402


@pytest.fixture(scope="module")
def handle_of():
    """case -> the handle of its pattern set (readPatternFromMemoryEx), one per set for the whole module"""
    handles = {}

    def get(case):
        key = (case.M, case.nocase)
        if key not in handles:
            h = api.PFAC.create()
            h.readPatternFromMemoryEx(case.patterns, api.PFACX_READ_NOCASE if case.nocase else 0)
            assert h.info().maxPatternLen == case.M
            handles[key] = h
        return handles[key]

    yield get
    for h in handles.values():
        h.destroy()


def feed(h, case, what=None, misalign=0, m=None):
    DeviceFeeder(h, m or fe.model(case), what or f"{case.name} device", misalign).run()


# ------------------------------------------------------------------------------------------------------------- A: piece-count edges

@pytest.mark.parametrize("P", fe.A_COUNTS)
def test_piece_counts_at_the_wave_block_and_trip_edges(handle_of, P):
    case = fe.piece_counts(P)
    feed(handle_of(case), case)


@pytest.mark.parametrize("P", [fe.PIECE_BLOCK + 1, fe.SUMS_TRIP + 1])
def test_piece_counts_from_a_misaligned_buffer(handle_of, P):
    case = fe.piece_counts(P)
    feed(handle_of(case), case, f"{case.name} device + 5", misalign=5)


def test_a_small_call_behind_a_large_one_on_the_same_handle(handle_of):
    """513 pieces right behind 65 537: the large call's scratch -- counts, block sums, seam lists -- is still there"""
    large, small = fe.piece_counts(fe.SUMS_TRIP + 1), fe.piece_counts(2 * fe.PIECE_BLOCK + 1)
    h = handle_of(large)
    scratch = h.info().deviceScratchBytes
    feed(h, large)
    assert h.info().deviceScratchBytes >= max(scratch, 12 * large.F)
    feed(h, small, f"{small.name} device behind {large.name}")


# --------------------------------------------------------------------------------------------- B: pairs relative to a block of pieces

@pytest.mark.parametrize("which", fe.B_WHICH)
def test_pairs_relative_to_a_block_of_pieces(handle_of, which):
    case = fe.block_positions(which)
    feed(handle_of(case), case)


def test_one_flow_set_twice_with_a_reset_between(handle_of):
    """every position a pair: the batches, a reset of all flows with every carry full, and the same schedule on the same set"""
    case = fe.block_positions("all-a")
    m = fe.twice_with_a_reset(case)
    assert [type(s) for s in m.steps].count(fr.End) == 2 and m.steps[2].kind == "reset"
    feed(handle_of(case), case, f"{case.name} device, twice with a reset", m=m)


# ---------------------------------------------------------------------------------------------------------------- C: seam shapes by M

C_CASES = [(s, False) for s in fe.C_SPANS] + [(s, True) for s in fe.C_NOCASE_SPANS]
C_IDS = [f"{s}{'-nocase' if n else ''}" for s, n in C_CASES]


@pytest.mark.parametrize("span,nocase", C_CASES, ids=C_IDS)
def test_seam_shapes_by_m(handle_of, span, nocase):
    case = fe.seam_shapes(span, nocase)
    feed(handle_of(case), case, misalign=3 if nocase else 0)


@pytest.mark.parametrize("span,nocase", C_CASES, ids=C_IDS)
def test_seam_shapes_by_m_piece_by_piece_through_the_stream_calls(handle_of, span, nocase):
    """pfac_stream_seam on the same M edges: every flow a stream of the same handle, fed the flow's pieces with PFACX_streamMatchFromDevice
    and ended with PFACX_streamFlush, every call against the model's slice of its batch"""
    case = fe.seam_shapes(span, nocase)
    h = handle_of(case)
    streams = [h.streamOpen() for _ in range(case.F)]
    try:
        cap = max(int(fe.piece_lengths(s).max()) for s in case.steps if isinstance(s, fr.Batch)) + case.M
        s_ids = torch.full((cap + 1,), -7, dtype=torch.int32, device="cuda:0")
        s_pos = torch.full((cap + 1,), -7, dtype=torch.int32, device="cuda:0")
        for k, step in enumerate(case.steps):
            if isinstance(step, fr.Batch):
                d_in = torch.from_numpy(step.buf).to("cuda:0")
            for j, f in enumerate(step.flows.tolist()):
                lo, hi = int(step.first[j]), int(step.first[j + 1])
                where = f"{case.name}: step {k}, flow {f}"
                if isinstance(step, fr.Batch):
                    a, b = int(step.offsets[j]), int(step.offsets[j + 1])
                    _, n, off = streams[f].match_device(d_in.data_ptr() + a, b - a, s_ids.data_ptr(), s_pos.data_ptr(), cap)
                    assert off == int(step.offs[j]), f"{where}: piece offset {off}"
                else:
                    _, n = streams[f].flush(s_ids.data_ptr(), s_pos.data_ptr(), cap)
                assert n == hi - lo, f"{where}: {n} pairs, want {hi - lo}"
                assert np.array_equal(s_pos[:n].cpu().numpy(), step.pos[lo:hi]), f"{where}: positions differ"
                assert np.array_equal(s_ids[:n].cpu().numpy(), step.ids[lo:hi]), f"{where}: ids differ"
        assert int(s_ids[cap]) == -7 and int(s_pos[cap]) == -7
    finally:
        for s in streams:
            s.close()


# -------------------------------------------------------------------------------------------------------------------- D: dense seams

@pytest.mark.parametrize("behind", [b"a", b"z"], ids=["a", "z"])
@pytest.mark.parametrize("span", fe.D_SPANS)
def test_dense_seams(handle_of, span, behind):
    case = fe.dense_seams(span, behind)
    feed(handle_of(case), case)
