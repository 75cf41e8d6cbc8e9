"""The kernels at 100 000 and 300 000 patterns and at match densities between the text's 0.05 % and the hostile 33 % (fixtures:
tests/scale_sets.py; their preconditions: tests/test_scale_host.py).  Every comparison is bit for bit over every position against the
HASHED oracle (the dense table of these sets would be 1.6 GB / 4.9 GB), with poisoned output buffers and canaries around them.

  100 000 patterns   every 2 KiB chunk of the text has more level-1 hits (min 259, median 304) than the filter kernel's hit list has codes
                     (128; 256 in the VETO = 2 instance): several list rounds per chunk with leftover candidates carried between them,
                     several ladder batches per trip -- in every chunk of the launch
  300 000 patterns   47 % of the text's positions pass level 1; a chunk has 886 .. 1024 hits (median 957), right below the 1024 above
                     which it goes to the tiled kernel: the threshold stream puts single chunks on either side
  both               chained table, jump tables, global tail table and bitmaps 3 .. 10 times the size of any the other tests walk
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import allmatch_ref as ref  # noqa: E402
from tests import flows_ref as fr  # noqa: E402
from tests import nocase_ref as nc  # noqa: E402
from tests import scale_sets as ss  # noqa: E402
from tests import stream_ref as sr  # noqa: E402
from tests.gpu_helpers import MODES, STAGE, VETO, assert_same, device_match, make_handle  # noqa: E402
from tests.test_batch_gpu import device_batch, per_segment_oracle, random_cuts  # noqa: E402
from tests.test_flows_gpu import DeviceFeeder  # noqa: E402
from tests.test_flows_host import FLOWS  # noqa: E402
from tests.test_match_all_gpu import check_list, device_all  # noqa: E402
from tests.test_nocase_gpu import caseless_handle  # noqa: E402
from tests.test_stream_gpu import feed_device  # noqa: E402

WINDOW = api.PFACX_WALKER_WINDOW << 8
HASH_BUFFER = MODES[3]
GUARD = 64
# (variant, name, also with misaligned pointers)
FULL_VARIANTS = [(api.PFACX_KERNEL_FILTER | WINDOW, "filter-window", False), (api.PFACX_KERNEL_FILTER | STAGE, "filter-stage", False),
                 (api.PFACX_KERNEL_FILTER | VETO, "filter-veto", True), (api.PFACX_KERNEL_NAIVE, "naive", True),
                 (api.PFACX_KERNEL_AUTO, "auto", True), (api.PFACX_KERNEL_REFTABLE, "reftable", False)]
DENSITY_VARIANTS = [(api.PFACX_KERNEL_FILTER | WINDOW, "filter"), (api.PFACX_KERNEL_FILTER | VETO, "filter-veto"),
                    (api.PFACX_KERNEL_NAIVE, "naive"), (api.PFACX_KERNEL_AUTO, "auto")]


def set_variant(h, variant):
    """the kernel variant and (second byte; none: PFACX_WALKER_AUTO) the walker of a handle whose set is loaded"""
    h.setKernelVariant(variant & 0xFF)
    h.setWalker(variant >> 8)


def device_reduce(h, data, in_offset=0):
    """matchFromDeviceReduce with poisoned arrays of n entries between canaries -> (ids, positions)"""
    n = int(data.size)
    d_in = torch.zeros(n + in_offset + 64, dtype=torch.uint8, device="cuda:0")
    d_in[in_offset:in_offset + n] = torch.from_numpy(np.ascontiguousarray(data)).to("cuda:0")
    d_ids = torch.full((n + 2 * GUARD,), -5, dtype=torch.int32, device="cuda:0")
    d_pos = torch.full((n + 2 * GUARD,), -5, dtype=torch.int32, device="cuda:0")
    _, count = h.matchFromDeviceReduce(d_in.data_ptr() + in_offset, n, d_ids.data_ptr() + 4 * GUARD, d_pos.data_ptr() + 4 * GUARD)
    torch.cuda.synchronize()
    for arr in (d_ids, d_pos):
        assert bool((arr[:GUARD] == -5).all()) and bool((arr[GUARD + n:] == -5).all()), "wrote outside the n entries"
    return d_ids[GUARD:GUARD + count].cpu().numpy(), d_pos[GUARD:GUARD + count].cpu().numpy()


def check_reduce(h, data, want, what, in_offset=0):
    """the pairs are the oracle's non-zero positions, in position order"""
    ids, pos = device_reduce(h, data, in_offset)
    nz = np.flatnonzero(want)
    assert ids.size == nz.size, f"{what}: {ids.size} pairs, want {nz.size}"
    assert_same(pos, nz, f"{what}: positions")
    assert_same(ids, want[nz], f"{what}: ids")


@pytest.fixture(scope="module")
def big_text():
    """{count: (pattern file, text(40 MiB + 1237), oracle result)}, each pair matched once"""
    out = {}
    for count in (ss.S100, ss.S300):
        pf, data = ss.pattern_file(count), ss.text(count, ss.BIG)
        out[count] = (pf, data, ss.want(pf, data))
    return out


@pytest.fixture(scope="module")
def threshold():
    data, hits = ss.threshold_stream()
    pf = ss.pattern_file(ss.S300)
    return pf, data, ss.want(pf, data), hits


# ------------------------------------------------------------------------------------------------------------------ 1. full result

@pytest.mark.parametrize("perf,tex,mode_name", MODES)
@pytest.mark.parametrize("count", [ss.S100, ss.S300])
def test_full_result_of_the_large_sets_in_every_kernel_and_mode(big_text, count, perf, tex, mode_name):
    """PFAC_matchFromDevice over text(40 MiB + 1237) (PFACX_KERNEL_AUTO takes the filter kernel from 32 MiB on): filter-window,
    filter-stage, filter-veto, naive and auto in the four table modes, reftable under PFAC_SPACE_DRIVEN; filter-veto, naive and auto
    again with misaligned pointers (input + 5 bytes, result + 3 ints).  One handle per set and mode, its variant and walker switched.
    The ONE combination left out is reftable under PFAC_TIME_DRIVEN: it would upload the dense table of 1.6 GB / 4.9 GB."""
    pf, data, want = big_text[count]
    h = make_handle(pf, perf, tex, FULL_VARIANTS[0][0])
    try:
        info = h.info()
        assert info.numOfPatterns == count and info.filterTailGlobalEntries > 0 and info.filterTailEntries == 0
        for variant, vname, misaligned in FULL_VARIANTS:
            if vname == "reftable" and perf != api.PFAC_SPACE_DRIVEN:
                continue
            set_variant(h, variant)
            what = f"{count} patterns / {mode_name} / {vname}"
            assert_same(device_match(h, data), want, what + " / aligned")
            if vname == "filter-veto":
                st = h.scanStats(data.size)
                assert st["veto"] == 2 and st["walksStarted"] > 0, st
                print(f"\n[{what}] level-1 pass {st['level1Hits'] / data.size:.3f}, walked {st['walksStarted'] / data.size:.4f}, dense chunks {st['denseChunks']}")
            if misaligned:
                assert_same(device_match(h, data, in_offset=5, out_offset=3), want, what + " / input +5 B, result +3 ints")
    finally:
        h.destroy()


# ------------------------------------------------------------------------------------------------------- 2. AUTO, call after call

def test_auto_over_consecutive_calls_on_one_handle(big_text):
    """S300 lets 47 % of the text through level 1: the vote a big launch leaves for the handle's next one (PFACX_info_t::streamDense)
    may go either way.  Three 40 MiB calls and a 20 MiB call (below 32 MiB: the tiled kernel) on one handle give the oracle's vector
    whichever kernel runs; which one did is printed."""
    pf, data, want = big_text[ss.S300]
    h = make_handle(pf, api.PFAC_SPACE_DRIVEN, api.PFAC_TEXTURE_ON, api.PFACX_KERNEL_AUTO)
    h.setWalker(api.PFACX_WALKER_AUTO)
    try:
        ran = []
        for call in range(3):
            ran.append("tiled" if h.info().streamDense else "filter")
            assert_same(device_match(h, data), want, f"auto / call {call} ({ran[-1]})")
        print(f"\n[auto, S300, 3 x 40 MiB] ran: {ran}, dense chunks of the last filter launch: {h.scanStats()['denseChunks']}")
        m = 20 << 20
        assert_same(device_match(h, data[:m + 2500])[:m], want[:m], "auto / 20 MiB")
    finally:
        h.destroy()


# ---------------------------------------------------------------------------------------------------------- 3. the dense threshold

@pytest.mark.parametrize("variant,vname", [(api.PFACX_KERNEL_FILTER | WINDOW, "filter-window"), (api.PFACX_KERNEL_FILTER | VETO, "filter-veto"),
                                           (api.PFACX_KERNEL_AUTO, "auto")])
def test_chunks_on_either_side_of_the_dense_threshold(threshold, variant, vname):
    """Single chunks of one launch go to the listed path (<= 1024 level-1 hits) and to the dense list for the tiled kernel (> 1024), in
    thousands of alternations, with chunks at 1023 .. 1025 among them.
    denseChunks EQUALS the model's count: the launch cuts its chunks from the first 16-byte aligned input byte (scan_module.hip:
    headPositions) -- byte 0 of a torch allocation -- so chunk k is [2048 k, 2048 k + 2048), the model's; a fresh chunk's `total` in
    scan_filter.hip is the popcount of all its level-1 bits, the model's count; and the chunks the launch does NOT take -- the last
    maxPatternLen + 192 bytes and the odd rest behind the last whole chunk are walked with bounds (scan_module.hip: filterLength) -- lie
    in the stream's last 16 KiB, where no chunk exceeds the threshold (scale_sets.check_threshold).  With misaligned pointers the grid
    moves by the misalignment and only the result is compared."""
    pf, data, want, hits = threshold
    chunks = data.size // ss.CHUNK
    h = make_handle(pf, api.PFAC_SPACE_DRIVEN, api.PFAC_TEXTURE_ON, variant)
    if not variant >> 8:
        h.setWalker(api.PFACX_WALKER_AUTO)
    try:
        assert_same(device_match(h, data), want, f"threshold stream / {vname}")
        st = h.scanStats(data.size)
        model = int(np.count_nonzero(hits > ss.DENSE_HITS))
        print(f"\n[threshold stream / {vname}] dense chunks {st['denseChunks']} of {chunks} (model {model}), walks {st['walksStarted']}")
        assert 0 < st["denseChunks"] < chunks
        assert st["denseChunks"] == model
        assert_same(device_match(h, data, in_offset=5, out_offset=3), want, f"threshold stream / {vname} / input +5 B, result +3 ints")
    finally:
        h.destroy()


# ------------------------------------------------------------------------------------------------- 4. compacted output, all-match

@pytest.mark.parametrize("variant,vname", [(api.PFACX_KERNEL_FILTER, "filter"), (api.PFACX_KERNEL_NAIVE, "naive")])
@pytest.mark.parametrize("which", ["s100-text", "s300-threshold"])
def test_compacted_output_and_all_match_at_scale(big_text, threshold, which, variant, vname):
    """PFAC_matchFromDeviceReduce (the filter variant: its own one-bit level 1) and PFACX_matchAllFromDevice (the expansion over the
    prefix table of 100 000 / 300 000 patterns) against the oracle's non-zero positions and tests/allmatch_ref.py"""
    count, (pf, data, want) = (ss.S100, big_text[ss.S100]) if which == "s100-text" else (ss.S300, threshold[:3])
    h = make_handle(pf, *HASH_BUFFER[:2], variant)
    try:
        check_reduce(h, data, want, f"{which} / {vname} / reduce")
        check_reduce(h, data, want, f"{which} / {vname} / reduce, input +3 B", in_offset=3)
        want_pos, want_ids = ref.expand_longest(ss.patterns(count), want)
        assert want_pos.size > np.count_nonzero(want)               # some positions hold more than one pattern
        st, n, pos, ids = device_all(h, data, capacity=max(data.size, want_pos.size))        # (the call wants capacity >= size)
        assert st == api.STATUS.SUCCESS and n == want_pos.size, (st, n, want_pos.size)
        check_list(pos, ids, want_pos, want_ids, f"{which} / {vname} / all-match")
    finally:
        h.destroy()


# --------------------------------------------------------------------------------------------------------- 5. batch, stream, flows

class _HashedSegments:
    """per_segment_oracle asks `o.match(segment, omp=...)`: the hashed oracle of the set"""

    def __init__(self, pf):
        self.pf = pf

    def match(self, data, omp=False):
        return ss._oracle(self.pf).match(data, hashed=True, omp=omp)


@pytest.mark.parametrize("variant,vname", [(api.PFACX_KERNEL_FILTER, "filter"), (api.PFACX_KERNEL_AUTO, "auto")])
def test_batch_of_segments_on_the_100k_set(big_text, variant, vname):
    """PFACX_matchBatchFromDevice: segments of 1.5 KiB, of 64 bytes and ragged ones (0 .. 4096 bytes), each against the oracle on that
    segment alone"""
    pf, data, _ = big_text[ss.S100]
    o = _HashedSegments(pf)
    h = make_handle(pf, *HASH_BUFFER[:2], variant)
    try:
        for shape, part, offs in (("1.5 KiB", data[:4 << 20], np.append(np.arange(0, 4 << 20, 1536), 4 << 20).astype(np.uint64)),
                                  ("64 B", data[5 << 20:7 << 20], np.arange(0, (2 << 20) + 1, 64, dtype=np.uint64)),
                                  ("ragged", data[ss.BIG - (4 << 20) - 1237:], random_cuts((4 << 20) + 1237, 4096, seed=100))):
            want = per_segment_oracle(o, part, offs)
            assert np.count_nonzero(want) > 100
            assert_same(device_batch(h, part, offs), want, f"batch / {vname} / {shape}")
        assert_same(device_batch(h, part, offs, in_offset=3, out_offset=1), want, f"batch / {vname} / ragged, misaligned")
    finally:
        h.destroy()


def test_stream_and_flows_on_the_100k_set(big_text):
    """one stream model (tests/stream_ref.py) and one flows schedule (tests/flows_ref.py, its check_coverage on) through the device
    calls: the seams of pieces cut inside occurrences, with the large tables behind them"""
    pf, data, want = big_text[ss.S100]
    part = data[ss.BIG - (3 << 20):]                             # (the planted end of the text included)
    full = want[ss.BIG - (3 << 20):]
    pos = np.flatnonzero(full > 0).astype(np.int64)
    ids = full[pos].astype(np.int32)
    lengths = sr.pattern_lengths(pf)
    M = int(lengths.max())
    sizes = sr.make_sizes(part.size, M, pos, ids, lengths, seed=100)
    assert sr.straddling(pos, ids, lengths, sizes) >= 20
    calls, flush = sr.split(pos, ids, sizes, M)
    with ss.hashed_oracle():
        m = fr.build(pf, part, FLOWS, 100)
    h = make_handle(pf, *HASH_BUFFER[:2], api.PFACX_KERNEL_AUTO)
    try:
        feed_device(h, part, sizes, calls, flush, "S100 stream")
        DeviceFeeder(h, m, "S100 flows").run()
    finally:
        h.destroy()


# ----------------------------------------------------------------------------------------------------------------- 6. caseless set

@pytest.fixture(scope="module")
def caseless():
    """(pattern file as written: random letter case, file with every pattern folded, input with random letter case, oracle result of the
    folded set over the folded input): S100 without the patterns whose fold another pattern has already (the oracle, like the
    reference, takes no duplicate lines)"""
    rng = np.random.Generator(np.random.PCG64(100))
    seen, folded = set(), []
    for p in ss.patterns(ss.S100):
        f = nc.fold(p)
        if f not in seen:
            seen.add(f)
            folded.append(f)
    assert len(folded) > 99_000
    raw = nc.flip_array(np.frombuffer(nc.pattern_bytes(folded), dtype=np.uint8), rng).tobytes()        # ('\n' is no letter)
    assert raw != nc.pattern_bytes(folded) and nc.fold(raw) == nc.pattern_bytes(folded)
    pf, ff = ss.scratch_path("s100_nocase.pat"), ss.scratch_path("s100_folded.pat")
    open(pf, "wb").write(raw)
    open(ff, "wb").write(nc.pattern_bytes(folded))
    data = nc.flip_array(ss.text(ss.S100, ss.BIG), rng)
    want = ss.want(ff, nc.fold_array(data))
    assert np.count_nonzero(want) > 400
    return pf, ff, data, want


@pytest.mark.parametrize("variant,vname", [(api.PFACX_KERNEL_FILTER, "filter"), (api.PFACX_KERNEL_NAIVE, "naive"), (api.PFACX_KERNEL_AUTO, "auto")])
def test_caseless_100k_set(caseless, variant, vname):
    """PFACX_READ_NOCASE: full result and compacted output equal the oracle of the folded set over the folded input"""
    pf, _, data, want = caseless
    h = caseless_handle(pf, *HASH_BUFFER[:2], variant)
    try:
        assert h.caseInsensitive() == 1
        assert_same(device_match(h, data), want, f"caseless / {vname}")
        assert_same(device_match(h, data, in_offset=5, out_offset=3), want, f"caseless / {vname} / misaligned")
        check_reduce(h, data, want, f"caseless / {vname} / reduce")
    finally:
        h.destroy()


# ----------------------------------------------------------------------------------------------------------------- 7. compiled set

def test_compiled_large_set_loaded_on_the_gpu(big_text, tmp_path):
    """S300 saved by a host-only handle, loaded by a GPU handle: 8 MiB under PFACX_KERNEL_AUTO (the tiled kernel), and the 40 MiB text (the
    filter kernel over the loaded filter tables)"""
    pf, data, want = big_text[ss.S300]
    path = str(tmp_path / "s300.pfacx")
    ss.host_handle(ss.S300).saveCompiled(path)
    h = api.PFAC.create()
    try:
        h.setKernelVariant(api.PFACX_KERNEL_AUTO)
        h.loadCompiled(path)
        assert h.info().numOfPatterns == ss.S300
        small = ss.text(ss.S300, 8 << 20)
        assert_same(device_match(h, small), ss.want(pf, small), "loaded S300 / auto / 8 MiB")
        assert_same(device_match(h, data), want, "loaded S300 / auto / 40 MiB")
    finally:
        h.destroy()


# ------------------------------------------------------------------------------------------------------------------ 8. density axis

def density_cases():
    return [(f"density-{t}", t) for t in ss.DENSITIES] + [(f"one-byte-{k}", k) for k in (1, 2, 4, 8)]


@pytest.mark.parametrize("name,arg", density_cases())
def test_match_densities_between_text_and_hostile(name, arg):
    """C3's 30 000 patterns at 0.5 %, 2 % and 10 % of positions matching (whole patterns planted), and with 1, 2, 4, 8 one-byte patterns over the
    plain text (3 % .. 13 %): every match is a 4-byte patch store ordered against the writer waves' zero stream.  40 MiB + 1237 under
    filter, filter-veto, naive and auto: the full vector and the compacted output."""
    if name.startswith("density"):
        data, want, density = ss.density_stream(arg)
        pf = ss.pattern_file(ss.C3)
    else:
        pf, data, want = ss.one_byte_set(arg)
        density = np.count_nonzero(want) / data.size
    h = make_handle(pf, *HASH_BUFFER[:2], DENSITY_VARIANTS[0][0])
    try:
        for variant, vname in DENSITY_VARIANTS:
            set_variant(h, variant)
            assert_same(device_match(h, data), want, f"{name} / {vname}")
            st = h.scanStats(data.size)
            print(f"\n[{name} / {vname}] density {density:.4f}, denseChunks {st['denseChunks']}, walksStarted {st['walksStarted']} (of the handle's last filter launch)")
            check_reduce(h, data, want, f"{name} / {vname} / reduce")
    finally:
        h.destroy()
