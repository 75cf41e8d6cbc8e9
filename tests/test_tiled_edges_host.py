"""The fixtures of tests/test_tiled_edges_gpu.py (tests/tiled_edges.py), checked without a device: the model of the tiled kernel's
early-out, the survivor counts that put a group on either side of the kernel's thresholds -- the kernel does not report which
branch a group took, so these counts are the evidence that the GPU test reaches each --, and that the oracle finds what was planted."""
import numpy as np
import pytest

from tests import tiled_edges as te
from tests.filter_model import level1_model, prefilter_model


def test_pattern_set_is_the_one_the_cases_need():
    pats = te.PATTERNS
    lens = sorted(len(p) for p in pats)
    assert pats[0] == b"q" and pats[1] == b"zz" and lens[-4:] == [60, 60, 200, 600] and len(set(pats)) == len(pats)
    assert 12 <= sum(3 <= k <= 40 for k in lens) and any(p != q and q.startswith(p) for p in pats for q in pats)
    assert te.LONG_A[:31] == te.LONG_B[:31] and te.LONG_A[31] != te.LONG_B[31]
    assert not any(p[0] in te.FILLER for p in pats), "the filler starts no pattern"
    assert te.SETS["qq"] == [b"qq"] + pats[1:]
    for name in te.SETS:
        info = te.host_handle(name).info()
        assert info.numOfPatterns == len(pats) and 600 < info.numOfStates < 1500 and info.maxPatternLen == 600 > te.HALO
    assert open(te.pattern_file("q"), "rb").read() == b"".join(p + b"\n" for p in pats)


def test_early_out_model_is_level_1_and_the_q_set_saturates_it():
    """level1_model restates the kernel's 3-gram test; it is prefilter_model's level 1.  Under "q" (a 1-byte pattern: 65 536 3-grams
    in a bitmap of 8192 bits) most filler positions pass it: every 1 KiB of filler is a dense group.  Under "qq" hardly any does."""
    data, _ = te.walks()
    for name in te.SETS:
        h = te.host_handle(name)
        assert np.array_equal(level1_model(h, data), prefilter_model(h, data, veto=False)[0])
    filler = te._filler(np.random.Generator(np.random.PCG64(1)), 64 * 1024)
    per_group = {name: level1_model(te.host_handle(name), filler).reshape(-1, 1024).sum(axis=1) for name in te.SETS}
    assert per_group["q"].min() >= 512, per_group["q"].min()
    assert per_group["qq"].max() <= te.LIST // 2, per_group["qq"].max()


def test_builders_are_deterministic():
    for build in (lambda: te.ragged(4097), lambda: te.walks(te.GROUP_SMALL, 7)[0], lambda: te.thresholds_small()[0]):
        first = build().copy()
        for cached in (te.ragged, te.walks, te.thresholds_small):
            cached.cache_clear()                   # built again, not looked up
        assert np.array_equal(build(), first)


@pytest.mark.parametrize("in_off", [0, 1, 9, 15])
def test_ragged_inputs(in_off):
    sizes = te.ragged_sizes(in_off)
    assert set(te.RAGGED_M) <= set(sizes) and all(m - in_off in sizes for m in te.RAGGED_M if m > in_off)
    assert any(n <= 15 - in_off for n in sizes) == (in_off < 15)       # the input that lies in front of the first aligned byte
    cut = te.pattern_id(te.LONG_A[:17])                                # what is left of LONG_A when its last 4 bytes lie beyond n
    for n in sizes:
        data = te.ragged(n)
        assert data.size == n and np.all(data[:40] == te.Q) and np.all(data[-41:] == te.Q)
        want, want_qq = te.want(data, "q"), te.want(data, "qq")
        assert want[0] == 1 and want[n - 1] == 1 and want_qq[n - 1] == 0           # `qq` at n - 1 would need the byte behind the input
        if n >= 96:
            at = n - te.RAGGED_CUT
            whole = np.concatenate([data, np.full(4, te.Q, dtype=np.uint8)])
            assert want[at] == cut and want_qq[at] == cut and te.want(whole, "q")[at] == te.pattern_id(te.LONG_A)
        if n >= 1023:
            mid = want_qq[64:n - 64]
            assert 0 < np.count_nonzero(mid) < mid.size // 20                        # sparse


@pytest.mark.parametrize("group,in_off,n", [(te.GROUP_SMALL, 0, te.WALKS_N), (te.GROUP_SMALL, 7, te.WALKS_N)])
def test_walks_straddle_the_boundaries_they_are_meant_for(group, in_off, n):
    data, planted = te.walks(group, in_off, n)
    specs = te.plant_specs()
    assert sorted(-rel for p, rel, _ in specs if len(p) <= 60) == list(range(72))
    for size in (200, 600):
        rels = [rel for p, rel, _ in specs if len(p) == size]
        assert sorted(rels) == sorted(2 * ([-d for d in te.START_BEFORE] + [e + 1 - size for e in te.END_BEHIND]))
    assert sum(whole is None for _, _, whole in specs) >= 18 + 20          # the near misses: wrong last byte
    for name in te.SETS:
        want = te.want(data, name)
        assert all(want[at] == pid for at, pid in planted), [(at, pid, want[at]) for at, pid in planted if want[at] != pid][:5]
        assert want[n - 600] == te.pattern_id(te.P600) and want[n - 30] == 0      # TAIL_CUT needs 8 bytes beyond n
    whole = np.concatenate([data, np.frombuffer(b"ABCDEFGH", dtype=np.uint8)])
    assert te.want(whole, "q")[n - 30] == te.pattern_id(te.TAIL_CUT)
    # the plants lie where a call at this input offset cuts its groups: every deep one begins in one group and ends in the next
    deep = [(at, len(te.PATTERNS[pid - 1])) for at, pid in planted[:-1] if pid in (te.pattern_id(te.P200), te.pattern_id(te.P600))]
    assert len(deep) == 18 and all((at + in_off) // group + 1 == (at + in_off + size - 1) // group for at, size in deep)
    ends = sorted((at + in_off + size - 1) % group for at, size in deep)
    assert all(ends.count(e) >= 2 for e in te.END_BEHIND)                 # P200 and P600, each ending 127, 128 and 129 bytes behind a group


@pytest.mark.parametrize("group,in_off", [(te.GROUP_BIG, 5), (te.GROUP_REF, 0)])
def test_shape_switch_inputs(group, in_off):
    data, planted = te.shape_switch(group, in_off)
    assert data.size == te.BIG_BYTES + 1 and te.SWITCH_SIZES == (te.BIG_BYTES - 1, te.BIG_BYTES, te.BIG_BYTES + 1)
    front = [at for at, _ in planted if at < te.BIG_BYTES // 2]
    back = [at for at, _ in planted if at >= te.BIG_BYTES // 2]
    assert len(front) == len(te.walks()[1]) - 1 and len(back) >= 5 and min(back) >= data.size - (64 << 10)
    n = te.SWITCH_SIZES[0]
    want = te.want(data[:n], "qq", omp=True)
    assert all(want[at] == pid for at, pid in planted)
    # dense stretches: the first group, the last (partial) one, one between sparse neighbours -- in the kernel's groups at this offset
    level1 = level1_model(te.host_handle("qq"), data[:n])
    padded = np.concatenate([np.zeros(in_off, dtype=bool), level1, np.zeros(-(in_off + n) % group, dtype=bool)])
    per_group = padded.reshape(-1, group).sum(axis=1)
    lone = 1000
    assert per_group[0] >= group - in_off - 1 and per_group[lone] >= group - 1 and max(per_group[lone - 1], per_group[lone + 1]) < group // 8
    assert per_group[-1] * 2 >= (in_off + n) % group > 0 and want[n - 2] == te.pattern_id(b"zz") and want[n - 1] == 0


def test_threshold_groups_have_exactly_the_intended_survivors():
    data, groups = te.thresholds_small()
    h = te.host_handle("qq")
    level1 = level1_model(h, data)
    assert np.array_equal(level1, prefilter_model(h, data, veto=False)[0])
    per_group = level1[:data.size // 1024 * 1024].reshape(-1, 1024).sum(axis=1)
    for target in te.SMALL_TARGETS:
        assert per_group[groups[target]] == target == te.survivors(data, 1024, groups[target])
    assert te.SMALL_TARGETS == (255, 256, 257, 511, 512, 513, 1024) and te.LIST == 256
    for g in groups.values():                                          # each between sparse (plain-list) groups
        assert per_group[g - 1] <= te.LIST // 2 and per_group[g + 1] <= te.LIST // 2
    lanes16 = level1[groups["lane16"] * 1024:][:1024].reshape(64, 16).sum(axis=1)
    lanes5 = level1[groups["lane5"] * 1024:][:1024].reshape(64, 16).sum(axis=1)
    for lanes in (lanes16, lanes5):
        assert te.LIST < lanes.sum() < 512 and 280 <= lanes.sum() <= 350      # crowded, not dense, about 300
    assert np.count_nonzero(lanes16 == 16) == 19 and np.all(np.sort(lanes16)[:-19] <= 3)
    assert lanes5.min() >= 4 and lanes5.max() <= 7 and abs(lanes5.mean() - 5) < 0.5
    want = te.want(data, "qq")
    g = groups[1024] * 1024
    assert np.all(want[g:g + 1024] == 1) and np.count_nonzero(want[groups[255] * 1024:][:1024]) >= 150


def test_big_threshold_groups_have_exactly_the_intended_survivors():
    data, groups = te.thresholds_big()
    assert data.size == te.BIG_BYTES
    assert te.BIG_TARGETS == {4096: (2047, 2048, 2049), 2048: (1023, 1024, 1025)}
    for (group, target), g in groups.items():
        assert te.survivors(data, group, g) == target
        assert te.survivors(data, group, g - 1) < group // 8 and te.survivors(data, group, g + 1) < group // 8
