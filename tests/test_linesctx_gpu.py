"""PFACX_matchLinesContextFromDevice (and once the host form on the GPU platform) against the model of tests/linesctx_ref.py: the cases of
tests/test_linesctx_host.py on the device form, plus what only the device has -- misaligned input pointers, the scratch accounting and
PFACX_trim, the gather over a context list, the kernel variants.  All arrays are poisoned and carry guard entries behind capacity
(tests/linesctx_helpers.py).  The largest input is 320 KiB."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402
from tests import linesctx_ref as model  # noqa: E402
from tests.lines_helpers import pattern_file  # noqa: E402
from tests.linesctx_helpers import GUARD, POISON, device_context, host_context  # noqa: E402
from tests.test_lines_gpu import device_gather, device_lines, gpu_handle  # noqa: E402

INVALID = api.STATUS.INVALID_PARAMETER


@pytest.fixture(scope="module")
def x_handle(workdir):
    h = gpu_handle(pattern_file(workdir, "ctx_x", model.X))
    yield h
    h.destroy()


def check(h, pats, data, before, after, invert, what, nocase=False, **kw):
    got = device_context(h, data, before, after, invert, **kw)
    model.same(got, model.context_model(pats, data, before, after, invert, nocase), what)
    return got


@pytest.mark.parametrize("invert", [False, True])
def test_no_context_is_the_plain_call(x_handle, invert):
    data = model.tiny_lines(200, [0, 1, 2, 40, 63, 64, 65, 130, 199])
    got = device_context(x_handle, data, 0, 0, invert)
    nl, start, length, index = device_lines(x_handle, data, invert)
    assert got[4][0] == nl and got[4][1] == got[4][2] == start.size
    assert np.array_equal(got[0], start) and np.array_equal(got[1], length) and np.array_equal(got[2], index)
    assert np.all(got[3] & 1 == 1), "without context every listed line is a member of H"
    model.same(got, model.context_model(model.X, data, 0, 0, invert), f"invert {invert}")


@pytest.mark.parametrize("hit", model.WORD_EDGE_HITS)
def test_single_hits_at_the_word_edges_of_the_line_bitmap(x_handle, hit):
    data = model.tiny_lines(model.WORD_EDGE_LINES, [hit])
    for before in model.WORD_EDGE_WINDOWS:
        for after in model.WORD_EDGE_WINDOWS:
            check(x_handle, model.X, data, before, after, False, f"hit {hit}/before {before}/after {after}")
    check(x_handle, model.X, data, 1, 32, True, f"hit {hit}/inverted")


@pytest.mark.parametrize("mis", [1, 15])
def test_input_pointer_off_alignment(x_handle, mis):
    for hit in (32, model.WORD_EDGE_LINES - 1):
        data = model.tiny_lines(model.WORD_EDGE_LINES, [hit])
        for before, after in ((1, 1), (33, 31), (0, 32)):
            check(x_handle, model.X, data, before, after, False, f"mis {mis}/hit {hit}/before {before}/after {after}", in_offset=mis)
        check(x_handle, model.X, data, 1, 0, True, f"mis {mis}/hit {hit}/inverted", in_offset=mis)


def test_windows_that_cross_whole_words_and_64_words(x_handle):
    data = model.wave_input()
    for before in model.WAVE_WINDOWS:
        for after in model.WAVE_WINDOWS:
            got = check(x_handle, model.X, data, before, after, False, f"before {before}/after {after}")
            assert got[4][2:] == (1, 1) and got[4][1] == min(before, model.WAVE_HIT) + 1 + min(after, model.WAVE_LINES - 1 - model.WAVE_HIT)


@pytest.mark.parametrize("case", model.SMALL, ids=[c[0] for c in model.SMALL])
def test_clipping_groups_and_invert(workdir, case):
    name, pats, data, before, after, invert = case
    h = gpu_handle(pattern_file(workdir, "ctx_" + name, pats))
    try:
        check(h, pats, data, before, after, invert, name)
    finally:
        h.destroy()


def test_group_counts_of_windows_apart_touching_and_overlapping(x_handle):
    want = {"windows-one-line-apart": (2, [0] * 9 + [1] * 9), "windows-touching": (1, [0] * 20), "windows-overlapping": (1, [0] * 24)}
    for name, pats, data, before, after, invert in model.SMALL:
        if name in want:
            got = device_context(x_handle, data, before, after, invert)
            assert (got[4][3], (got[3] >> 1).tolist()) == want[name], name
            assert got[2][(got[3] & 1) == 1].tolist() == [10, 20], name


@pytest.mark.parametrize("num", model.INVERT_LINE_COUNTS)
def test_inverted_with_every_line_matching_selects_nothing(x_handle, num):
    data = model.every_line_matches(num)
    for before, after in ((0, 0), (1, 1), (33, 2), (model.MAX, model.MAX)):
        got = device_context(x_handle, data, before, after, True)
        assert got[4] == (num, 0, 0, 0), f"{num} lines/before {before}/after {after}: {got[4]}"
    # one line that does not match, the last: its window reaches back, nothing behind numLines reaches in
    data = data[:-2] + b"z\n"
    check(x_handle, model.X, data, 2, model.MAX, True, f"{num} lines, the last does not match")


@pytest.mark.parametrize("window", model.FOLD_WINDOWS)
def test_320_kib_of_short_lines(x_handle, window):
    data = model.fold_input()
    got = check(x_handle, model.X, data, window, window, False, f"window {window}")
    assert got[4][2:] == (6, 2), "six hits, a group at each end"


def test_caseless_set(workdir):
    pats, data, before, after = model.NOCASE
    h = gpu_handle(pattern_file(workdir, "ctx_nocase", pats), api.PFACX_READ_NOCASE)
    try:
        got = check(h, pats, data, before, after, False, "nocase", nocase=True)     # (device_context: the input is unchanged afterwards)
        assert got[4][2] == 2 and model.context_model(pats, data, before, after, False, nocase=False)[4][2] == 0, "only the folded input matches"
        check(h, pats, data, 0, 1, True, "nocase/inverted", nocase=True)
    finally:
        h.destroy()


def test_null_index_and_null_tag(x_handle):
    data = model.tiny_lines(model.WORD_EDGE_LINES, [33, 64])
    full = device_context(x_handle, data, 2, 31, False)
    for with_index, with_tag in ((False, True), (True, False), (False, False)):
        got = device_context(x_handle, data, 2, 31, False, with_index=with_index, with_tag=with_tag)
        assert got[4] == full[4] and np.array_equal(got[0], full[0]) and np.array_equal(got[1], full[1])
        assert not with_index or np.array_equal(got[2], full[2])
        assert not with_tag or np.array_equal(got[3], full[3])


def test_host_form_on_the_gpu_platform(x_handle):
    data = model.tiny_lines(model.WORD_EDGE_LINES, [0, 33, 64])
    for invert in (False, True):
        model.same(host_context(x_handle, data, 2, 31, invert), model.context_model(model.X, data, 2, 31, invert), f"invert {invert}")


def test_error_rows_on_a_device_handle(workdir):
    h = gpu_handle(pattern_file(workdir, "ctx_errors", model.X))
    try:
        d_in = torch.from_numpy(np.frombuffer(b"x\ncd\n", dtype=np.uint8).copy()).to("cuda:0")
        d = [torch.full((5 + GUARD,), POISON, dtype=torch.int32, device="cuda:0") for _ in range(4)]
        I, (S, L, X, T) = d_in.data_ptr(), (t.data_ptr() for t in d)
        call = lambda *a: h.matchLinesContextFromDevice(*a, check=False)[0]  # noqa: E731
        assert call(I, 5, 0, 1, 1, S, L, X, T, 4) == INVALID and call(I, 1 << 31, 0, 1, 1, S, L, X, T, 1 << 31) == INVALID
        assert call(I, 5, 4, 1, 1, S, L, X, T, 5) == INVALID, "an unknown flag bit"
        assert call(None, 5, 0, 1, 1, S, L, X, T, 5) == INVALID and call(I, 5, 0, 1, 1, None, L, X, T, 5) == INVALID
        assert call(I, 5, 0, 1, 1, S, None, X, T, 5) == INVALID
        assert h.matchLinesContextFromDevice(I, 0, 1, 3, 3, S, L, X, T, 0, check=False) == (0, 0, 0, 0, 0), "size == 0"
        torch.cuda.synchronize()
        assert all(bool((t == POISON).all()) for t in d), "a refused call or a call of size 0 wrote"
        assert call(I, 5, 0, 1, 1, S, L, X, T, 5) == 0, "the handle is usable after refused calls"
    finally:
        h.destroy()
    bare = api.PFAC.create()
    try:
        assert bare.matchLinesContextFromDevice(I, 5, 0, 1, 1, S, L, X, T, 5, check=False)[0] == api.STATUS.PATTERNS_NOT_READY
    finally:
        bare.destroy()


def context_scratch_bytes(size, mis=0):
    """the formula of include/pfac_ext.h"""
    r = lambda b: (b + 255) & ~255  # noqa: E731
    B = (size + mis) // 2048 + 1
    return r(256 * B + 256) + r(128 * B) + 4 * r(4 * B) + 2 * r(4 * (B + 1)) + r(4)


def test_scratch_accounting_and_trim(workdir):
    pf = pattern_file(workdir, "ctx_scratch", model.X)
    data = model.tiny_lines(30000, [5, 29000])
    n = len(data)
    plain, h = gpu_handle(pf), gpu_handle(pf)
    try:
        fresh = h.info().deviceScratchBytes
        device_lines(plain, data, False)
        device_lines(h, data, False)
        after_plain = h.info().deviceScratchBytes
        assert after_plain == plain.info().deviceScratchBytes > fresh
        check(h, model.X, data, 3, 3, False, "first context call")
        assert h.info().deviceScratchBytes == after_plain + context_scratch_bytes(n), "the context stage takes what the header says, and a plain call took none of it"
        device_lines(h, data, True)
        check(h, model.X, data, 70, 0, True, "second context call")
        assert h.info().deviceScratchBytes == after_plain + context_scratch_bytes(n), "grow-only: the same size needs no more"
        assert plain.info().deviceScratchBytes == after_plain
        h.trim()
        assert h.info().deviceScratchBytes == fresh, "trim gives it back"
        check(h, model.X, data, 3, 3, False, "after trim")
    finally:
        h.destroy()
        plain.destroy()


def test_gather_over_a_context_list(workdir):
    name, pats, data, before, after, invert = next(c for c in model.SMALL if c[0] == "ordinary-text")
    h = gpu_handle(pattern_file(workdir, "ctx_gather", pats))
    try:
        for b, a in ((before, after), (0, 2), (3, 0)):
            got, kept = device_context(h, data, b, a, invert, keep=True)
            want = model.context_model(pats, data, b, a, invert)
            model.same(got, want, f"before {b}/after {a}")
            expect = model.text_of(data, want)[0]
            st, total, text = device_gather(h, kept, len(data), got[0].size)
            assert (st, total) == (0, len(expect)) and text[:total] == expect, f"before {b}/after {a}: the gathered text differs"
    finally:
        h.destroy()


def test_example_program_prints_what_grep_prints():
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-C", os.path.join(root, "examples"), "context_example"], check=True, stdout=subprocess.PIPE)
    source = open(os.path.join(root, "examples", "context_example.cpp")).read()
    log = "".join(line + "\n" for line in re.findall(r'^\s+"(10:[^"]*)\\n";?$', source, flags=re.M)).encode()
    assert log.count(b"\n") == 10, "the log of the example"
    p = subprocess.run([os.path.join(root, "examples", "context_example")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout == model.text_of(log, model.context_model([b"ERROR", b"timeout"], log, 1, 1))[1]
    assert p.stdout.count(b"--\n") == 1 and b"3:10:00:03 upstream timeout" in p.stdout and b"2-10:00:02" in p.stdout


@pytest.mark.parametrize("variant,vname", [(api.PFACX_KERNEL_NAIVE, "naive"), (api.PFACX_KERNEL_FILTER, "filter")])
def test_kernel_variants_equal_the_default(workdir, x_handle, variant, vname):
    data = model.tiny_lines(3000, [0, 31, 64, 1500, 2047, 2048, 2999])
    h = gpu_handle(pattern_file(workdir, "ctx_" + vname, model.X), variant=variant)
    try:
        for before, after, invert in ((2, 40, False), (1, 0, True)):
            got = check(h, model.X, data, before, after, invert, f"{vname}/before {before}/after {after}/invert {invert}")
            default = device_context(x_handle, data, before, after, invert)
            assert got[4] == default[4] and all(np.array_equal(g, d) for g, d in zip(got[:4], default[:4])), f"{vname} differs from the default variant"
    finally:
        h.destroy()
