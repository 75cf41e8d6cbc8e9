"""PFACX_gapsigOpen / PFACX_gapsigOpenText / PFACX_gapsigGetAnchors / PFACX_gapsigMatchFromHost on the CPU platforms (host-only handles: no
device needed) against the models of tests/gapsig_ref.py: every case of the table through both open calls, every gap spelling against the binary
form, every refusal with its line or id, the getter against the handle's own pattern list, a one-part signature against PFACX_sig*, every
capacity from 0 to the list's length with and without the end array, the status rows, the stale object, and the seeded random case with the
figures that make it worth running."""

import numpy as np
import pytest

from pfac_amd import api
from tests import gapsig_ref as ref
from tests import sig_ref
from tests.gapsig_ref import test_the_models_agree_on_every_case  # noqa: F401  (runs here: gapsig_ref.py is not collected)

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
INVALID, NOT_EXIST, TRUNCATED, BAD_HANDLE = (api.STATUS.INVALID_PARAMETER, api.STATUS.LIB_NOT_EXIST, api.STATUS.OUTPUT_TRUNCATED,
                                             api.STATUS.INVALID_HANDLE)
GUARD = 16


def host_handle(platform=api.PFAC_PLATFORM_CPU):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    return h


def host_gapsig(sg, data, capacity=None, with_end=True):
    """match_host into poisoned arrays of `capacity` entries (default: the full length, asked for first) with GUARD poisoned ints on both sides
    -> (status, (pos, ids, end) of the entries written, the full length); nothing outside the written entries may change, nor the input"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    n = buf.size
    if capacity is None:
        st, capacity = sg.match_host(buf.ctypes.data, n, None, None, None, 0, check=False)
        assert st in (0, TRUNCATED) and (st == TRUNCATED) == (capacity > 0)
    ids, pos, end = (np.full(GUARD + capacity + GUARD, -7, dtype=np.int32) for _ in range(3))
    st, total = sg.match_host(buf.ctypes.data, n, ids.ctypes.data + 4 * GUARD, pos.ctypes.data + 4 * GUARD,
                              end.ctypes.data + 4 * GUARD if with_end else None, capacity, check=False)
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > capacity)
    k = min(total, capacity)
    for a in (ids, pos, end):
        assert np.all(a[:GUARD] == -7) and np.all(a[GUARD + capacity:] == -7), "wrote outside the arrays"
        assert np.all(a[GUARD + k:GUARD + capacity] == -7), "wrote behind the list"
    if not with_end:
        assert np.all(end == -7)
    assert buf.tobytes() == bytes(data), "the caller's input was modified"
    return st, tuple(a[GUARD:GUARD + k].copy() for a in (pos, ids, end)), total


def check_getter(h, sg, sigs, max_len=0):
    """the getter equals the documented rule, and handle id q IS the q-th distinct anchor: the handle finds each anchor under that id"""
    got = sg.anchors()
    want, anchors = ref.model_anchors(sigs, max_len)
    for g, w, what in zip(got, want, ("anchor id", "anchor part", "anchor offset", "anchor length")):
        assert g.tolist() == w.tolist(), what
    for q, anchor in enumerate(anchors, start=1):
        found = h.match_host_array(np.frombuffer(anchor, dtype=np.uint8))
        assert int(found[0]) == q, f"the handle's pattern {q} is not the {q}-th distinct anchor"
    assert h.caseInsensitive() == 0
    return got


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_equals_the_models(case, platform, pname):
    name, lines, data, cut = case
    sigs = ref.parse_lines(lines)
    h = host_handle(platform)
    try:
        for form in ("text", "binary"):
            sg = h.gapsigOpenText(ref.text_of(lines), cut) if form == "text" else h.gapsigOpen(*ref.csr_of(sigs), cut)
            with sg:
                assert sg.status == 0 and sg.bad == 0 and sg.num_sigs == len(sigs)
                anchors = check_getter(h, sg, sigs, cut)
                want = ref.check_models(sigs, data, anchors, name)
                st, got, total = host_gapsig(sg, data)
                assert st == 0 and total == want[0].size
                ref.same(got, want, f"{name}/{pname}/{form}")
                if name in ref.WANT:
                    ids, pos, end = ref.WANT[name]
                    ref.same(got, (pos, ids, end), f"{name}/{pname}/{form}: by hand")
    finally:
        h.destroy()


def test_every_capacity_and_no_end_array():
    name, lines, data, cut = next(c for c in ref.CASES if c[0] == "owner-many-starts")
    sigs = ref.parse_lines(lines)
    h = host_handle()
    try:
        with h.gapsigOpenText(ref.text_of(lines)) as sg:
            want = ref.check_models(sigs, data, sg.anchors(), name)
            total = int(want[0].size)
            assert total == 133
            for cap in list(range(0, 6)) + [total - 1, total, total + 1]:
                for with_end in (True, False):
                    st, got, n = host_gapsig(sg, data, cap, with_end)
                    assert n == total and st == (TRUNCATED if cap < total else 0)
                    k = min(cap, total)
                    ref.same(got[:2], [w[:k] for w in want[:2]], f"capacity {cap}")
                    if with_end:
                        assert got[2].tolist() == want[2][:k].tolist()
            # the starts of one anchor occurrence ascend
            assert want[0][-64:].tolist() == sorted(want[0][-64:].tolist())
    finally:
        h.destroy()


SPELLINGS = [("{0}", 0, 0), ("{7}", 7, 7), ("{2-6}", 2, 6), ("{-5}", 0, 5), ("[0]", 0, 0), ("[7]", 7, 7), ("[2-6]", 2, 6), ("[-5]", 0, 5),
             ("{65535}", 65535, 65535), ("{65500-65535}", 65500, 65535), ("{0-63}", 0, 63), (" {3} ", 3, 3), ("\t[1-2]\t", 1, 2)]


def test_every_gap_spelling_equals_the_binary_form():
    data = b"ab" + b"." * 5 + b"cd ab......cd"
    h = host_handle()
    try:
        for text, lo, hi in SPELLINGS:
            line = "61 62" + text + "63 64"
            assert ref.parse_line(line.encode())[1] == [(lo, hi)], text
            with h.gapsigOpenText((line + "\r\n").encode()) as sg:
                got = host_gapsig(sg, data)[1]
            part = lambda raw: (np.frombuffer(raw, dtype=np.uint8), np.full(len(raw), 0xFF, dtype=np.uint8))  # noqa: E731
            with h.gapsigOpen(*ref.csr_of([([part(b"ab"), part(b"cd")], [(lo, hi)])])) as sg:
                want = host_gapsig(sg, data)[1]
            ref.same(got, want, text)
        # `??` runs stay inside their part: one part of six bytes, not a gap
        with h.gapsigOpenText(b"61 62 ?? ?? 63 64\n") as sg:
            assert sg.anchors()[1].tolist() == [0, 0] and host_gapsig(sg, b"ab..cd ab.cd")[1][0].tolist() == [0]
    finally:
        h.destroy()


TEXT_REFUSALS = [
    (b"61 62\n{1} 61\n", 2), (b"61 {1}\n", 1), (b"61 {1} {2} 62\n", 1), (b"61 62\n61 62\n61 {2-1} 62\n", 3), (b"61 * 62\n", 1), (b"61 {1-} 62\n", 1),
    (b"61 {65536} 62\n", 1), (b"61 {0-65536} 62\n", 1), (b"61 {} 62\n", 1), (b"61 {-} 62\n", 1), (b"61 {1] 62\n", 1), (b"61 [1} 62\n", 1),
    (b"61 {1 62\n", 1), (b"61 { 1} 62\n", 1), (b"61 {1--2} 62\n", 1), (b"61 {1-2-3} 62\n", 1), (b"61 {a} 62\n", 1), (b"61 } 62\n", 1),
    (b"61 62\n\n", 2), (b"6 {1} 62\n", 1), (b"61 {1} 6\n", 1), (b"61 6g\n", 1), (b"61 62\n61 {1} 62", 2), (b"{1}\n", 1),
    # what the binary form refuses, by line: slack 64, 65 parts, no anchor
    (b"61 62\n61 {0-64} 62\n", 2), (b"61 {0-32} 62 {0-32} 63\n", 1), (b"61 {0-63} 62\n" + b" {1} ".join([b"61"] * 65) + b"\n", 2),
    (b"61 62\n0A {1} ?? {2} 4?\n", 2), (b"?? {1-2} ??\n", 1),
]


def test_the_text_form_refuses_with_the_line():
    h = host_handle()
    try:
        h.readPatternFromMemory(b"keep\n")
        for text, line in TEXT_REFUSALS:
            sg = h.gapsigOpenText(text, check=False)
            assert (sg.status, sg.bad) == (INVALID, line), (text, sg.status, sg.bad)
            assert not sg._c
            if text.endswith(b"\n"):                                # the model refuses that line too, and none in front of it
                rows = text.split(b"\n")
                assert all(ref.check_limits(ref.parse_line(row)) is None for row in rows[:line - 1])
                try:
                    refused = ref.check_limits(ref.parse_line(rows[line - 1])) is not None
                except ValueError:
                    refused = True
                assert refused, f"the model accepts {text!r}"
        assert h.gapsigOpenText(b"", check=False).status == INVALID
        assert h.match_host_array(np.frombuffer(b"keep", dtype=np.uint8))[0] == 1, "a refused open call changed the handle's set"
        # 64 parts and slack 63 are the last that pass
        with h.gapsigOpenText(b" {1} ".join([b"61"] * 64) + b"\n61 {0-63} 62\n") as sg:
            assert sg.status == 0 and sg.num_sigs == 2
    finally:
        h.destroy()


def _part(raw, mask=None):
    raw = np.frombuffer(bytes(raw), dtype=np.uint8)
    return raw, np.full(raw.size, 0xFF, dtype=np.uint8) if mask is None else np.asarray(mask, dtype=np.uint8)


def test_the_binary_form_refuses_with_the_id():
    good = ([_part(b"ab"), _part(b"cd")], [(0, 2)])
    bad = {
        "slack 64": ([_part(b"ab"), _part(b"cd"), _part(b"ef")], [(5, 37), (0, 32)]),
        "65 parts": ([_part(b"a")] * 65, [(1, 1)] * 64),
        "no anchor": ([_part(b"\n"), _part(b"ab", [0xF0, 0x00])], [(0, 1)]),
        "lo above hi": ([_part(b"ab"), _part(b"cd")], [(3, 2)]),
        "hi above 65 535": ([_part(b"ab"), _part(b"cd")], [(0, 65536)]),
    }
    h = host_handle()
    try:
        h.readPatternFromMemory(b"keep\n")
        for what, sig in bad.items():
            for at in (1, 2, 3):
                sigs = [good, good]
                sigs.insert(at - 1, sig)
                sg = h.gapsigOpen(*ref.csr_of(sigs), check=False)
                assert (sg.status, sg.bad) == (INVALID, at), (what, at, sg.status, sg.bad)
        # an empty part, a part of 65 536 bytes, a signature without a part: the CSR arrays say so
        values, masks, part_off, sig_part, lo, hi = ref.csr_of([good, good])
        empty = part_off.copy()
        empty[3] = empty[2]
        assert (lambda s: (s.status, s.bad))(h.gapsigOpen(values, masks, empty, sig_part, lo, hi, check=False)) == (INVALID, 2)
        none = sig_part.copy()
        none[1] = 0
        assert (lambda s: (s.status, s.bad))(h.gapsigOpen(values, masks, part_off, none, lo, hi, check=False)) == (INVALID, 1)
        long_part = _part(bytes(65536))
        sg = h.gapsigOpen(*ref.csr_of([good, ([_part(b"ab"), long_part], [(0, 1)])]), check=False)
        assert (sg.status, sg.bad) == (INVALID, 2)
        # the span: every other limit keeps it far below 2^31 - 1 -- the model's check says the same of the widest signature there is
        assert 64 * 65535 + 63 * 65535 < 2 ** 31 - 1
        assert h.match_host_array(np.frombuffer(b"keep", dtype=np.uint8))[0] == 1, "a refused open call changed the handle's set"
        # the largest gaps pass, values are canonicalised: a value bit outside the mask changes nothing
        v, m = _part(b"a\xffc", [0xFF, 0x00, 0xFF])
        with h.gapsigOpen(*ref.csr_of([([(v, m), _part(b"z")], [(65535, 65535)])])) as sg:
            assert sg.status == 0 and host_gapsig(sg, b"a.c" + b"." * 65535 + b"z")[1][2].tolist() == [65539]
    finally:
        h.destroy()


def test_a_one_part_signature_equals_the_sig_calls():
    lines = ["61 ?? 63", "4D 5A ?? ?? 50 45", "6? 62", "61 ?? 63"]
    data = b"abc axc MZ..PE MZ.PE ab cb aXc"
    h = host_handle()
    try:
        with h.sigOpenText(sig_ref.text_of(lines)) as sg:
            pos, ids = sg.match_host_array(np.frombuffer(data, dtype=np.uint8))
            lens = [0] + [len(v) for v, _ in sig_ref.parse_lines(lines)]
        with h.gapsigOpenText(ref.text_of(lines)) as gs:
            st, got, _ = host_gapsig(gs, data)
        assert pos.size >= 8
        ref.same(got, (pos, ids, [int(p) + lens[int(i)] for p, i in zip(pos, ids)]), "one part")
    finally:
        h.destroy()


def test_status_rows_and_the_stale_object():
    h = host_handle()
    buf = np.frombuffer(b"ab.cd", dtype=np.uint8).copy()
    out = np.zeros(8, dtype=np.int32)
    try:
        sg = h.gapsigOpenText(b"61 62 {0-2} 63 64\n")
        args = (out.ctypes.data, out.ctypes.data, out.ctypes.data)
        assert sg.match_host(buf.ctypes.data, 0, None, None, None, 0) == (0, 0)
        assert sg.match_host(None, 5, *args, 8, check=False)[0] == INVALID
        assert sg.match_host(buf.ctypes.data, 1 << 31, *args, 8, check=False)[0] == INVALID
        assert sg.match_host(buf.ctypes.data, 5, None, None, None, 1, check=False)[0] == INVALID
        assert sg.match_host(buf.ctypes.data, 5, None, None, None, 0, check=False) == (TRUNCATED, 1)
        assert sg.match_device(buf.ctypes.data, 5, *args, 8, check=False)[0] == NOT_EXIST
        assert sg.pairs_device(buf.ctypes.data, 5, out.ctypes.data, out.ctypes.data, 1, None, None, None, 0, check=False)[0] == NOT_EXIST
        assert sg._lib.PFACX_gapsigGetAnchors(sg._c, None, None, None, None, 1) == INVALID
        assert sg._lib.PFACX_gapsigGetAnchors(sg._c, None, None, None, None, 2) == 0
        assert sg._lib.PFACX_gapsigMatchFromHost(None, buf.ctypes.data, 5, None, None, None, 0, None) == BAD_HANDLE
        before = h.info().deviceTableBytes
        h.readPatternFromMemory(b"other\n")                       # the object goes stale
        assert sg.match_host(buf.ctypes.data, 5, None, None, None, 0, check=False)[0] == INVALID
        assert sg.anchors(check=False) is not None and sg._lib.PFACX_gapsigGetAnchors(sg._c, None, None, None, None, 2) == INVALID
        assert h.info().deviceTableBytes == before
        assert sg.close() == 0
        left = h.gapsigOpenText(b"61 62 {0-2} 63 64\n")            # PFAC_destroy closes what is left open
        assert left.status == 0
    finally:
        h.destroy()


def test_the_seeded_random_case_is_worth_running():
    sigs, data = ref.random_case()
    assert all(ref.check_limits(s) is None for s in sigs)
    h = host_handle(api.PFAC_PLATFORM_CPU_OMP)
    try:
        with h.gapsigOpen(*ref.csr_of(sigs)) as sg:
            anchors = check_getter(h, sg, sigs)
            want, figures = ref.random_case_figures(sigs, data, anchors)
            print(figures)
            assert figures["entries"] >= 200 and figures["deep"] >= 20 and figures["late_owner"] >= 10 and figures["multi_start"] >= 10, figures
            for i in (1, 50, 120, 200):
                assert ref.starts_re(sigs[i - 1], data) == sorted(ref.brute(sigs[i - 1], data)), f"signature {i}: re"
            st, got, total = host_gapsig(sg, data)
            assert st == 0
            ref.same(got, want, "the random case")
    finally:
        h.destroy()
