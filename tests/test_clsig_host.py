"""PFACX_clsigOpen / PFACX_clsigOpenText / PFACX_clsigGetAnchors / PFACX_clsigMatchFromHost on the CPU platforms (host-only handles: no device
needed) against the models of tests/clsig_ref.py: every case of the table through both open calls, every refusal with its line or id and the set
untouched behind it, the fusion limits, the text parser line by line (each accepted line also compiled by re), the getter, a one-part set against
PFACX_sig* and a set of full classes, nibble classes and gaps against PFACX_gapsig*, every capacity with and without the end array, the status
rows, the stale object, and the seeded random case."""

import re

import numpy as np
import pytest

from pfac_amd import api
from tests import clsig_ref as ref
from tests.clsig_ref import test_the_models_agree_on_every_case  # noqa: F401  (runs here: clsig_ref.py is not collected)

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
INVALID, NOT_EXIST, TRUNCATED, BAD_HANDLE = (api.STATUS.INVALID_PARAMETER, api.STATUS.LIB_NOT_EXIST, api.STATUS.OUTPUT_TRUNCATED,
                                             api.STATUS.INVALID_HANDLE)
GUARD = 16


def host_handle(platform=api.PFAC_PLATFORM_CPU):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    return h


def host_clsig(sg, data, capacity=None, with_end=True):
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
    name, lines, data, cut, flags = case
    sigs = ref.parse_lines(lines)
    h = host_handle(platform)
    try:
        for form in ("text", "binary"):
            sg = h.clsigOpenText(ref.text_of(lines), cut, flags) if form == "text" else h.clsigOpen(*ref.csr_of(sigs), cut, flags)
            with sg:
                assert sg.status == 0 and sg.bad == 0 and sg.num_sigs == len(sigs)
                anchors = check_getter(h, sg, sigs, cut)
                want = ref.check_models(sigs, data, anchors, name, flags, lines)
                st, got, total = host_clsig(sg, data)
                assert st == 0 and total == want[0].size
                ref.same(got, want, f"{name}/{pname}/{form}")
                if name in ref.WANT:
                    ids, pos, end = ref.WANT[name]
                    ref.same(got, (pos, ids, end), f"{name}/{pname}/{form}: by hand")
    finally:
        h.destroy()


def test_every_capacity_and_no_end_array_and_both_ends():
    name, lines, data, cut, flags = next(c for c in ref.CASES if c[0] == "two-class-parts-share-bytes")
    sigs = ref.parse_lines(lines)
    h = host_handle()
    try:
        for flags in (0, ref.SHORTEST):
            with h.clsigOpenText(ref.text_of(lines), 0, flags) as sg:
                want = ref.check_models(sigs, data, sg.anchors(), name, flags, lines)
                total = int(want[0].size)
                assert total >= 6
                for cap in list(range(0, 4)) + [total - 1, total, total + 1]:
                    for with_end in (True, False):
                        st, got, n = host_clsig(sg, data, cap, with_end)
                        assert n == total and st == (TRUNCATED if cap < total else 0)
                        k = min(cap, total)
                        ref.same(got[:2], [w[:k] for w in want[:2]], f"capacity {cap}")
                        if with_end:
                            assert got[2].tolist() == want[2][:k].tolist()
        for bits in (2, 4, 1 << 31):
            assert h.clsigOpenText(ref.text_of(lines), 0, bits, check=False).status == INVALID, "an unknown flag bit"
            assert h.clsigOpen(*ref.csr_of(sigs), 0, bits, check=False).status == INVALID
    finally:
        h.destroy()


ACCEPTED_LINES = [b"AKIA[0-9A-Z]{16}", b"ghp_[A-Za-z0-9]{36}", b"xox[baprs]-[0-9A-Za-z-]{10,48}", b"-----BEGIN [A-Z ]{0,20}PRIVATE KEY-----",
                  b"[0-9]{3}-[0-9]{2}-[0-9]{4}", b"sess=[0-9a-f]{32};", b"(?<![0-9A-Za-z+/])tok_[0-9A-Za-z+/]{8}(?![0-9A-Za-z+/])",
                  b"a\\.b\\\\c\\[d\\]e\\(f\\)g\\{h\\}i\\?j\\*k\\+l\\|m\\^n\\$", b"x\\x41\\x00\\n\\r\\t\\f\\v\\0y", b"k\\d\\D\\w\\W\\s\\S", b"k[\\d_][^\\s]{2}[\\w-]",
                  b"k.{1,3}z", b"k[-a]{2}[a-]?[a\\-z][\\]\\\\^]", b"k[a^]{2}", b"k\xe9\xff[\x80-\xff]{2}", b"ab?c{0,1}d{3}", b"k[.(){}?*+|$]{2}",
                  b"key=[^;\\n]{1,40};\r"]


def test_the_text_form_line_by_line():
    """every accepted line means to the library what it means to re (the models run re on the very line), every refused line is refused alone
    and as the third of three with its line number, and the set stays untouched"""
    rng = np.random.default_rng(7)
    h = host_handle()
    try:
        for line in ACCEPTED_LINES:
            core = line[:-1] if line.endswith(b"\r") else line
            re.compile(core, re.S)
            sig = ref.parse_line(line)
            assert ref.check_limits(sig) is None, line
            data = rng.integers(0, 256, 600, dtype=np.uint8)
            ref.embed([sig], data, int(rng.integers(0, 1 << 30)), per_sig=4)
            with h.clsigOpenText(line + b"\n") as sg:
                anchors = check_getter(h, sg, [sig])
                want = ref.check_models([sig], data, anchors, repr(line), 0, [core])
                assert want[0].size >= 1, line
                ref.same(host_clsig(sg, data)[1], want, repr(line))
            with h.clsigOpen(*ref.csr_of([sig])) as sg:
                ref.same(host_clsig(sg, data)[1], want, f"{line!r}: the binary form")
        h.readPatternFromMemory(b"keep\n")
        for line in ref.REFUSED_LINES:
            sg = h.clsigOpenText(line + b"\n", check=False)
            assert (sg.status, sg.bad) == (INVALID, 1) and not sg._c, (line, sg.status, sg.bad)
            sg = h.clsigOpenText(b"ab[0-9]\nabc\n" + line + b"\n" + b"a*\n", check=False)
            assert (sg.status, sg.bad) == (INVALID, 3), (line, sg.status, sg.bad)
        for text, bad in ((b"", 0), (b"abc", 1), (b"abc\nab[0-9]", 2), (b"abc\n\n", 2), (b"[0-9]{3}[a-f]{2}\n", 1), (b"abc\n\\n[0-9]\n", 2),
                          (b"abc\nab.{0,64}c\n", 2), (b"a.{0,32}b.{0,32}c\n", 1)):
            sg = h.clsigOpenText(text, check=False)
            assert (sg.status, sg.bad) == (INVALID, bad), (text, sg.status, sg.bad)
        assert h.match_host_array(np.frombuffer(b"keep", dtype=np.uint8))[0] == 1, "a refused open call changed the handle's set"
    finally:
        h.destroy()


def _sig(*elems, nb=None, na=None):
    return ([(frozenset(m if not isinstance(m, int) else [m]), lo, hi) for m, lo, hi in elems], nb, na)


def test_the_binary_form_refuses_with_the_id():
    good = _sig((b"a", 1, 1), (b"b", 1, 1), (b"0123", 1, 2))
    digits = frozenset(b"0123456789")
    bad = {
        "slack 64": _sig((b"a", 1, 1), (digits, 0, 32), (b"b", 1, 1), (digits, 0, 32)),
        "65 parts": ([(frozenset(b"a"), 1, 1), (digits, 1, 1)] * 32 + [(frozenset(b"a"), 1, 1)], None, None),
        "no anchor": _sig((digits, 3, 3), (b"abcdef", 2, 2)),
        "only a newline": _sig((b"\n", 1, 1), (digits, 1, 1)),
        "a literal part of 65 536 bytes": _sig((b"a", 65535, 65535), (b"b", 1, 1)),
    }
    h = host_handle()
    try:
        h.readPatternFromMemory(b"keep\n")
        for what, sig in bad.items():
            assert ref.check_limits(sig) is not None, what
            for at in (1, 2, 3):
                sigs = [good, good]
                sigs.insert(at - 1, sig)
                sg = h.clsigOpen(*ref.csr_of(sigs), check=False)
                assert (sg.status, sg.bad) == (INVALID, at), (what, at, sg.status, sg.bad)
        # two bad ones: the first id; a structural refusal comes before an anchor refusal of a lower id
        sg = h.clsigOpen(*ref.csr_of([good, bad["slack 64"], bad["65 parts"]]), check=False)
        assert (sg.status, sg.bad) == (INVALID, 2)
        sg = h.clsigOpen(*ref.csr_of([bad["no anchor"], good, bad["slack 64"]]), check=False)
        assert (sg.status, sg.bad) == (INVALID, 3)
        # what only the arrays can say: lo > hi, hi == 0, hi > 65 535, a class outside the table, a boundary outside it, no elements, an empty class
        classes, cls, lo, hi, sig_elem, nb, na = ref.csr_of([good, good])

        def refused(**change):
            args = dict(classes=classes, cls=cls, lo=lo, hi=hi, sig_elem=sig_elem, nb=nb, na=na)
            args.update(change)
            s = h.clsigOpen(args["classes"], args["cls"], args["lo"], args["hi"], args["sig_elem"], args["nb"], args["na"], check=False)
            return s.status, s.bad

        def put(a, k, v):
            a = a.copy()
            a[k] = v
            return a

        assert refused() == (0, 0)
        h.readPatternFromMemory(b"keep\n")
        assert refused(lo=put(lo, 5, 3)) == (INVALID, 2)
        assert refused(lo=put(lo, 2, 0), hi=put(hi, 2, 0)) == (INVALID, 1)
        assert refused(hi=put(hi, 5, 65536)) == (INVALID, 2)
        assert refused(cls=put(cls, 4, classes.shape[0])) == (INVALID, 2)
        assert refused(nb=put(nb, 1, classes.shape[0])) == (INVALID, 2)
        assert refused(na=put(na, 0, -2)) == (INVALID, 1)
        assert refused(sig_elem=put(sig_elem, 1, 0)) == (INVALID, 1)
        assert refused(classes=put(classes, 0, 0)) == (INVALID, 0)
        assert refused(nb=None, na=None) == (0, 0), "both boundary arrays may be NULL"
        h.readPatternFromMemory(b"keep\n")
        lib, hnd = h._lib, h._h
        import ctypes as C
        s = C.c_void_p()
        p = lambda a: a.ctypes.data  # noqa: E731
        full = [p(classes.reshape(-1)), classes.shape[0], p(cls), p(lo), p(hi), p(sig_elem), None, None, 2, 0, 0, C.byref(s), None]
        for k in (0, 2, 3, 4, 5, 11):
            args = list(full)
            args[k] = None
            assert lib.PFACX_clsigOpen(hnd, *args) == INVALID, f"null argument {k}"
        for k, v in ((8, 0), (8, (1 << 31) - 1), (1, 0), (1, 65536)):
            args = list(full)
            args[k] = v
            assert lib.PFACX_clsigOpen(hnd, *args) == INVALID
        assert lib.PFACX_clsigOpen(None, *full) == BAD_HANDLE
        assert h.match_host_array(np.frombuffer(b"keep", dtype=np.uint8))[0] == 1, "a refused open call changed the handle's set"
        # the last that pass: 64 parts, slack 63, a literal part of 65 535 bytes, hi = 65 535
        parts64 = ([(frozenset(b"a"), 1, 1), (digits, 1, 1)] * 32, None, None)
        slack63 = _sig((b"a", 1, 1), (digits, 0, 31), (b"b", 1, 1), (digits, 0, 32))
        long_lit = _sig((b"a", 65534, 65534), (b"b", 1, 1), (digits, 1, 1))
        with h.clsigOpen(*ref.csr_of([parts64, slack63, long_lit])) as sg:
            assert sg.status == 0 and sg.anchors()[3].tolist() == [0, 1, 1, 32]
            st, got, _ = host_clsig(sg, b"x" + b"a" * 65534 + b"b7")
            assert [g.tolist() for g in got] == [[1, 65534], [3, 2], [65537, 65537]]     # the last a, b and 7 are signature 2 as well
        with h.clsigOpen(*ref.csr_of([_sig((b"k", 1, 1), (b"ab", 65535, 65535))])) as sg:
            assert host_clsig(sg, b"k" + b"a" * 65535)[1][2].tolist() == [65536] and host_clsig(sg, b"k" + b"a" * 65534)[2] == 0
    finally:
        h.destroy()


def test_special_cases_equal_the_sig_and_gapsig_calls():
    from tests import gapsig_ref, sig_ref
    h = host_handle()
    try:
        lines = ["61 62 63", "4D 5A 00 00 50 45", "61 2E 63"]
        data = b"abc abd MZ\0\0PE abc a.c"
        with h.sigOpenText(sig_ref.text_of(lines)) as sg:
            pos, ids = sg.match_host_array(np.frombuffer(data, dtype=np.uint8))
        with h.clsigOpenText(ref.text_of(next(c for c in ref.CASES if c[0] == "one-literal-part")[1])) as cs:
            got = host_clsig(cs, data)[1]
        lens = [0, 3, 6, 3]
        assert pos.size >= 4
        ref.same(got, (pos, ids, [int(p) + lens[int(i)] for p, i in zip(pos, ids)]), "one literal part against PFACX_sig*")
        # full classes (??), nibble classes (5?, ?A) and gaps: the same set through PFACX_gapsig* and PFACX_clsig* with SHORTEST_END, as sets
        gap_lines = ["4D 5A {2-6} 50 45 00", "E8 ?? ?? [0-8] 5? C3", "61 62 {0-3} ?A 63 64 {1-2} 65"]
        cls_lines = ["MZ.{2,6}PE\\x00", "\\xe8..{2}.{0,8}[P-_]\\xc3", "ab.{0,3}[\\x0a\\x1a*:JZjz\\x8a\\x9a\\xaa\\xba\\xca\\xda\\xea\\xfa]cd.{1,2}e"]
        cls_lines[1] = "\\xe8.{2}.{0,8}[P-_]\\xc3"
        rng = np.random.default_rng(11)
        data = rng.integers(0, 256, 3000, dtype=np.uint8)
        gsigs = gapsig_ref.parse_lines(gap_lines)
        gapsig_ref.embed(gsigs, data, 5, per_sig=6)
        with h.gapsigOpenText(gapsig_ref.text_of(gap_lines)) as gs:
            gpos, gids, gend = gs.match_host_array(data)
        with h.clsigOpenText(ref.text_of(cls_lines), 0, ref.SHORTEST) as cs:
            cpos, cids, cend = cs.match_host_array(data)
        assert gpos.size >= 12
        assert sorted(zip(gids.tolist(), gpos.tolist(), gend.tolist())) == sorted(zip(cids.tolist(), cpos.tolist(), cend.tolist()))
    finally:
        h.destroy()


def test_status_rows_the_getter_and_the_stale_object():
    h = host_handle()
    buf = np.frombuffer(b"ab12cd", dtype=np.uint8).copy()
    out = np.zeros(8, dtype=np.int32)
    try:
        sg = h.clsigOpenText(b"ab[0-9]{0,3}cd\n")
        args = (out.ctypes.data, out.ctypes.data, out.ctypes.data)
        assert sg.match_host(buf.ctypes.data, 0, None, None, None, 0) == (0, 0)
        assert sg.match_host(None, 6, *args, 8, check=False)[0] == INVALID
        assert sg.match_host(buf.ctypes.data, 1 << 31, *args, 8, check=False)[0] == INVALID
        assert sg.match_host(buf.ctypes.data, 6, None, None, None, 1, check=False)[0] == INVALID
        assert sg.match_host(buf.ctypes.data, 6, None, None, None, 0, check=False) == (TRUNCATED, 1)
        assert sg.match_device(buf.ctypes.data, 6, *args, 8, check=False)[0] == NOT_EXIST
        assert sg.pairs_device(buf.ctypes.data, 6, out.ctypes.data, out.ctypes.data, 1, None, None, None, 0, check=False)[0] == NOT_EXIST
        assert sg._lib.PFACX_clsigGetAnchors(sg._c, None, None, None, None, 1) == INVALID
        assert sg._lib.PFACX_clsigGetAnchors(sg._c, None, None, None, None, 2) == 0
        one = np.full(2, -7, dtype=np.int32)
        assert sg._lib.PFACX_clsigGetAnchors(sg._c, None, one.ctypes.data, None, None, 2) == 0 and one.tolist() == [0, 0]
        assert sg._lib.PFACX_clsigGetAnchors(None, None, None, None, None, 2) == BAD_HANDLE
        assert sg._lib.PFACX_clsigMatchFromHost(None, buf.ctypes.data, 6, None, None, None, 0, None) == BAD_HANDLE
        before = h.info().deviceTableBytes
        h.readPatternFromMemory(b"other\n")                       # the object goes stale
        assert sg.match_host(buf.ctypes.data, 6, None, None, None, 0, check=False)[0] == INVALID
        assert sg._lib.PFACX_clsigGetAnchors(sg._c, None, None, None, None, 2) == INVALID
        assert h.info().deviceTableBytes == before
        assert sg.close() == 0
        left = h.clsigOpenText(b"ab[0-9]{0,3}cd\n")              # PFAC_destroy closes what is left open
        assert left.status == 0
    finally:
        h.destroy()


def test_200_random_signatures_over_64_kib():
    sigs, data = ref.random_case()
    assert all(ref.check_limits(s) is None for s in sigs)
    h = host_handle(api.PFAC_PLATFORM_CPU_OMP)
    try:
        with h.clsigOpen(*ref.csr_of(sigs)) as sg:
            anchors = check_getter(h, sg, sigs)
            want, figures = ref.fast_list(sigs, data, anchors)
            print(figures)
            assert figures["entries"] >= 400 and figures["late_owner"] >= 5 and figures["multi_start"] >= 5, figures
            for i in (1, 50, 120, 200):
                got = ref.ends_by_sets(sigs[i - 1], data)
                assert sorted(got) == sorted(int(p) for p, j in zip(want[0], want[1]) if j == i), f"signature {i}: every start of the input"
            st, got, total = host_clsig(sg, data)
            assert st == 0
            ref.same(got, want, "the random case")
    finally:
        h.destroy()
