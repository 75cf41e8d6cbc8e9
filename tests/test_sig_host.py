"""PFACX_sigOpen / PFACX_sigOpenText / PFACX_sigGetAnchors / PFACX_sigMatchFromHost on the CPU platforms (host-only handles: no device needed)
against the models of tests/sig_ref.py: the parser's accepts and refusals with badLine and badSig, the canonical values, the anchor choice
(leftmost longest, the maxAnchorLen cut, 0x0A excluded, refused without a candidate), the getter against the handle's own pattern list, every
case of the table through both open calls, every capacity from 0 to the list's length, the status rows, the stale object, the SigSet wrapper, and
the bounds of the seeded random case the GPU file runs."""

import ctypes as C

import numpy as np
import pytest

from pfac_amd import api
from tests import sig_ref as ref
from tests.sig_ref import test_the_models_agree_on_every_case  # noqa: F401  (runs here: sig_ref.py is not collected)

PLATFORMS = [(api.PFAC_PLATFORM_CPU, "cpu"), (api.PFAC_PLATFORM_CPU_OMP, "cpu-omp")]
INVALID, NOT_EXIST, TRUNCATED, BAD_HANDLE = (api.STATUS.INVALID_PARAMETER, api.STATUS.LIB_NOT_EXIST, api.STATUS.OUTPUT_TRUNCATED,
                                             api.STATUS.INVALID_HANDLE)
GUARD = 16


def host_handle(platform=api.PFAC_PLATFORM_CPU):
    h = api.PFAC.createHostOnly()
    h.setPlatform(platform)
    return h


def host_sig(sg, data, capacity=None):
    """match_host into poisoned arrays of `capacity` entries (default: the full length, asked for first) with GUARD poisoned ints on both sides
    -> (status, (pos, ids) of the entries written, the full length); nothing outside the written entries may change, nor the input"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    n = buf.size
    if capacity is None:
        st, capacity = sg.match_host(buf.ctypes.data, n, None, None, 0, check=False)
        assert st in (0, TRUNCATED) and (st == TRUNCATED) == (capacity > 0)
    ids, pos = (np.full(GUARD + capacity + GUARD, -7, dtype=np.int32) for _ in range(2))
    st, total = sg.match_host(buf.ctypes.data, n, ids.ctypes.data + 4 * GUARD, pos.ctypes.data + 4 * GUARD, capacity, check=False)
    assert st in (0, TRUNCATED) and (st == TRUNCATED) == (total > capacity)
    k = min(total, capacity)
    for a in (ids, pos):
        assert np.all(a[:GUARD] == -7) and np.all(a[GUARD + capacity:] == -7), "wrote outside the arrays"
        assert np.all(a[GUARD + k:GUARD + capacity] == -7), "wrote behind the list"
    assert buf.tobytes() == bytes(data), "the caller's input was modified"
    return st, (pos[GUARD:GUARD + k].copy(), ids[GUARD:GUARD + k].copy()), total


def check_getter(h, sg, sigs, max_len=0):
    """the getter equals the documented rule, and handle id q IS the q-th distinct anchor: the handle finds each anchor under that id"""
    got = sg.anchors()
    want, anchors = ref.model_anchors(sigs, max_len)
    for g, w, what in zip(got, want, ("anchor id", "anchor offset", "anchor length")):
        assert g.tolist() == w.tolist(), what
    for q, anchor in enumerate(anchors, start=1):
        found = h.match_host_array(np.frombuffer(anchor, dtype=np.uint8))
        assert int(found[0]) == q, f"the handle's pattern {q} is not the {q}-th distinct anchor"
    assert h.caseInsensitive() == 0
    return got


@pytest.mark.parametrize("platform,pname", PLATFORMS)
@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_every_case_equals_the_models(case, platform, pname):
    name, data = case[0], case[2]
    lines = ref.case_lines(case)
    sigs = ref.parse_lines(lines)
    h = host_handle(platform)
    try:
        with h.sigOpenText(ref.text_of(lines)) as sg:
            assert sg.status == 0 and sg.bad == 0 and sg.num_sigs == len(sigs)
            _, off, length = check_getter(h, sg, sigs)
            want = ref.check_models(sigs, data, off, length, name)
            st, got, total = host_sig(sg, data)
            assert st == 0 and total == want[0].size
            ref.same(got, want, f"{name}/{pname}/text")
            if name in ref.WANT:
                ids, pos = ref.WANT[name]
                ref.same(got, (pos, ids), f"{name}/{pname}: against the list worked out by hand")
            ref.same(sg.match_host_array(np.frombuffer(data, dtype=np.uint8)), want, f"{name}/match_host_array")
        with h.sigOpen(*ref.csr_of(sigs)) as sg:                   # the binary form: the same object
            assert [a.tolist() for a in sg.anchors()] == [a.tolist() for a in ref.model_anchors(sigs)[0]]
            ref.same(host_sig(sg, data)[1], want, f"{name}/{pname}/binary")
    finally:
        h.destroy()


def test_every_capacity_from_zero_to_the_length():
    case = next(c for c in ref.CASES if c[0] == "an-anchor-is-a-prefix-of-another")
    sigs = ref.parse_lines(case[1])
    h = host_handle()
    try:
        with h.sigOpenText(ref.text_of(case[1])) as sg:
            _, off, length = sg.anchors()
            want = ref.check_models(sigs, case[2], off, length, case[0])
            total = int(want[0].size)
            assert total > 2
            for cap in (0, 1, total - 1, total, total + 3):
                st, got, n = host_sig(sg, case[2], capacity=cap)
                assert (st, n) == (TRUNCATED if cap < total else 0, total)
                ref.same(got, (want[0][:cap], want[1][:cap]), f"capacity {cap}")
    finally:
        h.destroy()


def test_the_parser_accepts_every_form():
    h = host_handle()
    try:
        text = b"4d5A\n 4D\t5a  \r\n??4d 5?\t?a 41\n4D 5A\r\n"
        with h.sigOpenText(text) as sg:
            assert sg.num_sigs == 4
            ids, off, length = sg.anchors()
            assert ids.tolist() == [0, 1, 1, 2, 1] and off.tolist() == [0, 0, 0, 1, 0] and length.tolist() == [0, 2, 2, 1, 2]
            # line 3 is ?? 4D 5? ?A 41: the half bytes admit 16 values each
            pos, got = sg.match_host_array(np.frombuffer(b"xM\x5f\x7aA xM\x6f\x7aA xM\x5f\x7bA", dtype=np.uint8))
            assert (got.tolist(), pos.tolist()) == ([3], [0])
    finally:
        h.destroy()


@pytest.mark.parametrize("text,line,why", [
    (b"41\n\n42\n", 2, "an empty line"),
    (b"41\n  \t\n", 2, "a line of blanks"),
    (b"41\n\r\n", 2, "a line of one carriage return"),
    (b"41 4\n", 1, "an odd digit at the end"),
    (b"41\n4 1\n", 2, "a blank inside a pair"),
    (b"414 2\n", 1, "an odd digit in front of a blank"),
    (b"41\n42\n4G\n", 3, "another character"),
    (b"41,42\n", 1, "a comma"),
    (b"41\r 42\n", 1, "a carriage return that is not in front of the newline"),
    (b"41\n?\n", 2, "one question mark"),
    (b"41\n42", 2, "bytes behind the last newline"),
    (b"41\n42\n ", 3, "a blank behind the last newline"),
    (b"41\n??\n", 2, "a signature without a fully specified byte"),
    (b"41\n4? ?1\n", 2, "only half bytes"),
    (b"0A\n", 1, "the only fully specified byte is 0x0A"),
    (b"41\n?? 0A 0a ??\n", 2, "only newlines and wildcards"),
])
def test_the_parser_refuses_with_the_line(text, line, why):
    h = host_handle()
    try:
        h.readPatternFromMemory(b"kept\n")
        sg = h.sigOpenText(text, check=False)
        assert (sg.status, sg.bad) == (INVALID, line), why
        assert not sg._c, "no object behind a refusal"
        assert int(h.match_host_array(np.frombuffer(b"kept", dtype=np.uint8))[0]) == 1, "a refusal leaves the handle's set alone"
    finally:
        h.destroy()


def test_the_binary_form_refuses_with_the_signature():
    lib = api.load_library()
    h = host_handle()
    try:
        def refused(values, masks, off):
            sg = h.sigOpen(values, masks, off, check=False)
            assert not sg._c
            return sg.status, sg.bad
        ff = lambda n: [0xFF] * n  # noqa: E731
        assert refused([1, 2, 3], ff(3), [0, 1, 1, 3]) == (INVALID, 2), "an offset that does not ascend: an empty signature"
        assert refused([1, 2, 3], ff(3), [0, 2, 1, 3]) == (INVALID, 2), "an offset that descends"
        assert refused([1, 2, 3], [0xFF, 0xF0, 0xFF], [0, 1, 2, 3]) == (INVALID, 2), "no fully specified byte"
        assert refused([1, 0x0A, 3], ff(3), [0, 1, 2, 3]) == (INVALID, 2), "the only fully specified byte is 0x0A"
        long = np.full(65536, 0x41, dtype=np.uint8)
        assert refused(np.concatenate([[1], long]), np.full(65537, 0xFF, np.uint8), [0, 1, 65537]) == (INVALID, 2), "65 536 bytes"
        with h.sigOpen(long[:65535], np.full(65535, 0xFF, np.uint8), [0, 65535]) as sg:
            assert sg.anchors()[2].tolist() == [0, 32], "65 535 bytes are fine"
        v, m, off = (np.array(a) for a in ([0x41], [0xFF], [0, 1]))
        v, m, off = v.astype(np.uint8), m.astype(np.uint8), off.astype(np.uint64)
        s, bad = C.c_void_p(), C.c_int(-1)
        args = lambda **kw: [kw.get("h", h._h), kw.get("v", v.ctypes.data), kw.get("m", m.ctypes.data), kw.get("off", off.ctypes.data),  # noqa: E731
                             kw.get("n", 1), 0, kw.get("s", C.byref(s)), kw.get("bad", C.byref(bad))]
        assert lib.PFACX_sigOpen(*args(h=None)) == BAD_HANDLE
        for null in ("v", "m", "off", "s"):
            assert lib.PFACX_sigOpen(*args(**{null: None})) == INVALID, null
        assert lib.PFACX_sigOpen(*args(n=0)) == INVALID and bad.value == 0, "numSigs == 0"
        assert lib.PFACX_sigOpen(*args(bad=None)) == 0 and s.value, "badSig may be null"
        assert lib.PFACX_sigClose(s) == 0
        assert lib.PFACX_sigOpenText(h._h, None, 0, 0, C.byref(s), C.byref(bad)) == INVALID
        assert lib.PFACX_sigOpenText(h._h, b"", 0, 0, C.byref(s), C.byref(bad)) == INVALID and bad.value == 0, "no line at all"
        assert lib.PFACX_sigOpenText(h._h, b"41\n", 3, 0, None, C.byref(bad)) == INVALID
        assert lib.PFACX_sigOpenText(None, b"41\n", 3, 0, C.byref(s), C.byref(bad)) == BAD_HANDLE
        assert lib.PFACX_sigOpenText(h._h, b"41\n4\n", 5, 0, C.byref(s), None) == INVALID, "badLine may be null"
    finally:
        h.destroy()


def test_values_are_canonicalised():
    """v &= m: the bits of a value outside its mask mean nothing, in the compare and in the anchor"""
    h = host_handle()
    try:
        data = b"xM\x5f\x7aA M\x50\x0aA"
        masks = [0x00, 0xFF, 0xF0, 0x0F, 0xFF]
        with h.sigOpen([0x00, 0x4D, 0x50, 0x0A, 0x41], masks, [0, 5]) as sg:
            want = host_sig(sg, data)[1]
            anchors = [a.tolist() for a in sg.anchors()]
        with h.sigOpen([0xAB, 0x4D, 0x5C, 0xEA, 0x41], masks, [0, 5]) as sg:
            ref.same(host_sig(sg, data)[1], want, "the same signature with stray bits")
            assert [a.tolist() for a in sg.anchors()] == anchors
        assert want[0].tolist() == [0, 5], "the second one has 0x0A under its half byte"
        # a stray 0x0A under a half mask is no newline, and a masked-out byte that reads 0x0A is no anchor byte either
        with h.sigOpen([0x0A, 0x41], [0x0F, 0xFF], [0, 2]) as sg:
            assert sg.anchors()[1].tolist() == [0, 1]
    finally:
        h.destroy()


@pytest.mark.parametrize("line,max_len,want", [
    ("61 62 ?? 63 64", 0, (0, 2)),                      # equal runs: the leftmost
    ("61 ?? 62 63 ?? 64 65 66 ?? 67 68 69", 0, (5, 3)),  # the longest, the leftmost of the two longest
    ("?? 61 62 63 64 65", 3, (1, 3)),                   # cut to its FIRST maxAnchorLen bytes
    ("61 62 ?? 63 64 65 66", 2, (3, 2)),                # the cut comes after the choice: the longer run wins, then it is cut
    ("61 62 63 0A 64 65", 0, (0, 3)),                   # 0x0A ends a run
    ("0A 61 0A 0A 62 63", 0, (4, 2)),
    ("6? 61 ?2 62", 0, (1, 1)),
    (" ".join(["41"] * 40), 0, (0, 32)),                # the default cut
    (" ".join(["41"] * 40), 33, (0, 33)),
    (" ".join(["41"] * 40), 100, (0, 40)),
])
def test_the_anchor_choice(line, max_len, want):
    assert ref.choose_anchor(*ref.parse_line(line.encode()), max_len) == want, "the model of the rule"
    h = host_handle()
    try:
        with h.sigOpenText(ref.text_of([line]), max_len) as sg:
            ids, off, length = check_getter(h, sg, ref.parse_lines([line]), max_len)
            assert (int(ids[1]), int(off[1]), int(length[1])) == (1,) + want
    finally:
        h.destroy()


def test_distinct_anchors_take_ids_in_order_of_first_appearance():
    lines = ["62 63 ??", "?? 61 62", "62 63 ?? ??", "61 62", "63", "?? 62 63"]
    h = host_handle()
    try:
        with h.sigOpenText(ref.text_of(lines)) as sg:
            ids, _, _ = check_getter(h, sg, ref.parse_lines(lines))
            assert ids.tolist() == [0, 1, 2, 1, 2, 3, 1]
            lib = api.load_library()
            short = np.zeros(len(lines), dtype=np.int32)
            assert lib.PFACX_sigGetAnchors(sg._c, short.ctypes.data, None, None, len(lines)) == INVALID, "n < S + 1"
            only = np.full(len(lines) + 1, -7, dtype=np.int32)
            assert lib.PFACX_sigGetAnchors(sg._c, None, None, only.ctypes.data, len(lines) + 1) == 0 and only.tolist() == [0, 2, 2, 2, 2, 1, 2]
    finally:
        h.destroy()


def test_status_rows_and_the_stale_object():
    lib = api.load_library()
    h = host_handle()
    try:
        sg = h.sigOpenText(b"61 ?? 63\n")
        data = np.frombuffer(b"abc", dtype=np.uint8).copy()
        ids, pos = (np.full(4, -7, dtype=np.int32) for _ in range(2))
        n = C.c_size_t(99)
        call = lambda fn, size=3, cap=4, inp=data.ctypes.data, i=ids.ctypes.data, p=pos.ctypes.data, num=C.byref(n): fn(  # noqa: E731
            sg._c, inp, size, i, p, cap, num)
        assert call(lib.PFACX_sigMatchFromHost) == 0 and n.value == 1 and (ids[0], pos[0]) == (1, 0)
        assert call(lib.PFACX_sigMatchFromHost, size=0) == 0 and n.value == 0, "size == 0"
        assert call(lib.PFACX_sigMatchFromHost, size=1 << 31) == INVALID, "size >= 2^31"
        assert call(lib.PFACX_sigMatchFromHost, inp=None) == INVALID and call(lib.PFACX_sigMatchFromHost, num=None) == INVALID
        assert call(lib.PFACX_sigMatchFromHost, i=None) == INVALID and call(lib.PFACX_sigMatchFromHost, p=None) == INVALID
        assert call(lib.PFACX_sigMatchFromHost, cap=0, i=None, p=None) == TRUNCATED and n.value == 1, "the count query"
        assert call(lib.PFACX_sigMatchFromDevice) == NOT_EXIST, "a device form on a host-only handle"
        assert call(lib.PFACX_sigMatchFromDevice, cap=2) == INVALID, "capacity < size"
        assert lib.PFACX_sigPairsFromDevice(sg._c, data.ctypes.data, 3, ids.ctypes.data, pos.ctypes.data, 1, None, None, 0, C.byref(n)) == NOT_EXIST
        assert lib.PFACX_sigMatchFromHost(None, data.ctypes.data, 3, None, None, 0, C.byref(n)) == BAD_HANDLE
        # the handle reads another set: only the close call works
        h.readPatternFromMemory(b"a\n")
        assert call(lib.PFACX_sigMatchFromHost) == INVALID and call(lib.PFACX_sigMatchFromDevice) in (INVALID, NOT_EXIST)
        assert sg.anchors(check=False) and lib.PFACX_sigGetAnchors(sg._c, ids.ctypes.data, None, None, 4) == INVALID
        assert sg.close() == 0
        # a second open replaces the set of the first: the first object goes stale the same way
        first = h.sigOpenText(b"61\n")
        second = h.sigOpenText(b"62\n")
        assert first.match_host(data.ctypes.data, 3, None, None, 0, check=False)[0] == INVALID
        assert second.match_host(data.ctypes.data, 3, None, None, 0, check=False) == (TRUNCATED, 1)
        assert first.close() == 0 and second.close() == 0
        assert lib.PFACX_sigClose(None) == BAD_HANDLE
    finally:
        h.destroy()


def test_destroy_closes_the_object_and_the_handle_counts_no_device_tables():
    h = host_handle()
    sg = h.sigOpenText(b"61 ?? 63\n")
    assert h.info().deviceTableBytes == 0, "a host-only handle uploads nothing"
    h.destroy()
    sg._c = C.c_void_p()                                        # PFAC_destroy closed it


def test_the_seeded_random_case_is_inside_its_bounds():
    """the case tests/test_sig_gpu.py runs: the model alone yields at least 100 and at most 50 000 entries, and the host form equals it"""
    sigs, data = ref.random_case()
    assert len(sigs) == 200 and data.size == 1 << 16
    (_, off, length), anchors = ref.model_anchors(sigs)
    want = ref.check_models(sigs, data, off, length, "random")
    assert 100 <= want[0].size <= 50000, want[0].size
    h = host_handle(api.PFAC_PLATFORM_CPU_OMP)
    try:
        with h.sigOpen(*ref.csr_of(sigs)) as sg:
            check_getter(h, sg, sigs)
            ref.same(sg.match_host_array(data), want, "random/host")
    finally:
        h.destroy()
