"""The four kinds of object a caller opens on a handle -- streams, flow sets, rule sets, group tables -- side by side on ONE handle: they share
the handle's registry, its close and its generation rule (pfac_host.h: HandleObject).  Host-only handles on the CPU platform: no device needed.
Every answer is checked against the references of the kinds' own tests (stream_ref, flows_ref, rules_ref, groups_ref)."""

import ctypes as C

import numpy as np

from pfac_amd import api
from tests import flows_ref as fr
from tests import groups_ref as gr
from tests import rules_ref as rr
from tests import stream_ref as sr
from tests.spans_helpers import pattern_file

INVALID, NOT_READY = api.STATUS.INVALID_PARAMETER, api.STATUS.PATTERNS_NOT_READY

PATS = [b"ab", b"abc", b"cd"]
OTHER = [b"cd", b"dab", b"x"]                        # the set that replaces it: as many patterns, other answers
DATA = np.frombuffer(b"xabcd ab cd\nabcab cdab x\ncdabc", dtype=np.uint8)
OFFSETS = [0, 12, 25, 30]                            # the segments of the rules and groups calls: the three lines
RULES = [[1], [2, 3], [3]]
MASKS = [0, 1, 2, 4]
SEG_MASKS = [7, 2, 5]


def host_handle(pf):
    h = api.PFAC.createHostOnly()
    h.setPlatform(api.PFAC_PLATFORM_CPU)
    h.readPatternFromFile(pf)
    return h


class References:
    """what every kind must answer over DATA on the set of `pats`, computed once"""

    def __init__(self, workdir, name, pats):
        self.pf = pattern_file(workdir, name, pats)
        pos, ids = sr.full_list(self.pf, DATA)
        assert pos.size >= 5, "an input that matches nothing checks nothing"
        self.M = int(sr.pattern_lengths(self.pf).max())
        self.stream = sr.split(pos, ids, [DATA.size], self.M)                 # one piece, then the flush
        self.flows = fr.build(self.pf, DATA, 2, 7, whole=True, big=False, sizes_of=lambda n, *_: [n])      # two flows, one piece each, one batch
        self.rules = rr.fired_py(pats, RULES, DATA.tobytes(), OFFSETS)
        self.groups = gr.groups_ref(pats, MASKS, DATA.tobytes(), OFFSETS, SEG_MASKS, True)
        assert self.rules[0].size and self.groups[0].size


def use(obj, ref, what):
    """one use of an open object, with the answer the reference gives"""
    if isinstance(obj, api.Stream):
        calls, flush = ref.stream
        sr.run(lambda off, size: obj.match_host_array(DATA[off:off + size]), obj.flush_host_array, DATA, [DATA.size], calls, flush, what)
    elif isinstance(obj, api.Flows):
        fr.run(ref.flows, lambda b: obj.match_host_array(b.buf, b.offsets, b.flows)[1:], lambda f: obj.flush_host_array(f)[1:], obj.reset, what)
    elif isinstance(obj, api.Rules):
        rr.same(obj.match_host_array(DATA, OFFSETS), ref.rules, what)
    else:
        gr.same(obj.match_host_array(DATA, OFFSETS, SEG_MASKS, True), ref.groups, what)


def refused(obj):
    """the statuses of every match and flush call of an object"""
    ids, pos = (np.zeros(DATA.size + 8, dtype=np.int32) for _ in range(2))
    buf = DATA.copy()
    off = np.array(OFFSETS, dtype=np.uintp)
    if isinstance(obj, api.Stream):
        return [obj.match_host(buf.ctypes.data, buf.size, ids.ctypes.data, pos.ctypes.data, ids.size, check=False)[0],
                obj.flush(ids.ctypes.data, pos.ctypes.data, ids.size, check=False)[0]]
    if isinstance(obj, api.Flows):
        return [obj.match_host_array(buf, [0, buf.size], [0], check=False)[0], obj.flush_host_array([0, 1], check=False)[0]]
    if isinstance(obj, api.Rules):
        return [obj.match_host(buf.ctypes.data, buf.size, off.ctypes.data, 3, ids.ctypes.data, pos.ctypes.data, ids.size, None, check=False)[0]]
    return [obj.match_host(buf.ctypes.data, buf.size, off.ctypes.data, 3, None, 0, ids.ctypes.data, pos.ctypes.data, ids.size, None, None, check=False)[0]]


def open_kind(h, kind):
    if kind == "stream":
        return h.streamOpen()
    if kind == "flows":
        return h.flowsOpen(2)
    if kind == "rules":
        return h.rulesOpen(*rr.csr(RULES))
    return h.groupsOpen(np.array(MASKS, dtype=np.uint64))


def test_mixed_kinds_on_one_handle(workdir):
    ref = References(workdir, "children_mixed", PATS)
    h = host_handle(ref.pf)
    table_bytes = h.info().deviceTableBytes
    order = ["stream", "rules", "flows", "groups", "rules", "stream", "groups", "flows"]
    objs = [open_kind(h, kind) for kind in order]
    assert h.info().deviceTableBytes == table_bytes
    for k, obj in enumerate(objs):
        use(obj, ref, f"object {k} ({order[k]})")
    for k in (3, 5, 1, 7):                             # neither the opening order nor its reverse; one of each kind
        assert objs[k].close() == 0
        assert h.info().deviceTableBytes == table_bytes
    for k in (0, 2, 4, 6):
        use(objs[k], ref, f"object {k} ({order[k]}), four others closed")
    assert h.info().deviceTableBytes == table_bytes      # nothing is on a device
    assert h.destroy() == 0                            # with four still open


def test_replacing_the_set(workdir):
    ref, other = References(workdir, "children_first", PATS), References(workdir, "children_other", OTHER)
    h = host_handle(ref.pf)
    try:
        objs = {kind: open_kind(h, kind) for kind in ("stream", "flows", "rules", "groups")}
        for kind, obj in objs.items():
            use(obj, ref, kind)
        h.readPatternFromFile(other.pf)
        for kind, obj in objs.items():
            assert refused(obj) == [INVALID] * (2 if kind in ("stream", "flows") else 1), kind
        assert objs["stream"].reset() == 0 and objs["flows"].reset() == 0      # (the whole-set form)
        use(objs["stream"], other, "the stream on the new set")
        use(objs["flows"], other, "the flow set on the new set")
        for kind in ("rules", "groups"):               # no reset: opened anew
            assert refused(objs[kind]) == [INVALID], kind
            assert objs[kind].close() == 0
            fresh = open_kind(h, kind)
            use(fresh, other, kind + " opened on the new set")
            assert fresh.close() == 0
    finally:
        assert h.destroy() == 0                        # with the stream and the flow set open


def test_no_set_loaded():
    h = api.PFAC.createHostOnly()
    try:
        lib, off, ids = h._lib, (C.c_int * 2)(0, 1), (C.c_int * 1)(1)
        member, masks = (C.c_uint * 4)(1, 0, 0, 0), (C.c_ulonglong * 2)(0, 1)      # one PFACX_rule_member_t: {1, 0, 0, 0}
        for name, args in (("PFACX_streamOpen", ()), ("PFACX_flowsOpen", (2,)), ("PFACX_rulesOpen", (off, ids, 1)), ("PFACX_rulesOpenEx", (off, member, 1)),
                           ("PFACX_groupsOpen", (masks, 2))):
            out = C.c_void_p(0xDEAD)
            assert getattr(lib, name)(h._h, *args, C.byref(out)) == NOT_READY, name
            assert not out.value, name + ": the out pointer is not null"
    finally:
        assert h.destroy() == 0
