"""The argument ladder of the six verify families -- PFACX_case*, sig*, approx*, gapsig*, edit*, clsig* and the clsigBatch* forms -- on a CPU-platform
handle (no device needed): for every family and each of its three forms the same bad arguments, one at a time with everything else valid, and the
status of each.  The three forms share one frame (pfac_amd/csrc/verify_calls.h); what this file pins is the ORDER of its checks: a device form on
such a handle answers LIB_NOT_EXIST only behind every argument refusal and in front of the generation check and the empty exits, a host form
checks the generation in front of its size == 0 exit.  No refusal may touch the place for the length.  (A closed object is freed memory: only the
stale object -- the set replaced under it -- is walked.)
What a CPU-platform handle cannot show is the order INSIDE the lock of the device forms, which LIB_NOT_EXIST hides: the generation against the
size == 0 and numPairs == 0 exits, and the all-zero segFirst that clsigBatch leaves for an empty list.  This file does not pin that order; the GPU
suites of the families (tests/test_*_gpu.py: stale objects, empty inputs, empty lists) are its only guard."""

import ctypes as C

import numpy as np
import pytest

from pfac_amd import api

OK, INVALID, NOT_EXIST, TRUNCATED, BAD_HANDLE = (0, api.STATUS.INVALID_PARAMETER, api.STATUS.LIB_NOT_EXIST, api.STATUS.OUTPUT_TRUNCATED,
                                                 api.STATUS.INVALID_HANDLE)
POISON = 2 ** 64 - 7
TEXT = b"xxabcdefghxxabcdefghxx"          # every family's one pattern occurs twice, exactly


def open_case(h):
    h.readPatternFromMemoryEx(b"abcdefgh\n", api.PFACX_READ_NOCASE)
    return h.caseOpen(b"abcdefgh\n", [0, 1])


# name -> (the call prefix, open(handle), the arguments between size and the lists, the aux output arrays, segFirst behind the capacity?)
FAMILIES = {
    "case": ("PFACX_case", open_case, "flags", 0, False),
    "sig": ("PFACX_sig", lambda h: h.sigOpenText(b"61 62 63 64 65 66 67 68\n"), "", 0, False),
    "approx": ("PFACX_approx", lambda h: h.approxOpen([b"abcdefgh"], [1]), "", 1, False),
    "gapsig": ("PFACX_gapsig", lambda h: h.gapsigOpenText(b"61 62 63 64 {0-2} 67 68\n"), "", 1, False),
    "edit": ("PFACX_edit", lambda h: h.editOpen([b"abcdefgh"], [1]), "", 2, False),
    "clsig": ("PFACX_clsig", lambda h: h.clsigOpenText(b"abcd[e-f]{1,3}gh\n"), "", 1, False),
    "clsigBatch": ("PFACX_clsigBatch", lambda h: h.clsigOpenText(b"abcd[e-f]{1,3}gh\n"), "offsets", 1, True),
}
FORMS = ("MatchFromDevice", "MatchFromHost", "PairsFromDevice")


class Call:
    """one form of one family over valid arguments, any of which a rung replaces"""

    def __init__(self, family, form, obj):
        prefix, _, self.pre, self.aux, self.seg_first = FAMILIES[family]
        self.fn = getattr(obj._lib, prefix + form)
        self.pairs = form == "PairsFromDevice"
        self.buf = np.frombuffer(TEXT, dtype=np.uint8).copy()
        self.out = [np.full(64, -7, dtype=np.int32) for _ in range(2 + self.aux)]
        self.pair_arrays = [np.array([1, 1], dtype=np.int32), np.array([2, 12], dtype=np.int32)]
        self.offsets = np.array([0, 11, len(TEXT)], dtype=np.uint64)
        self.first = np.full(3, POISON, dtype=np.uint64)
        self.valid = dict(obj=obj._c, input=self.buf.ctypes.data, size=self.buf.size, flags=0, offsets=self.offsets.ctypes.data, segments=2,
                          pair_ids=self.pair_arrays[0].ctypes.data, pair_pos=self.pair_arrays[1].ctypes.data, num_pairs=2,
                          outs=[a.ctypes.data for a in self.out], capacity=64, seg_first=self.first.ctypes.data, count=True)

    def __call__(self, **changed):
        a = dict(self.valid, **changed)
        n = C.c_size_t(POISON)
        args = [a["obj"], a["input"], a["size"]]
        args += [a["flags"]] if self.pre == "flags" else [a["offsets"], a["segments"]] if self.pre == "offsets" else []
        args += [a["pair_ids"], a["pair_pos"], a["num_pairs"]] if self.pairs else []
        args += list(a["outs"]) + [a["capacity"]] + ([a["seg_first"]] if self.seg_first else []) + [C.byref(n) if a["count"] else None]
        return self.fn(*args), n.value

    def nulled(self, i):
        outs = list(self.valid["outs"])
        outs[i] = None
        return outs


@pytest.fixture(params=list(FAMILIES))
def opened(request):
    h = api.PFAC.createHostOnly()
    h.setPlatform(api.PFAC_PLATFORM_CPU)
    obj = FAMILIES[request.param][1](h)
    yield request.param, h, obj
    h.destroy()


def refusals(call):
    """the rungs every form shares -> [(what, arguments, status)]"""
    rungs = [("null object", dict(obj=None), BAD_HANDLE),
             ("null object wins over a null input", dict(obj=None, input=None), BAD_HANDLE),
             ("null input", dict(input=None), INVALID),
             ("null count pointer", dict(count=False), INVALID),
             ("size > 2^31 - 1", dict(size=1 << 31, capacity=1 << 31), INVALID),
             ("null ids with a capacity", dict(outs=call.nulled(0)), INVALID),
             ("null pos with a capacity", dict(outs=call.nulled(1)), INVALID)]
    if call.pre == "flags":
        rungs.append(("an unknown flag", dict(flags=2), INVALID))
    if call.pre == "offsets":
        rungs += [("null offsets", dict(offsets=None), INVALID), ("no segment for bytes", dict(segments=0), INVALID),
                  ("2^31 - 1 segments", dict(segments=2 ** 31 - 1), INVALID)]
    return rungs


@pytest.mark.parametrize("form", FORMS)
def test_the_ladder_of_bad_arguments(opened, form):
    family, h, obj = opened
    call = Call(family, form, obj)
    device = form != "MatchFromHost"
    for what, args, want in refusals(call):
        assert call(**args) == (want, POISON), f"{family} {form}: {what}"
    no_outs = [None] * (2 + call.aux)
    if form == "MatchFromDevice":
        # the device form wants its arrays whatever the capacity, and capacity >= size; behind every refusal: no module on this handle
        assert call(outs=no_outs, capacity=0, size=0) == (INVALID, POISON), "null arrays, nothing to write"
        assert call(capacity=call.buf.size - 1) == (INVALID, POISON), "capacity < size"
        assert call() == (NOT_EXIST, POISON)
        assert call(size=0) == (NOT_EXIST, POISON), "size == 0 is looked at behind the module"
        assert call(size=0, capacity=0) == (NOT_EXIST, POISON)
        for i in range(2, 2 + call.aux):
            assert call(outs=call.nulled(i)) == (NOT_EXIST, POISON), "an aux array may be null"
    elif form == "PairsFromDevice":
        ids, pos = call.pair_arrays[0].ctypes.data, call.pair_arrays[1].ctypes.data
        assert call(num_pairs=1 << 31) == (INVALID, POISON), "numPairs > 2^31 - 1"
        assert call(capacity=(1 << 62) + 1) == (INVALID, POISON), "a capacity whose bytes overflow"
        assert call(pair_ids=None) == (INVALID, POISON) and call(pair_pos=None) == (INVALID, POISON)
        for i in range(2 + call.aux):                        # every output array against both pair arrays
            for pair in (ids, pos):
                outs = list(call.valid["outs"])
                outs[i] = pair + 4
                assert call(outs=outs, capacity=2) == (INVALID, POISON), f"{family}: output {i} overlaps a pair array"
        outs = list(call.valid["outs"])
        outs[0] = ids + 8
        assert call(outs=outs, capacity=2) == (NOT_EXIST, POISON), "behind the pair arrays: no overlap"
        outs[0] = ids
        assert call(outs=outs, capacity=0) == (NOT_EXIST, POISON) and call(outs=outs, num_pairs=0) == (NOT_EXIST, POISON), "nothing written or read"
        assert call() == (NOT_EXIST, POISON)
        assert call(outs=no_outs, capacity=0) == (NOT_EXIST, POISON), "a count query"
        assert call(pair_ids=None, pair_pos=None, num_pairs=0) == (NOT_EXIST, POISON), "numPairs == 0 is looked at behind the module"
        assert call(size=0) == (NOT_EXIST, POISON), "size == 0 too"
        for i in range(2, 2 + call.aux):
            assert call(outs=call.nulled(i)) == (NOT_EXIST, POISON), "an aux array may be null"
    else:
        st, total = call()
        assert st == OK and total >= 2, "both occurrences"
        assert call(outs=no_outs, capacity=0) == (TRUNCATED, total), "a count query"
        assert call(capacity=1) == (TRUNCATED, total)
        for i in range(2, 2 + call.aux):
            assert call(outs=call.nulled(i)) == (OK, total), "an aux array may be null"
        assert call(size=0) == (OK, 0) and call(size=0, outs=no_outs, capacity=0) == (OK, 0)
        if call.pre == "offsets":
            assert call(size=0, segments=0) == (OK, 0), "no segment for no bytes"
            bad = np.array([0, 12, 11], dtype=np.uint64)
            assert call(offsets=bad.ctypes.data) == (INVALID, POISON), "offsets that descend"
            assert call(offsets=bad.ctypes.data, size=0) == (OK, 0), "... are not looked at for no bytes"
    # the stale object: the set replaced under it
    h.readPatternFromMemory(b"other\n")
    if device:
        assert call() == (NOT_EXIST, POISON), "the module is asked for in front of the generation"
        assert call(input=None) == (INVALID, POISON), "... behind the arguments"
    else:
        assert call() == (INVALID, POISON)
        assert call(size=0) == (INVALID, POISON), "the generation is checked in front of the size == 0 exit"
        assert call(input=None) == (INVALID, POISON) and call(obj=None) == (BAD_HANDLE, POISON)
    assert obj.close() == 0
