"""The host forms on a GPU-platform handle whose pattern set is replaced by one with the SAME number of patterns: PFACX_matchAllFromHost,
countFromHost, matchWordsFromHost (both modes), matchSpansFromHost, matchDisjointFromHost, matchLinesFromHost and replaceFromHost.  Each takes its
longest pairs from hostLongestPairs, which on this platform reads the set's generation under the handle's lock, and runs its post-pass under a
SetPin on that generation (pfac_amd/csrc/pfac_host.h); every result equals that of a host-only CPU handle that holds the same set.  Set A has
chains of prefixes, set B none and other lengths per id: what a comparison of pattern counts could not tell apart.

The batch host forms -- PFACX_countBatchFromHost, PFACX_rulesMatchFromHost (a plain and a conditioned rule set) and PFACX_groupsMatchFromHost (both
modes) -- take the longest pairs of every segment from HostBatchPairs and pin the same way; here the input is cut into segments at its newlines,
and rule sets and group tables are opened anew on each set: one opened on the set before answers INVALID_PARAMETER."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfac_amd import api  # noqa: E402

SET_A = b"a\nab\nabc\nabcd\nhe\nhers\n"
SET_B = b"she\nhi\nbcda\nx\ndog\ncats\n"
NUM_IDS = 6
LINES = [b"abcd she sells hers, his dog and cats", b"x marks hi; abc ab a_b (he) hers_", b"one penny a piece", b"do cat abcda bcda shells", b"",
         b"x: 1 + 2 = 3", b"the dogs do chase cats: abcdabcd he she his", b"do it once more"]


def make_input():
    text, k = b"", 0
    while len(text) < 4096:
        text += LINES[k % len(LINES)] + b"\n"
        k += 1
    return np.frombuffer(text, dtype=np.uint8).copy()


def ptr(a):
    return a.ctypes.data


# rule r is RULES[RULE_OFF[r]:RULE_OFF[r + 1]]; the conditioned set: pattern 1 and no pattern 6; pattern 5 inside the last 12 bytes of the
# segment; pattern 2 inside its first 8 bytes and pattern 4 anywhere
RULE_OFF = [0, 1, 3, 5, 6]
RULES = [1, 2, 5, 3, 4, 6]
COND_OFF = [0, 2, 3, 5]
COND_MEMBERS = [(1, 0, 0, 0), (6, api.PFACX_RULE_NOT, 0, 0), (5, api.PFACX_RULE_FROM_END, 0, 12), (2, 0, 0, 8), (4, 0, 0, 0)]
PATTERN_MASKS = np.array([0, 1, 2, 4, 8, 16, 32], dtype=np.uint64)


def segments_of(data):
    """the offsets of the segments that end behind each newline (and at the end of the buffer)"""
    cuts = (np.flatnonzero(data == 10) + 1).tolist()
    return np.array([0] + cuts + ([int(data.size)] if cuts[-1] != data.size else []), dtype=np.uintp)


def rules_form(rules, data, off, cap):
    seg, rule = (np.full(cap, -5, dtype=np.int32) for _ in range(2))
    first = np.full(off.size, 0xDEAD, dtype=np.uintp)
    st, n = rules.match_host(ptr(data), int(data.size), ptr(off), off.size - 1, ptr(seg), ptr(rule), cap, ptr(first), check=False)
    return (st, n, seg[:n].copy(), rule[:n].copy(), first)


def groups_form(groups, data, off, seg_masks, flags, cap):
    ids, pos = (np.full(cap, -5, dtype=np.int32) for _ in range(2))
    first = np.full(off.size, 0xDEAD, dtype=np.uintp)
    hit = np.full(off.size - 1, 0xDEAD, dtype=np.uint64)
    st, n = groups.match_host(ptr(data), int(data.size), ptr(off), off.size - 1, ptr(seg_masks), flags, ptr(ids), ptr(pos), cap, ptr(first), ptr(hit),
                              check=False)
    return (st, n, ids[:n].copy(), pos[:n].copy(), first, hit)


def batch_forms(h, data, got):
    """... and the batch host forms over `data` cut at its newlines, rule sets and group tables opened on the set `h` holds now"""
    n = int(data.size)
    cap = 4 * n
    off = segments_of(data)
    segments = off.size - 1
    ids = np.full(cap, -5, dtype=np.int32)
    counts = np.full(cap, 77, dtype=np.uint32)
    first = np.full(segments + 1, 0xDEAD, dtype=np.uintp)
    st, entries, total = h.countBatchFromHost(ptr(data), n, ptr(off), segments, 0, ptr(ids), ptr(counts), cap, ptr(first))
    got["count_batch"] = (st, entries, total, ids[:entries].copy(), counts[:entries].copy(), first)
    for name, rules in (("rules", h.rulesOpen(RULE_OFF, RULES)), ("rules_cond", h.rulesOpenEx(COND_OFF, COND_MEMBERS))):
        got[name] = rules_form(rules, data, off, cap)
        rules.close()
    seg_masks = np.array([(k * 11 + 1) & 63 for k in range(segments)], dtype=np.uint64)       # every subset of the six bits, 0 included
    groups = h.groupsOpen(PATTERN_MASKS)
    for name, flags in (("groups_all", api.PFACX_GROUPS_ALL), ("groups", 0)):
        got[name] = groups_form(groups, data, off, seg_masks, flags, cap)
    groups.close()


BATCH_FORMS = ("count_batch", "rules", "rules_cond", "groups_all", "groups")


def every_form(h, data, tokens):
    """every host form over `data` -> {form: everything it wrote}; `tokens`: the (ids, pos) PFACX_replaceFromHost is given (None: this set's own
    disjoint list)"""
    n = int(data.size)
    cap = 4 * n
    a, b, c = (np.full(cap, -5, dtype=np.int32) for _ in range(3))
    got = {}
    st, total = h.matchAllFromHost(ptr(data), n, ptr(a), ptr(b), cap)
    got["all"] = (st, total, a[:total].copy(), b[:total].copy())
    counts = np.full(NUM_IDS + 1, 77, dtype=np.uint64)
    st, total = h.countFromHost(ptr(data), n, 0, ptr(counts), NUM_IDS + 1)
    got["count"] = (st, total, counts.copy())
    for name, flags in (("words", 0), ("words_all", api.PFACX_WORDS_ALL)):
        st, total = h.matchWordsFromHost(ptr(data), n, None, flags, ptr(a), ptr(b), cap)
        got[name] = (st, total, a[:total].copy(), b[:total].copy())
    st, ns, covered = h.matchSpansFromHost(ptr(data), n, ptr(a), ptr(b), cap)
    got["spans"] = (st, ns, covered, a[:ns].copy(), b[:ns].copy())
    st, nt, covered = h.matchDisjointFromHost(ptr(data), n, ptr(a), ptr(b), cap)
    got["disjoint"] = (st, nt, covered, a[:nt].copy(), b[:nt].copy())
    if tokens is None:
        tokens = (a[:nt].copy(), b[:nt].copy())
    st, nl, ns = h.matchLinesFromHost(ptr(data), n, 0, ptr(a), ptr(b), ptr(c), cap)
    got["lines"] = (st, nl, ns, a[:ns].copy(), b[:ns].copy(), c[:ns].copy())
    repl = [b"<%d>" % i for i in range(1, NUM_IDS + 1)]
    off = np.cumsum([0, 0] + [len(r) for r in repl]).astype(np.int32)          # ids 0 and F + 1 have offsets and no string
    blob = np.frombuffer(b"".join(repl), dtype=np.uint8).copy()
    out = np.full(8 * n, 0xEE, dtype=np.uint8)
    ids, pos = (np.ascontiguousarray(t, dtype=np.int32) for t in tokens)
    st, total = h.replaceFromHost(ptr(data), n, ptr(ids), ptr(pos), int(ids.size), ptr(off), int(off.size), ptr(blob), int(blob.size), ptr(out), int(out.size))
    got["replace"] = (st, total, out[:total].copy())
    batch_forms(h, data, got)
    return got, tokens


def same(x, y):
    return len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y))


def test_host_forms_follow_a_set_replaced_by_one_of_the_same_size():
    data = make_input()
    gpu, cpu = api.PFAC.create(), api.PFAC.createHostOnly()
    try:
        tokens = None
        for name, patterns in (("A", SET_A), ("B", SET_B)):
            gpu.readPatternFromMemory(patterns)
            cpu.readPatternFromMemory(patterns)
            want, tokens = every_form(cpu, data, tokens)         # the replacement of both rounds gets the tokens of set A
            got, _ = every_form(gpu, data, tokens)
            assert want["all"][1] > 0 and want["replace"][1] > 0
            assert all(want[form][1] > 0 for form in BATCH_FORMS), f"set {name}: {[want[form][1] for form in BATCH_FORMS]}"
            for form in want:
                assert want[form][0] == 0 and same(got[form], want[form]), f"set {name}, {form}: {got[form][:3]} want {want[form][:3]}"
            if name == "A":                                      # what is opened on set A now is asked again once set B is loaded
                stale = (gpu.rulesOpen(RULE_OFF, RULES), gpu.groupsOpen(PATTERN_MASKS))
            else:
                off = segments_of(data)
                assert rules_form(stale[0], data, off, 16)[:2] == (api.STATUS.INVALID_PARAMETER, 0)
                assert groups_form(stale[1], data, off, np.full(off.size - 1, 63, dtype=np.uint64), 0, 16)[:2] == (api.STATUS.INVALID_PARAMETER, 0)
    finally:
        gpu.destroy()
        cpu.destroy()
