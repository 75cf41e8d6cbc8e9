"""The model of the flow-rule calls (PFACX_flowRules*) for tests/test_flowrules_host.py and test_flowrules_gpu.py.

Nothing here uses the library's rule or flow code.  The input is a schedule of tests/flows_ref.py: per step the pairs every piece of every flow
must return.  A pair's id is expanded by a prefix relation computed here from the pattern BYTES (pattern q occurs where pattern p is the longest iff
q's bytes are a prefix of p's), a flow is a set of the byte strings seen since its last reset, a rule is the set of the byte strings of its ids (so
duplicate lines need no id resolution), and a rule fires on the piece after whose pairs its set is inside the flow's for the first time.  A flush
step is a call with the flush's pairs followed by a reset of its flows (what the caller of PFACX_flowsFlush does); a reset step is a reset.

build() asserts the coverage a lucky schedule could miss (Coverage) and the end-to-end property: for every flow life that ended in a flush, the
union of the rules fired over all its steps is what tests/rules_ref.py fires over the life's whole bytes as one segment.
"""
import os

import numpy as np

from tests import flows_ref as fr
from tests import nocase_ref as nc
from tests import rules_ref as rr


class Call:
    """one pairs call: src is the flows_ref step (a Batch, or an End of kind 'flush') whose ids / first / flows are the input"""

    def __init__(self, src, flush, piece, rule, fired_first):
        self.src, self.flush, self.piece, self.rule, self.fired_first = src, flush, piece, rule, fired_first


class Reset:
    def __init__(self, flows):
        self.flows = flows


class Coverage:
    three_calls = False        # a rule completed by members first seen in three different calls
    two_in_one_call = False    # ... by two members new in the same call
    seen_again = False         # a member of a fired rule fed again
    prefix_only = False        # a member that never was the longest pattern at its position
    by_flush = False           # a rule completed by a flush's pairs
    fired_again = False        # a (flow, rule) that fires a second time after a reset
    fired = 0


class Model:
    def __init__(self):
        self.steps = []
        self.cov = Coverage()
        self.flows = None      # the flows_ref model


def prefix_chains(pats):
    """chain[id] (ids from 1): the byte strings of the patterns that occur where pattern id is the longest -- the prefixes of its bytes that are
    patterns, itself included"""
    have = set(pats)
    return [None] + [[p[:n] for n in range(1, len(p) + 1) if p[:n] in have] for p in pats]


def build(m, pats, rules, fold=None):
    """the flow-rule model of the flows_ref model m: pats[i] is pattern id i + 1 as the handle matches it (folded, for a caseless set), rules a
    list of 1-based id lists"""
    chain = prefix_chains(pats)
    members = [frozenset(pats[i - 1] for i in ids) for ids in rules]
    by_bytes = {}
    for r, ms in enumerate(members):
        for b in ms:
            by_bytes.setdefault(b, []).append(r)
    out = Model()
    out.flows = m
    cov = out.cov
    seen = [dict() for _ in range(m.F)]            # per flow: bytes -> [number of the call it was first seen in, it has been a pair's own id]
    fired_now = [set() for _ in range(m.F)]        # per flow: the rules fired since its last reset
    fired_ever = [set() for _ in range(m.F)]
    life = [[] for _ in range(m.F)]                # per flow: the pieces' bytes since its last reset
    union = [set() for _ in range(m.F)]

    def reset(flows):
        for f in flows:
            seen[f].clear()
            fired_now[f].clear()
            life[f] = []
            union[f] = set()

    for no, s in enumerate(m.steps):
        if isinstance(s, fr.End) and s.kind == "reset":
            out.steps.append(Reset(s.flows))
            reset(s.flows.tolist())
            continue
        flush = isinstance(s, fr.End)
        piece, rule, first = [], [], [0]
        for k, f in enumerate(s.flows.tolist()):
            if not flush:
                life[f].append(s.buf[int(s.offsets[k]):int(s.offsets[k + 1])])
            new = {}
            for i in s.ids[int(s.first[k]):int(s.first[k + 1])].tolist():
                own = pats[i - 1]
                for b in chain[i]:
                    if b in seen[f]:
                        seen[f][b][1] = seen[f][b][1] or b == own
                        cov.seen_again = cov.seen_again or any(r in fired_now[f] for r in by_bytes.get(b, ()))
                    else:
                        new.setdefault(b, [no, False])
                        new[b][1] = new[b][1] or b == own
            touched = sorted({r for b in new for r in by_bytes.get(b, ())})
            for r in touched:
                if all(b in seen[f] or b in new for b in members[r]):          # (a new member: it was not complete before)
                    piece.append(k)
                    rule.append(r)
                    union[f].add(r)
                    cov.fired += 1
                    at = [new[b] if b in new else seen[f][b] for b in members[r]]
                    cov.three_calls = cov.three_calls or len({a[0] for a in at}) >= 3
                    cov.two_in_one_call = cov.two_in_one_call or sum(b in new for b in members[r]) >= 2
                    cov.prefix_only = cov.prefix_only or any(not a[1] for a in at)
                    cov.by_flush = cov.by_flush or flush
                    cov.fired_again = cov.fired_again or r in fired_ever[f]
                    fired_now[f].add(r)
                    fired_ever[f].add(r)
            seen[f].update(new)
            first.append(len(piece))
        out.steps.append(Call(s, flush, np.array(piece, np.int32), np.array(rule, np.int32), np.array(first, np.uint64)))
        if flush:
            for f in s.flows.tolist():                                         # fed completely: the rules of the whole stream as one segment
                whole = np.concatenate(life[f]) if life[f] else np.zeros(0, np.uint8)
                whole = whole if fold is None else fold(whole)
                want = set(rr.fired_py(pats, rules, whole.tobytes())[1].tolist())
                assert union[f] == want, f"flow {f}: the model fired {sorted(union[f])}, the stream as one segment fires {sorted(want)}"
            reset(s.flows.tolist())
    return out


class Sets:
    """the same semantics for hand-made pairs: call(ids, first, flows) -> (piece[], rule[], firedFirst[]) and reset(flows); an id outside
    [1, F] is skipped"""

    def __init__(self, pats, rules, num_flows):
        self.pats, self.chain = pats, prefix_chains(pats)
        self.members = [frozenset(pats[i - 1] for i in ids) for ids in rules]
        self.seen = [set() for _ in range(num_flows)]

    def call(self, ids, first, flows):
        piece, rule, fired_first = [], [], [0]
        for k, f in enumerate(np.asarray(flows).tolist()):
            new = set()
            for i in np.asarray(ids)[int(first[k]):int(first[k + 1])].tolist():
                if 1 <= i <= len(self.pats):
                    new.update(self.chain[i])
            both = self.seen[f] | new
            for r, ms in enumerate(self.members):
                if ms <= both and not ms <= self.seen[f]:
                    piece.append(k)
                    rule.append(r)
            self.seen[f] = both
            fired_first.append(len(piece))
        return np.array(piece, np.int32), np.array(rule, np.int32), np.array(fired_first, np.uint64)

    def reset(self, flows=None):
        for f in range(len(self.seen)) if flows is None else flows:
            self.seen[f] = set()


def check_coverage(fm):
    c = fm.cov
    assert c.three_calls, "no rule completed by members from three different calls"
    assert c.two_in_one_call, "no rule completed by two members new in the same call"
    assert c.seen_again, "no member seen again after its rule fired"
    assert c.prefix_only, "no member that occurs only as a proper prefix of the longest pattern at its position"
    assert c.by_flush, "no rule completed by a flush's pairs"
    assert c.fired_again, "no flow reset midway whose rules fire a second time"
    fr.check_coverage(fm.flows)            # a flow that sits a batch out, a batch of 64 pieces or more, one of a single piece


def run(fm, call, reset, what):
    """the schedule through call(step) -> (piece[], rule[], firedFirst[numPieces + 1], full length) and reset(flow ids); a flush step's flows are
    reset behind its call"""
    for k, s in enumerate(fm.steps):
        if isinstance(s, Reset):
            reset(s.flows)
            continue
        where = f"{what}: step {k} ({'flush' if s.flush else 'batch'} of {s.src.flows.size} pieces, {s.src.ids.size} pairs)"
        piece, rule, first, total = call(s)
        assert total == s.piece.size, f"{where}: {total} fired, want {s.piece.size}"
        assert np.array_equal(np.asarray(first, dtype=np.uint64), s.fired_first), f"{where}: pieceFiredFirst differs"
        assert np.array_equal(piece, s.piece), f"{where}: pieces differ"
        assert np.array_equal(rule, s.rule), f"{where}: rules differ: got {rule.tolist()[:20]} want {s.rule.tolist()[:20]}"
        if s.flush:
            reset(s.src.flows)


# ----------------------------------------------------------------------------- the workload both test files share

FLOWS = 70
FLOW_BYTES = 4096
TOKENS = 40

NAMED = [b"User-Agent:", b"sqlmap", b"GET", b"GET /admin", b"passwd", b"/etc/", b"/etc/passwd", b"EOF!"]


def patterns():
    """ids 1 - 8: NAMED (`GET` and `/etc/` are only ever planted inside their longer patterns); 9 - 48: tokens"""
    return NAMED + [b"Tok%02d;" % i for i in range(TOKENS)]


def rule_list(seed=5):
    rng = np.random.Generator(np.random.PCG64(seed))
    rules = [[1, 2], [3], [3, 5], [4, 6], [6, 7, 5], [8], [8, 1], [8, 3, 2], [2, 2, 1], [48, 1, 9], list(range(9, 41))]
    for _ in range(200):
        rules.append([int(i) for i in rng.integers(1, len(patterns()) + 1, size=int(rng.integers(1, 5)))])
    return rules


RESTART = {3: ("flush", 0.5), 9: ("reset", 0.3), 41: ("reset", 0.7), 69: ("flush", 0.9)}


def workload(workdir, nocase=False, seed=31):
    """(pattern file the oracle reads, pattern bytes the handle reads, patterns as matched, rules, flows_ref model, flow-rule model): 70 flows of
    4 KiB of lower-case noise with some forty patterns planted in each, EOF! as the last bytes of every flow life (shorter than M - 1: pending until the flush).
    nocase: the handle reads the patterns as they are, the data has half its letters flipped, the model matches the fold of both"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pats = patterns()
    plant = [p for p in pats if p not in (b"GET", b"/etc/", b"EOF!")]
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz ", dtype=np.uint8)
    data = alpha[rng.integers(0, alpha.size, FLOWS * FLOW_BYTES)].copy()
    for f in range(FLOWS):
        for _ in range(40):
            p = np.frombuffer(plant[int(rng.integers(0, len(plant)))], dtype=np.uint8)
            at = f * FLOW_BYTES + int(rng.integers(0, FLOW_BYTES - 40))
            data[at:at + p.size] = p
        ends = [FLOW_BYTES] + ([int(FLOW_BYTES * RESTART[f][1])] if f in RESTART else [])
        for e in ends:
            data[f * FLOW_BYTES + e - 4:f * FLOW_BYTES + e] = np.frombuffer(b"EOF!", dtype=np.uint8)
    matched = [nc.fold(p) for p in pats] if nocase else pats
    if nocase:
        data = nc.flip_array(data, rng)
    pf = nc.write_patterns(os.path.join(workdir, "flowrules_%s.pat" % ("nocase" if nocase else "plain")), matched)
    rules = rule_list()
    m = fr.build(pf, data, FLOWS, seed, restart=RESTART, fold=nc.fold_array if nocase else None)
    fm = build(m, matched, rules, fold=nc.fold_array if nocase else None)
    check_coverage(fm)
    return pf, nc.pattern_bytes(pats), matched, rules, m, fm
