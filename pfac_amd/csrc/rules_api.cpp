/*
 * rules_api.cpp -- PFACX_rulesOpen / PFACX_rulesClose / PFACX_rulesMatchFromDevice / ...FromHost (include/pfac_ext.h): which segments of a batch
 * contain every pattern of a rule.
 *
 * A rule set is inverted once, at open: every named id resolved to the id that is reported (duplicate lines), the ids of a rule made distinct and
 * numbered 0 .. 31 in ascending order, then a CSR by pattern id -- memberOff[F + 2], member[] = rule << 5 | bit, ascending rule -- and need[rule],
 * the full mask.  Pattern id occurs in a segment iff it lies on the prefix chain (Automaton::prefixPattern) of one of the segment's longest pairs, so
 * both forms work on longest pairs.  The device form takes the ordered pairs of the batch in the handle's pair scratch from scratchBatchPairs
 * (batch_api.cpp) and runs PFACX_rulesRun (scan_rules.hip) over them.  The host form takes the longest pairs of every segment from HostBatchPairs
 * (batch_api.cpp), pins the set the rules were opened on, and decides the touched rules of every segment (firedOnHost) inside the shared host pieces
 * of pfac_host.h: touchedRuleMasks, the walk that sets one mask per touched rule, and sortedSegmentLists, the frame of the fired list.  RuleTables
 * (pfac_host.h) is what the open inverts into; the layout of its windows and links is declared in pfac_context.h for both libraries.
 *
 * PFACX_rulesOpenEx is the same open over members {pattern, flags, offset, depth}: what is made distinct and numbered is the member,
 * need[rule] keeps the bits of the positive members only (a bit a negated member sets makes mask != need), and memberCond[], indexed like member[],
 * holds each membership's window.  PFACX_rulesOpen is its unconditioned case and leaves memberCond empty: a plain set, which runs what it always has.
 * For a conditioned set both forms keep the pairs' positions and OR a membership's bit only where the pattern on the chain, by itself, lies inside
 * the segment and satisfies the window (windowHolds here, pfac_rules_pass<EMIT, true> on the device); no input byte is read for it.
 *
 * PFACX_rulesOpenSeq is the same open over members that also carry {distance, within}.  A rule with a PFACX_RULE_RELATIVE member keeps
 * its members in the order given, nothing merged: bit b is member b, a relative member sets its bit like any conditioned one, so mask == need[rule] is
 * necessary and makes the rule a CANDIDATE.  What decides it is the rule's CHAINS -- seqOff[numRules + 1] and seqLink[], kSeqLinkWords words per link
 * in rule order (pfac_context.h): {resolved id | kSeqFirst on a chain's first link, lo, hi as in memberCond, distance, within} -- which
 * chainsHoldOnHost verifies link by link over the segment's occurrences, and pfac_rules_seq_pass on the device.  A set without a relative member
 * has no seqOff and is the conditioned set PFACX_rulesOpenEx makes of the same members.
 */
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "pfac_host.h"

struct PFACX_rules_s : pfac_internal::HandleObject {
    pfac_internal::RuleTables t;
    /* the same on the device, uploaded by the first device call: state of the set (deviceTableBytes), freed by PFACX_rulesClose */
    pfac::DeviceBuffer<int> d_memberOff, d_seqOff;
    pfac::DeviceBuffer<unsigned int> d_member, d_need, d_memberCond, d_seqLink;

    template <class Self, class F> static void forEachDeviceBuffer(Self &s, F f) { f(s.d_memberOff); f(s.d_member); f(s.d_need); f(s.d_memberCond); f(s.d_seqOff); f(s.d_seqLink); }
    void releaseDevice() { forEachDeviceBuffer(*this, [](auto &b) { b.release(); }); }
    ~PFACX_rules_s() override { releaseDevice(); }
    size_t deviceBytes() const override { size_t n = 0; forEachDeviceBuffer(*this, [&n](const auto &b) { n += b.bytes(); }); return n; }
};

using namespace pfac_internal;

namespace {

constexpr size_t kMaxRules = size_t(1) << 24, kMaxRulePatterns = 32;

using pfac::kCondFromEnd, pfac::kCondEnd, pfac::kSeqLinkWords, pfac::kSeqFirst;      /* pfac_context.h: memberCond's hi, a link of seqLink */

/* a member as the tables keep it: ordered and compared by (resolved id, flags, offset, depth); distance and within are not 0 on a relative member
 * alone, and a rule that has one is neither ordered nor compared */
struct Member {
    int id;
    unsigned int flags, offset, depth, distance = 0, within = 0;
    bool operator<(const Member &o) const
    {
        if (id != o.id) return id < o.id;
        if (flags != o.flags) return flags < o.flags;
        return offset != o.offset ? offset < o.offset : depth < o.depth;
    }
    bool operator==(const Member &o) const { return id == o.id && flags == o.flags && offset == o.offset && depth == o.depth; }
};

/* Does the occurrence at segment-relative s, of length len, in a segment of n bytes satisfy the window {lo, hi} of memberCond?  The test of
 * scan_rules.hip: an occurrence that does not lie inside the segment satisfies nothing, so a + len <= n < 2^31 and nothing wraps */
inline bool windowHolds(long long s, long long len, long long n, unsigned int lo, unsigned int hi)
{
    const long long tail = n - s - len;
    if (s < 0 || tail < 0) return false;
    const long long a = (hi & kCondFromEnd) ? tail : s;
    return a >= (long long)lo && a + len <= (long long)(hi & kCondEnd);
}

/* {lo, hi} of memberCond for a member's own window */
inline void condOf(const Member &m, unsigned int &lo, unsigned int &hi)
{
    const unsigned long long end = m.depth ? (unsigned long long)m.offset + m.depth : kCondEnd;       /* 64-bit: offset + depth does not wrap */
    lo = m.offset;
    hi = (unsigned int)std::min<unsigned long long>(end, kCondEnd) | ((m.flags & PFACX_RULE_FROM_END) ? kCondFromEnd : 0u);
}

/* The rules inverted into *s (the caller holds c->lock; the arguments are checked for null); memberAt(j): member j of the caller's array as a
 * PFACX_rule_seq_member_t.  conditioned: windows and polarity are kept (PFACX_rulesOpenEx); else every member is {id, 0, 0, 0} and the set is plain.
 * flagBits: the flags the call knows -- with PFACX_RULE_RELATIVE among them (PFACX_rulesOpenSeq) a rule that has such a member keeps its order and
 * gets its chains.  false: a rule set the contract refuses */
template <typename MemberAt>
bool invertRules(const pfac::Automaton &fa, const int *ruleOff, MemberAt memberAt, size_t numRules, bool conditioned, unsigned int flagBits,
                 RuleTables *s)
{
    const size_t F = (size_t)fa.numPatterns;
    if (ruleOff[0] != 0) return false;
    for (size_t r = 0; r < numRules; r++)
        if (ruleOff[r + 1] < ruleOff[r]) return false;
    ReportedIds reported(fa);                               /* (a lower id of duplicate lines may be named) */
    std::vector<std::vector<Member>> rules(numRules);
    for (size_t r = 0; r < numRules; r++) {
        std::vector<Member> &ids = rules[r];
        bool positive = false, relative = false;
        for (int j = ruleOff[r]; j < ruleOff[r + 1]; j++) {
            const PFACX_rule_seq_member_t given = memberAt((size_t)j);
            const int id = given.pattern;
            if (id < 1 || (size_t)id > F || (given.flags & ~flagBits)) return false;
            if (given.flags & PFACX_RULE_RELATIVE) {        /* tied to the member in front: there is one, and both are positive */
                if (j == ruleOff[r] || (given.flags & PFACX_RULE_NOT) || (ids.back().flags & PFACX_RULE_NOT)) return false;
                relative = true;
            } else if (given.distance != 0 || given.within != 0) {
                return false;
            }
            positive = positive || !(given.flags & PFACX_RULE_NOT);
            const int as = reported.of(id);
            if (as == 0) return false;
            ids.push_back(Member{as, given.flags, given.offset, given.depth, given.distance, given.within});
        }
        if (!relative) {                                    /* (a rule with a chain: the order given, nothing merged) */
            std::sort(ids.begin(), ids.end());
            ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        } else if (s->seqOff.empty()) {
            s->seqOff.assign(numRules + 1, 0);
        }
        if (ids.empty() || ids.size() > kMaxRulePatterns || !positive) return false;
    }
    s->memberOff.assign(F + 2, 0);
    for (const std::vector<Member> &ids : rules)
        for (const Member &m : ids) s->memberOff[(size_t)m.id + 1]++;
    for (size_t id = 0; id <= F; id++) s->memberOff[id + 1] += s->memberOff[id];
    s->member.resize((size_t)s->memberOff[F + 1]);
    s->memberCond.assign(conditioned ? 2 * s->member.size() : 0, 0u);
    s->need.resize(numRules);
    std::vector<int> at(s->memberOff.begin(), s->memberOff.end() - 1);
    for (size_t r = 0; r < numRules; r++) {                 /* ascending r: the memberships of a pattern ascend */
        const std::vector<Member> &ids = rules[r];
        unsigned int need = 0;
        for (size_t b = 0; b < ids.size(); b++) {
            const Member &m = ids[b];
            const size_t j = (size_t)at[(size_t)m.id]++;
            s->member[j] = (unsigned int)(r << 5 | b);
            if (!(m.flags & PFACX_RULE_NOT)) need |= 1u << b;
            if (conditioned) condOf(m, s->memberCond[2 * j], s->memberCond[2 * j + 1]);
        }
        s->need[r] = need;
        if (s->sequenced()) {                               /* the chains: every maximal run "member, then relative members" of two members or more */
            for (size_t b = 0; b < ids.size(); b++) {
                const bool rel = (ids[b].flags & PFACX_RULE_RELATIVE) != 0;
                if (!rel && !(b + 1 < ids.size() && (ids[b + 1].flags & PFACX_RULE_RELATIVE))) continue;
                unsigned int lo, hi;
                condOf(ids[b], lo, hi);
                const unsigned int link[kSeqLinkWords] = {(unsigned int)ids[b].id | (rel ? 0u : kSeqFirst), lo, hi, ids[b].distance, ids[b].within};
                s->seqLink.insert(s->seqLink.end(), link, link + kSeqLinkWords);
            }
            s->seqOff[r + 1] = (int)(s->seqLink.size() / kSeqLinkWords);
        }
    }
    s->numRules = numRules;
    s->numIds = F;
    return true;
}

/* what both match calls check first, in the order of the contract (the generation and the pattern set: under the lock) */
PFAC_status_t checkMatchArgs(PFACX_rules_t rules, const void *input, size_t size, const size_t *offsets, size_t numSegments, const int *firedSeg,
                             const int *firedRule, size_t capacity, const size_t *h_numFired)
{
    if (!rules || !rules->handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!input || !h_numFired || (capacity && (!firedSeg || !firedRule)) || (!offsets && numSegments != 1)) return PFAC_STATUS_INVALID_PARAMETER;
    if (size >= kTwoGiB || numSegments >= kTwoGiB || (numSegments == 0 && size > 0)) return PFAC_STATUS_INVALID_PARAMETER;
    return PFAC_STATUS_SUCCESS;
}

/* Do all chains of rule r hold in a segment of n bytes whose numPairs longest pairs are (ids[i], pos[i]), pos relative to the segment and ascending?
 * Link by link: `reach` is the ascending starts of the occurrences of the link in front that satisfy their own window and, behind a chain's first
 * link, have a reachable predecessor.  An occurrence at s of the next link is reachable iff some start p of reach has p + lenPrev + distance <= s
 * and (within == 0 or s + len <= p + lenPrev + within): p in [low, high], which the LARGEST p <= high decides -- exact, whatever the assignment a
 * search would have tried first.  64-bit throughout: distance = 0xFFFFFFFF makes high negative */
bool chainsHoldOnHost(const pfac::Automaton &fa, const RuleTables &s, unsigned int r, const int *ids, const int *pos, int numPairs, long long n,
                      std::vector<long long> &reach, std::vector<long long> &next)
{
    long long lenPrev = 0;
    for (int l = s.seqOff[r]; l < s.seqOff[r + 1]; l++) {
        const unsigned int *link = &s.seqLink[kSeqLinkWords * (size_t)l];
        const int id = (int)(link[0] & ~kSeqFirst);
        const bool first = (link[0] & kSeqFirst) != 0;
        const long long len = fa.patternLen[(size_t)id], distance = link[3], within = link[4];
        next.clear();
        for (int i = 0; i < numPairs; i++) {
            bool occurs = false;
            forEachChainMember(fa, ids[i], [&](int q) { occurs = q == id; return !occurs; });
            const long long at = pos[i];
            if (!occurs || !windowHolds(at, len, n, link[1], link[2])) continue;
            if (!first) {
                const long long high = at - distance - lenPrev, low = within ? at + len - within - lenPrev : 0;
                const auto behind = std::upper_bound(reach.begin(), reach.end(), high);
                if (behind == reach.begin() || *(behind - 1) < low) continue;
            }
            next.push_back(at);
        }
        if (next.empty()) return false;                     /* whichever link it is: its chain does not hold */
        if (!std::is_sorted(next.begin(), next.end())) std::sort(next.begin(), next.end());         /* (pairs that came in another order) */
        reach.swap(next);
        lenPrev = len;
    }
    return true;
}

/* The fired list of a batch whose longest pairs are known: the ids of segment k at ids[first[k], first[k] + numPairs[k]), their positions in the
 * segment at pos[] likewise (read for a conditioned set only: may be null for a plain one); segment k has first[k + 1] - first[k] bytes.  Returns
 * the full length */
size_t firedOnHost(const pfac::Automaton &fa, const RuleTables &t, const int *ids, const int *pos, const size_t *first, const int *numPairs,
                   size_t numSegments, int *firedSeg, int *firedRule, size_t capacity, size_t *segFirst)
{
    std::vector<unsigned int> mask(t.numRules, 0u), touched;
    std::vector<long long> reach, next;                     /* chainsHoldOnHost's */
    const bool cond = t.conditioned();
    auto fill = [&](size_t k, std::vector<unsigned int> &fired) {
        const int *segIds = ids + first[k], *segPos = cond ? pos + first[k] : nullptr;
        const long long n = (long long)(first[k + 1] - first[k]);
        touchedRuleMasks(fa, t, segIds, (size_t)numPairs[k], mask, touched, [&](size_t i, size_t j, int q) {      /* a plain set: every occurrence */
            return !cond || windowHolds(segPos[i], fa.patternLen[(size_t)q], n, t.memberCond[2 * j], t.memberCond[2 * j + 1]);
        });
        for (unsigned int r : touched) {
            /* (a candidate with chains: verified over the segment's pairs) */
            if (mask[r] == t.need[r] &&
                (!t.sequenced() || t.seqOff[r] == t.seqOff[r + 1] || chainsHoldOnHost(fa, t, r, segIds, segPos, numPairs[k], n, reach, next)))
                fired.push_back(r);
            mask[r] = 0;
        }
    };
    return sortedSegmentLists<unsigned int>(numSegments, capacity, segFirst, fill, storeSegmentAndRule(firedSeg, firedRule));
}

/* the first device call of a rule set: its tables (the caller holds the handle's lock) */
PFAC_status_t ensureDeviceTables(PFACX_rules_s *s)
{
    if (s->d_need) return PFAC_STATUS_SUCCESS;
    const RuleTables &t = s->t;
    PFAC_status_t st = uploadAll(s->d_memberOff, t.memberOff, s->d_member, t.member, s->d_need, t.need);
    if (st == PFAC_STATUS_SUCCESS && t.conditioned()) st = uploadAll(s->d_memberCond, t.memberCond);
    if (st == PFAC_STATUS_SUCCESS && t.sequenced()) st = uploadAll(s->d_seqOff, t.seqOff, s->d_seqLink, t.seqLink);
    if (st != PFAC_STATUS_SUCCESS) s->releaseDevice();
    return st;
}

/* PFACX_rulesOpen (conditioned == false: memberAt gives {id, 0, 0, 0, 0, 0}), PFACX_rulesOpenEx and PFACX_rulesOpenSeq behind their null checks */
template <typename MemberAt>
PFAC_status_t openRules(PFAC_handle_t handle, const int *h_ruleOff, MemberAt memberAt, size_t numRules, bool conditioned, unsigned int flagBits,
                        PFACX_rules_t *rules)
{
    if (numRules == 0 || numRules >= kMaxRules) return PFAC_STATUS_INVALID_PARAMETER;
    return adoptNew(handle, rules, [&](PFACX_rules_s &s) {
        return invertRules(handle->fa, h_ruleOff, memberAt, numRules, conditioned, flagBits, &s.t) ? PFAC_STATUS_SUCCESS : PFAC_STATUS_INVALID_PARAMETER;
    });
}
constexpr unsigned int kCondFlags = PFACX_RULE_NOT | PFACX_RULE_FROM_END;

} // namespace

/* pfac_host.h: what PFACX_rulesOpen makes of its arrays, for the flow-rule sets */
PFAC_status_t pfac_internal::invertPlainRules(const pfac::Automaton &fa, const int *h_ruleOff, const int *h_rulePatterns, size_t numRules, RuleTables *out)
{
    if (numRules == 0 || numRules >= kMaxRules) return PFAC_STATUS_INVALID_PARAMETER;
    const auto memberAt = [=](size_t j) { return PFACX_rule_seq_member_t{h_rulePatterns[j], 0u, 0u, 0u, 0u, 0u}; };
    return invertRules(fa, h_ruleOff, memberAt, numRules, false, 0u, out) ? PFAC_STATUS_SUCCESS : PFAC_STATUS_INVALID_PARAMETER;
}

extern "C" {

PFAC_status_t PFACX_rulesOpen(PFAC_handle_t handle, const int *h_ruleOff, const int *h_rulePatterns, size_t numRules, PFACX_rules_t *rules)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!rules) return PFAC_STATUS_INVALID_PARAMETER;
    *rules = nullptr;
    if (!h_ruleOff || !h_rulePatterns) return PFAC_STATUS_INVALID_PARAMETER;
    return openRules(handle, h_ruleOff, [=](size_t j) { return PFACX_rule_seq_member_t{h_rulePatterns[j], 0u, 0u, 0u, 0u, 0u}; }, numRules, false, 0u,
                     rules);
}

PFAC_status_t PFACX_rulesOpenEx(PFAC_handle_t handle, const int *h_ruleOff, const PFACX_rule_member_t *h_members, size_t numRules, PFACX_rules_t *rules)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!rules) return PFAC_STATUS_INVALID_PARAMETER;
    *rules = nullptr;
    if (!h_ruleOff || !h_members) return PFAC_STATUS_INVALID_PARAMETER;
    return openRules(handle, h_ruleOff,
                     [=](size_t j) {
                         const PFACX_rule_member_t &m = h_members[j];
                         return PFACX_rule_seq_member_t{m.pattern, m.flags, m.offset, m.depth, 0u, 0u};
                     },
                     numRules, true, kCondFlags, rules);
}

PFAC_status_t PFACX_rulesOpenSeq(PFAC_handle_t handle, const int *h_ruleOff, const PFACX_rule_seq_member_t *h_members, size_t numRules,
                                 PFACX_rules_t *rules)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!rules) return PFAC_STATUS_INVALID_PARAMETER;
    *rules = nullptr;
    if (!h_ruleOff || !h_members) return PFAC_STATUS_INVALID_PARAMETER;
    return openRules(handle, h_ruleOff, [=](size_t j) { return h_members[j]; }, numRules, true, kCondFlags | PFACX_RULE_RELATIVE, rules);
}

PFAC_status_t PFACX_rulesClose(PFACX_rules_t rules) { return closeObject(rules); }

PFAC_status_t PFACX_rulesMatchFromDevice(PFACX_rules_t rules, char *d_input, size_t size, const size_t *d_offsets, size_t numSegments,
                                         int *d_firedSeg, int *d_firedRule, size_t capacity, size_t *d_segFirst, size_t *h_numFired)
{
    PFAC_status_t st = checkMatchArgs(rules, d_input, size, d_offsets, numSegments, d_firedSeg, d_firedRule, capacity, h_numFired);
    if (st != PFAC_STATUS_SUCCESS) return st;
    PFAC_context *c = rules->handle;
    if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(c->lock);
    st = checkSetGeneration(c, rules->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0) {
        st = zeroSegmentArrays(d_segFirst, nullptr, numSegments);
        if (st == PFAC_STATUS_SUCCESS) *h_numFired = 0;
        return st;
    }
    st = ensureDeviceTables(rules);
    if (st == PFAC_STATUS_SUCCESS) st = ensureAllTable(c);
    const bool cond = rules->t.conditioned();
    if (st == PFAC_STATUS_SUCCESS && cond) st = ensurePatternLen(c);            /* the window test's, offsets or none */
    BatchPairs pairs{};
    if (st == PFAC_STATUS_SUCCESS) st = scratchBatchPairs(c, d_input, size, d_offsets, numSegments, &pairs);
    if (st != PFAC_STATUS_SUCCESS) return st;
    PFACX_rulesRun_t run{};
    run.d_pairIds = pairs.ids;
    run.count = pairs.count;
    run.d_segFirstPairs = pairs.segFirstPairs;
    run.numSegments = numSegments;
    run.d_table = c->scratch.allTable.get();
    run.numIds = rules->t.numIds;
    run.d_memberOff = rules->d_memberOff.get();
    run.d_member = rules->d_member.get();
    run.d_need = rules->d_need.get();
    run.numRules = rules->t.numRules;
    run.d_firedSeg = d_firedSeg;
    run.d_firedRule = d_firedRule;
    run.capacity = capacity;
    run.d_segFirst = d_segFirst;
    if (cond) {                                                                 /* the window test: positions, bounds and lengths, no input byte */
        run.d_pairPos = pairs.pos;
        run.d_offsets = d_offsets;
        run.size = size;
        run.d_patternLen = c->scratch.patternLen.get();
        run.d_memberCond = rules->d_memberCond.get();
        run.d_seqOff = rules->d_seqOff.get();                                   /* (both null for a set without chains) */
        run.d_seqLink = rules->d_seqLink.get();
    }
    size_t total = 0;
    st = c->rules_run_ptr(c, &run, &total);
    if (st != PFAC_STATUS_SUCCESS) return st;
    *h_numFired = total;
    return truncatedIf(total, capacity);
}

PFAC_status_t PFACX_rulesMatchFromHost(PFACX_rules_t rules, char *h_input, size_t size, const size_t *h_offsets, size_t numSegments,
                                       int *h_firedSeg, int *h_firedRule, size_t capacity, size_t *h_segFirst, size_t *h_numFired)
{
    PFAC_status_t st = checkMatchArgs(rules, h_input, size, h_offsets, numSegments, h_firedSeg, h_firedRule, capacity, h_numFired);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (h_offsets && numSegments && !batchOffsetsValid(h_offsets, numSegments, size)) return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = rules->handle;
    std::unique_lock<std::mutex> guard(c->lock);
    st = checkSetGeneration(c, rules->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0) {
        if (h_segFirst && numSegments) std::memset(h_segFirst, 0, (numSegments + 1) * sizeof(size_t));
        *h_numFired = 0;
        return PFAC_STATUS_SUCCESS;
    }
    HostBatchPairs pairs(c, h_input, size, h_offsets, numSegments, rules->t.conditioned(), guard);       /* a conditioned set reads the positions */
    if (pairs.status != PFAC_STATUS_SUCCESS) return pairs.status;
    if (pairs.pin(rules->generation) != PFAC_STATUS_SUCCESS) return PFAC_STATUS_INVALID_PARAMETER;      /* another thread has replaced the set meanwhile: the contract's answer for a rule set */
    try {
        const size_t total = firedOnHost(c->fa, rules->t, pairs.ids, pairs.pos, pairs.offsets, pairs.numPairs.data(), numSegments, h_firedSeg, h_firedRule,
                                         capacity, h_segFirst);
        *h_numFired = total;
        return truncatedIf(total, capacity);
    } catch (const std::bad_alloc &) {
        return PFAC_STATUS_ALLOC_FAILED;
    }
}

} /* extern "C" */
