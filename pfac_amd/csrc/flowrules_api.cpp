/*
 * flowrules_api.cpp -- PFACX_flowRulesOpen / Close / Reset / PairsFromDevice / PairsFromHost (include/pfac_ext.h): which rules a
 * flows call completes on each of its pieces, members that arrived in earlier calls included.
 *
 * A flow-rule set is the plain rule set of PFACX_rulesOpen -- validated and inverted by the same code (invertPlainRules, rules_api.cpp) into the
 * same RuleTables (pfac_host.h) -- plus
 * the state of numFlows flows.  The D distinct resolved ids the rules name are numbered in ascending order (bitOf[id], -1 for every other
 * pattern), and a flow's state is one bitmap of D bits: the patterns that have occurred in it since its last reset.  Rule r's forward list --
 * ruleBits[ruleFirst[r] + b]: the bit of its b-th member -- turns the bitmap into the mask the rule had BEFORE a call; the inverted tables give
 * the bits the call's pairs add; the rule fires iff the two together are the full mask and the old one alone was not.
 * The calls take pairs, not bytes: ids and pieceFirst of a flows call (or flush), with that call's flow ids.  The device form runs
 * PFACX_flowRulesRun (scan_flowrules.hip) over the caller's device arrays; its bitmaps are ONE device allocation, made with the tables by the
 * first device call.  The host form works on host arrays, the same on every platform, with the bitmaps in a host vector: the shared walk and
 * list frame of pfac_host.h (touchedRuleMasks, sortedSegmentLists) around its own decision (firedOnHost).  Both leave every flow as it was unless
 * the whole list fitted the caller's arrays.
 * Every call holds the set's own lock and the handle's lock from the check of the pattern set to its end.
 */
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "pfac_host.h"

struct PFACX_flowRules_s : pfac_internal::HandleObject {
    int kind = 0;                             /* 0: not fed yet, 1: host calls, 2: device calls */
    size_t numFlows = 0;
    size_t numBits = 0;                       /* D: the distinct resolved ids the rules name */
    size_t words = 0;                         /* ceil(D / 32): the words of a flow's bitmap */
    pfac_internal::RuleTables t;              /* memberOff[F + 2], member[] = rule << 5 | bit, need[rule]: a plain set */
    std::vector<int> ruleFirst;               /* [numRules + 1]: rule r has ruleFirst[r + 1] - ruleFirst[r] members */
    std::vector<unsigned int> ruleBits;       /* the forward list: the bit of member b of rule r at ruleFirst[r] + b */
    std::vector<int> bitOf;                   /* [F + 1] by id: its bit in a flow's bitmap, -1: no rule names it */
    std::vector<unsigned int> h_bits;         /* host-fed: numFlows x words, made by the first host call */
    std::vector<unsigned int> named;          /* per flow: the number of the last call that named it (a flow named twice) */
    unsigned int callNo = 0;
    /* device-fed: the tables and, in ONE allocation, the bitmaps -- state of the set (deviceTableBytes), made by the first device call */
    pfac::DeviceBuffer<int> d_memberOff, d_ruleFirst, d_bitOf;
    pfac::DeviceBuffer<unsigned int> d_member, d_ruleBits, d_flowBits;
    std::mutex lock;                          /* one call at a time per set */

    template <class Self, class F> static void forEachDeviceBuffer(Self &s, F f) { f(s.d_memberOff); f(s.d_ruleFirst); f(s.d_bitOf); f(s.d_member); f(s.d_ruleBits); f(s.d_flowBits); }
    void releaseDevice() { forEachDeviceBuffer(*this, [](auto &b) { b.release(); }); }
    ~PFACX_flowRules_s() override { releaseDevice(); }
    size_t deviceBytes() const override { size_t n = 0; forEachDeviceBuffer(*this, [&n](const auto &b) { n += b.bytes(); }); return n; }
};

using namespace pfac_internal;

namespace {

/* bitOf, ruleFirst and ruleBits from the inverted tables: bits in ascending id order, bit b of a rule its b-th resolved id */
void buildForward(PFACX_flowRules_s &s)
{
    const size_t F = s.t.numIds, R = s.t.numRules;
    s.bitOf.assign(F + 1, -1);
    size_t D = 0;
    for (size_t id = 1; id <= F; id++)
        if (s.t.memberOff[id + 1] > s.t.memberOff[id]) s.bitOf[id] = (int)D++;
    s.numBits = D;
    s.words = (D + 31) / 32;
    s.ruleFirst.assign(R + 1, 0);
    for (size_t r = 0; r < R; r++) s.ruleFirst[r + 1] = s.ruleFirst[r] + __builtin_popcount(s.t.need[r]);
    s.ruleBits.assign(s.t.member.size(), 0u);
    for (size_t id = 1; id <= F; id++)
        for (int j = s.t.memberOff[id]; j < s.t.memberOff[id + 1]; j++) {
            const unsigned int m = s.t.member[(size_t)j];
            s.ruleBits[(size_t)s.ruleFirst[m >> 5] + (m & 31u)] = (unsigned int)s.bitOf[id];
        }
}

/* every id below numFlows, no flow twice */
bool idsValid(PFACX_flowRules_s *s, const unsigned int *ids, size_t n)
{
    s->callNo = s->callNo + 1u ? s->callNo + 1u : 1u;
    if (s->callNo == 1u) std::fill(s->named.begin(), s->named.end(), 0u);
    for (size_t k = 0; k < n; k++) {
        if (ids[k] >= s->numFlows || s->named[ids[k]] == s->callNo) return false;
        s->named[ids[k]] = s->callNo;
    }
    return true;
}

/* what both pairs calls check before they hold a lock */
PFAC_status_t checkPairsArgs(PFACX_flowRules_t fr, const int *ids, size_t numPairs, const int *pieceFirst, const unsigned int *h_flowIds,
                             size_t numPieces, const int *firedPiece, const int *firedRule, size_t capacity, const size_t *h_numFired)
{
    if (!fr || !fr->handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!h_numFired || (capacity && (!firedPiece || !firedRule)) || numPairs >= kTwoGiB || numPieces >= kTwoGiB) return PFAC_STATUS_INVALID_PARAMETER;
    if (numPieces == 0) return numPairs == 0 ? PFAC_STATUS_SUCCESS : PFAC_STATUS_INVALID_PARAMETER;
    if (!pieceFirst || !h_flowIds || (numPairs && !ids)) return PFAC_STATUS_INVALID_PARAMETER;
    return PFAC_STATUS_SUCCESS;
}

/* the first device call of a set: its tables and its bitmaps, all flows empty (the caller holds the handle's lock) */
PFAC_status_t ensureDeviceState(PFACX_flowRules_s *s)
{
    if (s->d_flowBits) return PFAC_STATUS_SUCCESS;
    PFAC_status_t st = uploadAll(s->d_memberOff, s->t.memberOff, s->d_member, s->t.member, s->d_ruleFirst, s->ruleFirst, s->d_ruleBits, s->ruleBits,
                                 s->d_bitOf, s->bitOf);
    if (st == PFAC_STATUS_SUCCESS) st = s->d_flowBits.reserve(s->numFlows * s->words);
    if (st == PFAC_STATUS_SUCCESS && hipMemset(s->d_flowBits.get(), 0, s->d_flowBits.bytes()) != hipSuccess) st = PFAC_STATUS_INTERNAL_ERROR;
    if (st != PFAC_STATUS_SUCCESS) s->releaseDevice();
    return st;
}

/* The fired list of one call on the host: the pairs of piece k are ids[first[k], first[k + 1]) (validated), its flow flowIds[k].  Returns the
 * full length; the bitmaps are only read */
size_t firedOnHost(const pfac::Automaton &fa, const PFACX_flowRules_s &s, const int *ids, const int *first, const unsigned int *flowIds,
                   size_t numPieces, int *firedPiece, int *firedRule, size_t capacity, size_t *pieceFiredFirst)
{
    std::vector<unsigned int> mask(s.t.numRules, 0u), touched;
    auto fill = [&](size_t k, std::vector<unsigned int> &fired) {
        const unsigned int *seen = s.h_bits.data() + (size_t)flowIds[k] * s.words;
        touchedRuleMasks(fa, s.t, ids + first[k], (size_t)(first[k + 1] - first[k]), mask, touched, [](size_t, size_t, int) { return true; });
        for (unsigned int r : touched) {
            unsigned int old = 0;
            for (int b = 0; b < s.ruleFirst[r + 1] - s.ruleFirst[r]; b++) {
                const unsigned int bit = s.ruleBits[(size_t)(s.ruleFirst[r] + b)];
                old |= ((seen[bit >> 5] >> (bit & 31u)) & 1u) << b;
            }
            if ((old | mask[r]) == s.t.need[r] && old != s.t.need[r]) fired.push_back(r);       /* complete now, not before */
            mask[r] = 0;
        }
    };
    return sortedSegmentLists<unsigned int>(numPieces, capacity, pieceFiredFirst, fill, storeSegmentAndRule(firedPiece, firedRule));
}

/* ... and, the list having fitted, the pairs into their flows' bitmaps */
void commitOnHost(const pfac::Automaton &fa, PFACX_flowRules_s &s, const int *ids, const int *first, const unsigned int *flowIds, size_t numPieces)
{
    for (size_t k = 0; k < numPieces; k++) {
        unsigned int *seen = s.h_bits.data() + (size_t)flowIds[k] * s.words;
        for (int i = first[k]; i < first[k + 1]; i++)
            forEachChainMember(fa, ids[i], [&](int q) {
                const int bit = s.bitOf[(size_t)q];
                if (bit >= 0) seen[(size_t)bit >> 5] |= 1u << ((unsigned int)bit & 31u);
                return true;
            });
    }
}

} // namespace

extern "C" {

PFAC_status_t PFACX_flowRulesOpen(PFAC_handle_t handle, const int *h_ruleOff, const int *h_rulePatterns, size_t numRules, size_t numFlows,
                                  PFACX_flowRules_t *fr)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!fr) return PFAC_STATUS_INVALID_PARAMETER;
    *fr = nullptr;
    if (!h_ruleOff || !h_rulePatterns || numFlows == 0 || numFlows >= kTwoGiB) return PFAC_STATUS_INVALID_PARAMETER;
    return adoptNew(handle, fr, [=](PFACX_flowRules_s &s) -> PFAC_status_t {
        const PFAC_status_t st = invertPlainRules(handle->fa, h_ruleOff, h_rulePatterns, numRules, &s.t);
        if (st != PFAC_STATUS_SUCCESS) return st;
        buildForward(s);
        if (numFlows > SIZE_MAX / sizeof(unsigned int) / s.words) return PFAC_STATUS_ALLOC_FAILED;       /* (a rule has a member: words >= 1) */
        s.numFlows = numFlows;
        s.named.assign(numFlows, 0u);
        return PFAC_STATUS_SUCCESS;
    });
}

PFAC_status_t PFACX_flowRulesClose(PFACX_flowRules_t fr) { return closeObject(fr); }

PFAC_status_t PFACX_flowRulesReset(PFACX_flowRules_t fr, const unsigned int *h_flowIds, size_t n)
{
    if (!fr || !fr->handle) return PFAC_STATUS_INVALID_HANDLE;
    std::lock_guard<std::mutex> own(fr->lock);
    std::lock_guard<std::mutex> guard(fr->handle->lock);
    const PFAC_status_t st = checkSetGeneration(fr->handle, fr->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    const size_t flowBytes = fr->words * sizeof(unsigned int);
    if (!h_flowIds && n == 0) {
        if (fr->d_flowBits && hipMemset(fr->d_flowBits.get(), 0, fr->d_flowBits.bytes()) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
        std::fill(fr->h_bits.begin(), fr->h_bits.end(), 0u);
        fr->kind = 0;
        return PFAC_STATUS_SUCCESS;
    }
    if (!h_flowIds) return PFAC_STATUS_INVALID_PARAMETER;
    for (size_t k = 0; k < n; k++) if (h_flowIds[k] >= fr->numFlows) return PFAC_STATUS_INVALID_PARAMETER;
    for (size_t k = 0; k < n; k++) {
        const size_t at = (size_t)h_flowIds[k] * fr->words;
        if (fr->d_flowBits && hipMemset(fr->d_flowBits.get() + at, 0, flowBytes) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
        if (!fr->h_bits.empty()) std::fill_n(fr->h_bits.begin() + (ptrdiff_t)at, fr->words, 0u);
    }
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_flowRulesPairsFromDevice(PFACX_flowRules_t fr, const int *d_pairIds, size_t numPairs, const int *d_pieceFirst,
                                             const unsigned int *h_flowIds, size_t numPieces, int *d_firedPiece, int *d_firedRule, size_t capacity,
                                             size_t *d_pieceFiredFirst, size_t *h_numFired)
{
    PFAC_status_t st = checkPairsArgs(fr, d_pairIds, numPairs, d_pieceFirst, h_flowIds, numPieces, d_firedPiece, d_firedRule, capacity, h_numFired);
    if (st != PFAC_STATUS_SUCCESS) return st;
    PFAC_context *c = fr->handle;
    if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> own(fr->lock);
    std::lock_guard<std::mutex> guard(c->lock);
    st = checkSetGeneration(c, fr->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (numPieces == 0) { *h_numFired = 0; return PFAC_STATUS_SUCCESS; }
    if (!idsValid(fr, h_flowIds, numPieces)) return PFAC_STATUS_INVALID_PARAMETER;
    if (numPairs && fr->kind == 1) return PFAC_STATUS_INVALID_PARAMETER;         /* a host-fed set */
    st = ensureDeviceState(fr);
    if (st == PFAC_STATUS_SUCCESS) st = ensureAllTable(c);
    if (st != PFAC_STATUS_SUCCESS) return st;
    PFACX_flowRulesRun_t run{};
    run.d_pairIds = d_pairIds;
    run.count = numPairs;
    run.d_pieceFirst = d_pieceFirst;
    run.h_flowIds = h_flowIds;
    run.numPieces = numPieces;
    run.d_table = c->scratch.allTable.get();
    run.numIds = fr->t.numIds;
    run.d_memberOff = fr->d_memberOff.get();
    run.d_member = fr->d_member.get();
    run.d_ruleFirst = fr->d_ruleFirst.get();
    run.d_ruleBits = fr->d_ruleBits.get();
    run.d_bitOf = fr->d_bitOf.get();
    run.numRules = fr->t.numRules;
    run.d_flowBits = fr->d_flowBits.get();
    run.numFlows = fr->numFlows;
    run.wordsPerFlow = fr->words;
    run.d_firedPiece = d_firedPiece;
    run.d_firedRule = d_firedRule;
    run.capacity = capacity;
    run.d_pieceFiredFirst = d_pieceFiredFirst;
    size_t total = 0;
    st = c->flowrules_run_ptr(c, &run, &total);
    if (st != PFAC_STATUS_SUCCESS) return st;
    *h_numFired = total;
    if (total <= capacity && numPairs) fr->kind = 2;                             /* the flows have moved on */
    return truncatedIf(total, capacity);
}

PFAC_status_t PFACX_flowRulesPairsFromHost(PFACX_flowRules_t fr, const int *h_pairIds, size_t numPairs, const int *h_pieceFirst,
                                           const unsigned int *h_flowIds, size_t numPieces, int *h_firedPiece, int *h_firedRule, size_t capacity,
                                           size_t *h_pieceFiredFirst, size_t *h_numFired)
{
    PFAC_status_t st = checkPairsArgs(fr, h_pairIds, numPairs, h_pieceFirst, h_flowIds, numPieces, h_firedPiece, h_firedRule, capacity, h_numFired);
    if (st != PFAC_STATUS_SUCCESS) return st;
    PFAC_context *c = fr->handle;
    std::lock_guard<std::mutex> own(fr->lock);
    std::lock_guard<std::mutex> guard(c->lock);
    st = checkSetGeneration(c, fr->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (numPieces == 0) { *h_numFired = 0; return PFAC_STATUS_SUCCESS; }
    if (h_pieceFirst[0] != 0 || (size_t)h_pieceFirst[numPieces] != numPairs) return PFAC_STATUS_INVALID_PARAMETER;
    for (size_t k = 0; k < numPieces; k++)
        if (h_pieceFirst[k + 1] < h_pieceFirst[k]) return PFAC_STATUS_INVALID_PARAMETER;
    if (!idsValid(fr, h_flowIds, numPieces)) return PFAC_STATUS_INVALID_PARAMETER;
    if (numPairs && fr->kind == 2) return PFAC_STATUS_INVALID_PARAMETER;         /* a device-fed set */
    try {
        if (fr->h_bits.empty()) fr->h_bits.assign(fr->numFlows * fr->words, 0u);
        const size_t total = firedOnHost(c->fa, *fr, h_pairIds, h_pieceFirst, h_flowIds, numPieces, h_firedPiece, h_firedRule, capacity, h_pieceFiredFirst);
        *h_numFired = total;
        if (total <= capacity && numPairs) {                                     /* the flows move on */
            commitOnHost(c->fa, *fr, h_pairIds, h_pieceFirst, h_flowIds, numPieces);
            fr->kind = 1;
        }
        return truncatedIf(total, capacity);
    } catch (const std::bad_alloc &) {
        return PFAC_STATUS_ALLOC_FAILED;
    }
}

} /* extern "C" */
