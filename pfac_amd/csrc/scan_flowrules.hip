/*
 * scan_flowrules.hip -- flow-rule sets (include/pfac_ext.h: PFACX_flowRules*): which rules a flows call COMPLETES on each of its
 * pieces, members that arrived in earlier calls included.
 *
 * The input is what a flows call returned, still on the device: the longest pairs' ids and the first pair of each piece.  Pattern id has occurred
 * in a flow iff it lies on the prefix chain of a pair fed for that flow, so a flow's state is ONE bitmap over the D patterns the rules name
 * (bitOf[id]: its bit, -1 for a pattern no rule names), not a mask per (flow, rule).  The rule set is the inverted one of the rules calls --
 * memberOff / member (rule << 5 | bit, ascending rule) -- plus its forward list: rule r has ruleFirst[r + 1] - ruleFirst[r] members, its full
 * mask is that many low bits, and member b is bit ruleBits[ruleFirst[r] + b] of a flow's bitmap.
 *
 *   pfac_flowrules_pass<false>  segmentWindows of scan_passes.h with a piece in place of a segment: a block takes whole pieces and walks a piece's
 *                               pairs once per window of kFlowRulesWindow rules it touches, over mask[], a direct-indexed LDS table of 32-bit
 *                               masks; a thread follows its pair's prefix chain (forEachChainMember) and ORs the bit of every membership inside
 *                               the window into mask[rule - window], as the rules pass does.  What is this unit's is the decision on a touched
 *                               rule: `old` is built from the flow's bitmap over the rule's forward list -- at most 32 bit tests, for touched
 *                               rules only -- and the rule fires iff (old | new) == need && old != need: complete now, not before.  The
 *                               piece's count goes to pieceFiredFirst[k], 64-bit
 *   pfac_array_scan             the exclusive 64-bit scan of the counts in place, the total to the host
 *   pfac_flowrules_pass<true>   the same walk for the pieces with entries below `capacity`: the popcount prefix is the write position; nothing
 *                               is staged, nothing is written at or beyond capacity.  It reads the bitmaps the count pass read: nothing has
 *                               changed them
 *   (hipMemcpyAsync)            the first entries to the caller's array, where given
 *   pfac_flowrules_commit       ONLY when the host has seen that the list fits: for every pair and every id on its chain that has a bit, an
 *                               atomicOr into the flow's bitmap.  A block takes whole pieces, the flows of a call are distinct, so no two
 *                               blocks share a flow's words; behind the emit pass, which recomputes from the old state.  A truncated call
 *                               never launches it: no flow's state changes
 * SCRATCH (DeviceScratch::flowRules): 4 numPieces bytes for the flows of the pieces and 8 (numPieces + 1) bytes for the counts, each rounded up to
 * 256.  LDS of a block of the passes: 4 kFlowRulesWindow + kFlowRulesWindow / 8 + 2 kFlowRulesTouched + 28 bytes = 35 868 bytes: four blocks,
 * sixteen waves, on a compute unit's 160 KiB (profiles/flowrules_resources.txt).  The commit kernel uses no LDS.
 * Plain C++, vector stores, LDS and global atomics only.  The caller's device arrays are never trusted: a first pair is clamped to the pair list
 * where it is read, a decreasing pair is an empty piece, an id outside [1, numIds] is skipped before it indexes anything; the flows of the pieces
 * come from the host side, which has validated them.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_flowrules.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"

namespace {

constexpr unsigned int kFlowRulesBlockPairs = 256;                      /* pairs a block takes from a piece in one go: one per thread (pfac_amd/api.py: PFACX_FLOWRULES_BLOCK_PAIRS) */
constexpr unsigned int kFlowRulesWindowLog2 = 13;
constexpr unsigned int kFlowRulesWindow = 1u << kFlowRulesWindowLog2;   /* rules per window: 32 KiB of masks, four blocks per compute unit (PFACX_FLOWRULES_WINDOW) */
constexpr unsigned int kFlowRulesTouched = 1024;                        /* entries of the touched list (PFACX_FLOWRULES_TOUCHED) */

struct FlowRulesArgs {
    SegmentFrame f;                     /* the pairs' count, the pieces' first pairs, pieceFiredFirst, the capacity (scan_passes.h) */
    const int *pairIds;                 /* the longest pairs' ids */
    const unsigned int *flowIds;        /* [numPieces]: validated by the host side, uploaded into the call's scratch */
    const pfac::Int2 *table;            /* [numIds + 1] {prefixPattern, chainLen} by id */
    unsigned int numIds;
    const int *memberOff;               /* [numIds + 2] */
    const unsigned int *member;         /* rule << 5 | bit, ascending rule within a pattern */
    const int *ruleFirst;               /* [numRules + 1] */
    const unsigned int *ruleBits;       /* the forward list: member b of rule r is bit ruleBits[ruleFirst[r] + b] of a flow's bitmap */
    const int *bitOf;                   /* [numIds + 1]: the bit of a pattern, -1: none */
    unsigned int *flowBits;             /* numFlows x wordsPerFlow */
    unsigned int wordsPerFlow;
    int *firedPiece, *firedRule;
};

/* the frame of scan_passes.h (segmentWindows) over mask[]: a slot is the bits a rule's members set IN THIS CALL, decided -- against what the flow
 * has seen before -- and cleared where it is compared */
template <bool EMIT>
__global__ __launch_bounds__(kFlowRulesBlockPairs) void pfac_flowrules_pass(FlowRulesArgs a)
{
    __shared__ unsigned int mask[kFlowRulesWindow];
    const unsigned int *seen = a.flowBits;                                          /* the bitmap of the piece's flow */
    segmentWindows<EMIT, kFlowRulesWindowLog2, kFlowRulesTouched, kFlowRulesBlockPairs, false>(
        a.f, mask, [&](unsigned int k) { seen = a.flowBits + (size_t)a.flowIds[k] * a.wordsPerFlow; },
        [&](unsigned int i, unsigned int w0, auto touch, auto beyond) {
            forEachChainMember(a.table, a.numIds, a.pairIds[i], [&](int q) {
                unsigned int lo = (unsigned int)a.memberOff[q];
                const unsigned int end = (unsigned int)a.memberOff[q + 1];
                if (w0 != 0) {                                                      /* the first membership at or behind the window's first rule */
                    unsigned int hi = end;
                    while (lo < hi) {
                        const unsigned int mid = lo + (hi - lo) / 2;
                        if ((a.member[mid] >> 5) < w0) lo = mid + 1; else hi = mid;
                    }
                }
                for (; lo < end; lo++) {
                    const unsigned int m = a.member[lo], r = (m >> 5) - w0;
                    if (r >= kFlowRulesWindow) {
                        beyond((m >> 5) >> kFlowRulesWindowLog2);
                        break;
                    }
                    if (atomicOr(&mask[r], 1u << (m & 31u)) == 0u) touch(r);
                }
                return true;
            });
        },
        /* (a touched entry is not 0 and rule < numRules; a rule has 1 to 32 members) */
        [&](unsigned int fresh, unsigned int rule) {
            const unsigned int first = (unsigned int)a.ruleFirst[rule], n = (unsigned int)a.ruleFirst[rule + 1] - first;
            const unsigned int need = n >= 32u ? 0xFFFFFFFFu : (1u << n) - 1u;
            unsigned int old = 0;
            for (unsigned int b = 0; b < n && b < 32u; b++) {
                const unsigned int bit = a.ruleBits[first + b];
                old |= ((seen[bit >> 5] >> (bit & 31u)) & 1u) << b;
            }
            return (old | fresh) == need && old != need;
        },
        [&](unsigned long long o, unsigned int k, unsigned int rule, unsigned int) {
            a.firedPiece[o] = (int)k;
            a.firedRule[o] = (int)rule;
        });
}

/* the pieces' pairs into their flows' bitmaps; launched only where the whole list fitted */
__global__ __launch_bounds__(kFlowRulesBlockPairs) void pfac_flowrules_commit(FlowRulesArgs a)
{
    const unsigned int bitsPerFlow = a.wordsPerFlow * 32u;
    for (unsigned int k = blockIdx.x; k < a.f.numSegments; k += gridDim.x) {
        unsigned int first = clampFirstPair(a.f.segFirstPairs[k], a.f.count), last = clampFirstPair(a.f.segFirstPairs[k + 1], a.f.count);
        if (last < first) last = first;
        unsigned int *seen = a.flowBits + (size_t)a.flowIds[k] * a.wordsPerFlow;
        for (unsigned int i = first + threadIdx.x; i < last; i += kFlowRulesBlockPairs) {
            forEachChainMember(a.table, a.numIds, a.pairIds[i], [&](int q) {
                const int bit = a.bitOf[q];
                if (bit >= 0 && (unsigned int)bit < bitsPerFlow) {
                    const unsigned int w = 1u << ((unsigned int)bit & 31u);
                    if ((seen[(unsigned int)bit >> 5] & w) == 0u) atomicOr(&seen[(unsigned int)bit >> 5], w);
                }
                return true;
            });
        }
    }
}

} // namespace

extern "C" {

PFAC_status_t PFACX_flowRulesRun(PFAC_handle_t handle, const PFACX_flowRulesRun_t *run, size_t *h_total)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!run || !h_total || run->numPieces == 0 || run->numPieces >= (size_t)0x80000000u || run->count >= (size_t)0x80000000u ||
        run->numRules == 0 || run->numRules >= (size_t(1) << 24) || run->numIds >= (size_t)0x7fffffff || (run->count && !run->d_pairIds) ||
        !run->d_pieceFirst || !run->h_flowIds || !run->d_table || !run->d_memberOff || !run->d_member || !run->d_ruleFirst || !run->d_ruleBits ||
        !run->d_bitOf || !run->d_flowBits || run->numFlows == 0 || run->wordsPerFlow == 0 || run->wordsPerFlow >= (size_t(1) << 26) ||
        (run->capacity && (!run->d_firedPiece || !run->d_firedRule)))
        return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = handle;
    FlowRulesArgs a{};
    a.f.count = (unsigned int)run->count;
    a.f.segFirstPairs = run->d_pieceFirst;
    a.f.numSegments = (unsigned int)run->numPieces;
    a.f.capacity = run->capacity;
    a.pairIds = run->d_pairIds;
    a.table = static_cast<const pfac::Int2 *>(run->d_table);
    a.numIds = (unsigned int)run->numIds;
    a.memberOff = run->d_memberOff;
    a.member = run->d_member;
    a.ruleFirst = run->d_ruleFirst;
    a.ruleBits = run->d_ruleBits;
    a.bitOf = run->d_bitOf;
    a.flowBits = run->d_flowBits;
    a.wordsPerFlow = (unsigned int)run->wordsPerFlow;
    a.firedPiece = run->d_firedPiece;
    a.firedRule = run->d_firedRule;
    /* the flows of the pieces (the host side has validated them), then the counts */
    unsigned int *flowIds = nullptr;
    const PFAC_status_t carved = carveScratch(c->scratch.flowRules, [&](ScratchCarver &k) {
        flowIds = k.take<unsigned int>(a.f.numSegments);
        a.f.segFirst = k.take<unsigned long long>((size_t)a.f.numSegments + 1);
    });
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    if (hipMemcpyAsync(flowIds, run->h_flowIds, (size_t)a.f.numSegments * sizeof(unsigned int), hipMemcpyHostToDevice, nullptr) != hipSuccess)
        return PFAC_STATUS_INTERNAL_ERROR;
    a.flowIds = flowIds;
    const HostHandoff list(c, pfac::kHostFlowRules);
    if (!segmentWindowPasses(c, a, pfac_flowrules_pass<false>, pfac_flowrules_pass<true>, kFlowRulesBlockPairs, list, run->d_pieceFiredFirst))
        return PFAC_STATUS_INTERNAL_ERROR;
    unsigned long long total = 0;
    if (!list.finish(&total, a.f.segFirst + a.f.numSegments)) return PFAC_STATUS_INTERNAL_ERROR;
    if (total <= run->capacity && run->count != 0) {                                /* the list fits: the flows move on */
        const unsigned int grid = a.f.numSegments < gridCap(c, 8) ? a.f.numSegments : gridCap(c, 8);
        hipLaunchKernelGGL(pfac_flowrules_commit, dim3(grid), dim3(kFlowRulesBlockPairs), 0, 0, a);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
    }
    *h_total = (size_t)total;
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
