/*
 * scan_rules.hip -- rule sets (include/pfac_ext.h: PFACX_rules*): which segments of a batch contain every pattern of a rule.
 *
 * Pattern id occurs in segment k iff it lies on the prefix chain (Automaton::prefixPattern) of one of the segment's LONGEST pairs, so the fired list
 * follows from the ordered compacted batch scan (the pairs and the first pair of each segment, in handle scratch), the {prefixPattern, chainLen} table
 * of the all-match calls and the rule set inverted by pattern: memberOff / member (rule << 5 | bit, ascending rule) and need[rule], the full mask.
 * Nothing here is sized by segments x rules:
 *
 *   pfac_rules_pass<false>   segmentWindows of scan_passes.h -- a block takes whole segments and walks a segment's pairs once per WINDOW of
 *                            kRulesWindow rules it touches; the touched list, nextWindow, the bitmap and its sweep are the frame's -- over
 *                            mask[kRulesWindow], a direct-indexed LDS table of 32-bit masks.  What is this unit's: a thread follows its pair's prefix
 *                            chain and, for every membership of a pattern on it that lies in the window (the first by binary search: they ascend), ORs
 *                            the bit into mask[rule - window] with an LDS atomic; whoever finds the entry zero touches it; the first membership BEHIND
 *                            the window is handed to the frame (beyond).  A touched entry with mask == need[rule] is an entry of the list, and every
 *                            touched entry is cleared where it is compared (RESET_IN_SWEEP == false: a window in which nothing fired is not swept).
 *                            The segment's count goes to segFirst[k], 64-bit
 *   pfac_array_scan          the exclusive 64-bit scan of the counts in place (scan_passes.h): segFirst[numSegments + 1], the total to the host
 *   pfac_rules_pass<true>    the same walk for every segment that fired something below `capacity` (all others leave at once): the popcount
 *                            prefix is the write position, ascending rule order within the segment without a sort; nothing at or beyond capacity
 *   (hipMemcpyAsync)         segFirst to the caller's array, where given
 *   pfac_host_done           the call's sequence number to mapped host memory (scan_passes.h: HostHandoff)
 * Pass 2 recomputes what pass 1 found instead of staging it: a staged list would be as long as the fired list, which has no bound the caller has not
 * set.  The launches are segmentWindowPasses (scan_passes.h).
 * SCRATCH: 8 (numSegments + 1) bytes rounded up to 256 (DeviceScratch::rules).  LDS of a block: 4 kRulesWindow + kRulesWindow / 8 + 2 kRulesTouched
 * + 48 bytes = 35.05 KiB: four blocks, sixteen waves, on a compute unit's 160 KiB.
 * Plain C++, vector stores and LDS atomics only; for a plain set the caller's offsets are not read here (scan_batch.hip has clamped them into the
 * first pairs, which are clamped to the pair list again where they are read).
 *
 * CONDITIONED SETS (PFACX_rulesOpenEx): pfac_rules_pass<EMIT, COND>.  COND == false is the code above and what a plain set launches.
 * With COND a membership has a window memberCond[j] = {offset, end | direction} and a polarity that lives in need[] alone (the positive bits: mask ==
 * need says "every positive member, no negated one").  The walk loads the segment's bounds once per segment (the caller's offsets clamped to [0, size];
 * none: 0 and size), the pair's position once per pair and patternLen[q] once per member of its chain, and ORs a membership's bit only if THAT member
 * lies inside the segment and satisfies the window -- the longest pattern at a position can fail a window its proper prefix passes.  No input byte is
 * read.  nextWindow is lowered in front of the test: a later window can hold a rule this pair completes or vetoes.  Windows, the touched list and its
 * sweep, the bitmap, the emit, pass 2 and the clean state are the same code; a failed test touches nothing.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_rules.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"

namespace {

constexpr unsigned int kRulesBlockPairs = 256;                          /* pairs a block takes from a segment in one go: one per thread (pfac_amd/api.py: PFACX_RULES_BLOCK_PAIRS) */
constexpr unsigned int kRulesWindowLog2 = 13;
constexpr unsigned int kRulesWindow = 1u << kRulesWindowLog2;           /* rules per window: 32 KiB of masks, four blocks per compute unit (PFACX_RULES_WINDOW) */
constexpr unsigned int kRulesTouched = 1024;                            /* entries of the touched list (PFACX_RULES_TOUCHED) */

struct RulesArgs {
    SegmentFrame f;                     /* the pairs' count, the segments' first pairs, segFirst, the capacity (scan_passes.h) */
    const int *pairIds;                 /* the ordered longest pairs' ids */
    const pfac::Int2 *table;            /* [numIds + 1] {prefixPattern, chainLen} by id */
    unsigned int numIds;
    const int *memberOff;               /* [numIds + 2] */
    const unsigned int *member;         /* rule << 5 | bit, ascending rule within a pattern */
    const unsigned int *need;           /* [numRules] */
    unsigned int numRules;
    int *firedSeg, *firedRule;
    /* a conditioned set (COND) only; all null or 0 for a plain one */
    const int *pairPos;                 /* the pairs' positions in the buffer */
    const unsigned long long *offsets;  /* [numSegments + 1] bytes, clamped to [0, size] where read; null: one segment [0, size) */
    unsigned int size;
    const int *patternLen;              /* [numIds + 1] by id */
    const uint2 *memberCond;            /* indexed like member: x the window's offset, y its end (bits 0 .. 30, saturated) and kCondFromEnd */
};
constexpr unsigned int kCondFromEnd = 0x80000000u, kCondEnd = 0x7FFFFFFFu;
static_assert(sizeof(size_t) == sizeof(unsigned long long), "the caller's offsets are 64-bit");

/* segment bound k of a conditioned call: the caller's offset clamped to [0, size], as scan_batch.hip clamps it */
__device__ __forceinline__ int boundOf(const RulesArgs &a, unsigned int k)
{
    const unsigned long long o = a.offsets[k];
    return (int)(o < a.size ? (unsigned int)o : a.size);
}

/* the frame of scan_passes.h (segmentWindows) over mask[]: a slot is a rule's mask, decided -- and cleared -- where it is compared with need[] */
template <bool EMIT, bool COND>
__global__ __launch_bounds__(kRulesBlockPairs) void pfac_rules_pass(RulesArgs a)
{
    __shared__ unsigned int mask[kRulesWindow];
    int segStart = 0, segEnd = 0;                                                   /* COND: the segment's bytes [segStart, segEnd) of the buffer (size < 2^31) */
    segmentWindows<EMIT, kRulesWindowLog2, kRulesTouched, kRulesBlockPairs, false>(
        a.f, mask,
        [&](unsigned int k) {
            if constexpr (COND) {
                segStart = 0;
                segEnd = (int)a.size;
                if (a.offsets != nullptr) {
                    segStart = boundOf(a, k);
                    segEnd = boundOf(a, k + 1);
                }
            }
        },
        [&](unsigned int i, unsigned int w0, auto touch, auto beyond) {
            int q = a.pairIds[i];
            if (q < 1 || (unsigned int)q > a.numIds) return;
            const int steps = a.table[q].y;                                         /* the patterns on the chain, q included: the walk ends there whatever the table says */
            int at = 0, room = 0;                                                   /* COND: the pair's position in its segment, the bytes from there to the segment's end */
            if constexpr (COND) {
                const int p = a.pairPos[i];
                at = p - segStart;                                                  /* (both in [-2^31, 2^31): no wrap) */
                room = segEnd - p;
            }
            for (int s = 0; s < (steps > 1 ? steps : 1) && q >= 1 && (unsigned int)q <= a.numIds; s++) {
                /* COND: the member of the chain by itself -- the bytes behind it in the segment; negative (or at < 0): it does not lie inside,
                 * and satisfies nothing.  Inside, at + len <= segEnd - segStart < 2^31: the sums below do not wrap */
                int len = 0, tail = -1;
                if constexpr (COND) {
                    len = a.patternLen[q];
                    tail = at < 0 || len < 0 || len > room ? -1 : room - len;
                }
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
                    if (r >= kRulesWindow) {
                        beyond((m >> 5) >> kRulesWindowLog2);                       /* whatever the window test says: the next window is visited */
                        break;
                    }
                    if constexpr (COND) {
                        const uint2 c = a.memberCond[lo];
                        const unsigned int from = (c.y & kCondFromEnd) ? (unsigned int)tail : (unsigned int)at;
                        if (tail < 0 || from < c.x || from + (unsigned int)len > (c.y & kCondEnd)) continue;
                    }
                    if (atomicOr(&mask[r], 1u << (m & 31u)) == 0u) touch(r);
                }
                q = a.table[q].x;
            }
        },
        /* (need[] is never 0: an untouched entry cannot fire; rule < numRules where the mask is not 0) */
        [&](unsigned int m, unsigned int rule) { return m == a.need[rule]; },
        [&](unsigned long long o, unsigned int k, unsigned int rule, unsigned int) {
            a.firedSeg[o] = (int)k;
            a.firedRule[o] = (int)rule;
        });
}

} // namespace

extern "C" {

PFAC_status_t PFACX_rulesRun(PFAC_handle_t handle, const PFACX_rulesRun_t *run, size_t *h_total)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!run || !h_total || run->numSegments == 0 || run->numSegments >= (size_t)0x80000000u || run->count >= (size_t)0x80000000u ||
        run->numRules == 0 || run->numRules >= (size_t(1) << 24) || run->numIds >= (size_t)0x7fffffff || (run->count && !run->d_pairIds) ||
        !run->d_table || !run->d_memberOff || !run->d_member || !run->d_need || (run->capacity && (!run->d_firedSeg || !run->d_firedRule)))
        return PFAC_STATUS_INVALID_PARAMETER;
    const bool cond = run->d_memberCond != nullptr;
    if (cond && ((run->count && !run->d_pairPos) || !run->d_patternLen || run->size >= (size_t)0x80000000u)) return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = handle;
    RulesArgs a{};
    a.f.count = (unsigned int)run->count;
    a.f.segFirstPairs = run->d_segFirstPairs;
    a.f.numSegments = (unsigned int)run->numSegments;
    a.f.capacity = run->capacity;
    a.pairIds = run->d_pairIds;
    a.table = static_cast<const pfac::Int2 *>(run->d_table);
    a.numIds = (unsigned int)run->numIds;
    a.memberOff = run->d_memberOff;
    a.member = run->d_member;
    a.need = run->d_need;
    a.numRules = (unsigned int)run->numRules;
    a.firedSeg = run->d_firedSeg;
    a.firedRule = run->d_firedRule;
    if (cond) {
        a.pairPos = run->d_pairPos;
        a.offsets = reinterpret_cast<const unsigned long long *>(run->d_offsets);
        a.size = (unsigned int)run->size;
        a.patternLen = run->d_patternLen;
        a.memberCond = reinterpret_cast<const uint2 *>(run->d_memberCond);
    }
    const PFAC_status_t carved = carveSegFirst(c->scratch.rules, a.f, 0);
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    const HostHandoff list(c, pfac::kHostRules);
    const auto count = cond ? pfac_rules_pass<false, true> : pfac_rules_pass<false, false>;       /* a plain set launches what it always has */
    const auto emit = cond ? pfac_rules_pass<true, true> : pfac_rules_pass<true, false>;
    if (!segmentWindowPasses(c, a, count, emit, kRulesBlockPairs, list, run->d_segFirst)) return PFAC_STATUS_INTERNAL_ERROR;
    unsigned long long total = 0;
    if (!list.finish(&total, a.f.segFirst + a.f.numSegments)) return PFAC_STATUS_INTERNAL_ERROR;
    *h_total = (size_t)total;
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
