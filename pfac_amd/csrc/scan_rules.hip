/*
 * scan_rules.hip -- rule sets (include/pfac_ext.h: PFACX_rules*): which segments of a batch contain every pattern of a rule.
 *
 * Pattern id occurs in segment k iff it lies on the prefix chain (Automaton::prefixPattern) of one of the segment's LONGEST pairs, so the fired list
 * follows from the ordered compacted batch scan (the pairs and the first pair of each segment, in handle scratch), the {prefixPattern, chainLen} table
 * of the all-match calls and the rule set inverted by pattern: memberOff / member (rule << 5 | bit, ascending rule) and need[rule], the full mask.
 * Nothing here is sized by segments x rules:
 *
 *   pfac_rules_pass<false>   a block takes whole segments, k = blockIdx.x, + gridDim.x, ...  It keeps in LDS a direct-indexed table mask[kRulesWindow]
 *                            of 32-bit masks, a fired bitmap of kRulesWindow bits and a list of kRulesTouched touched table entries; rules
 *                            [w kRulesWindow, (w + 1) kRulesWindow) are WINDOW w.  For a window the block walks the segment's pairs, kRulesBlockPairs
 *                            a trip, one per thread; a thread follows its pair's prefix chain and, for every membership of a pattern on it that
 *                            lies in the window (the first by binary search: they ascend), ORs the bit into mask[rule - window] with an LDS
 *                            atomic; whoever finds the entry zero appends it to the touched list (a list that overflows only counts on: the sweep
 *                            below then covers the whole table).  The first membership BEHIND the window lowers nextWindow (LDS atomic minimum):
 *                            the block goes on with the next window any pair of the segment has a membership in, so a segment costs the windows
 *                            it touches, not numRules / kRulesWindow.  Then: touched entries with mask == need[rule] set their bit in the fired
 *                            bitmap, every touched entry is cleared; the bitmap's words are swept in order, one per thread -- popcounts under a
 *                            block prefix give the number of fired rules -- and cleared on the way.  The segment's count goes to counts[k], 64-bit
 *   pfac_array_scan          the exclusive 64-bit scan of the counts in place (scan_passes.h): segFirst[numSegments + 1], the total to the host
 *   pfac_rules_pass<true>    the same walk for every segment that fired something below `capacity` (all others leave at once): the popcount
 *                            prefix is the write position, ascending rule order within the segment without a sort; nothing at or beyond capacity
 *   (hipMemcpyAsync)         segFirst to the caller's array, where given
 *   pfac_host_done           the call's sequence number to mapped host memory (scan_passes.h: HostHandoff)
 * Pass 2 recomputes what pass 1 found instead of staging it: a staged list would be as long as the fired list, which has no bound the caller has not
 * set.  Whatever path a segment takes -- touched list, overflow sweep, truncation, no touch at all -- mask[], the bitmap, the touched count and
 * nextWindow are as the kernel's prologue left them when the segment ends.
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
constexpr unsigned int kRulesWords = kRulesWindow / 32;                 /* words of the fired bitmap */
constexpr unsigned int kNoWindow = 0xFFFFFFFFu;
static_assert(kRulesWords == kRulesBlockPairs, "the emit sweep gives every thread one word of the bitmap");
static_assert(kRulesWindow <= 65536, "the touched list holds 16-bit table indices");

struct RulesArgs {
    const int *pairIds;                 /* the ordered longest pairs' ids */
    unsigned int count;
    const int *segFirstPairs;           /* [numSegments + 1], clamped where read; null: one segment of all pairs */
    unsigned int numSegments;
    const pfac::Int2 *table;            /* [numIds + 1] {prefixPattern, chainLen} by id */
    unsigned int numIds;
    const int *memberOff;               /* [numIds + 2] */
    const unsigned int *member;         /* rule << 5 | bit, ascending rule within a pattern */
    const unsigned int *need;           /* [numRules] */
    unsigned int numRules;
    unsigned long long *segFirst;       /* [numSegments + 1]: pass 1 writes the counts, the scan turns them into the first fired pair of each segment */
    int *firedSeg, *firedRule;
    unsigned long long capacity;
    /* a conditioned set (COND) only; all null or 0 for a plain one */
    const int *pairPos;                 /* the pairs' positions in the buffer */
    const unsigned long long *offsets;  /* [numSegments + 1] bytes, clamped to [0, size] where read; null: one segment [0, size) */
    unsigned int size;
    const int *patternLen;              /* [numIds + 1] by id */
    const uint2 *memberCond;            /* indexed like member: x the window's offset, y its end (bits 0 .. 30, saturated) and kCondFromEnd */
};
constexpr unsigned int kCondFromEnd = 0x80000000u, kCondEnd = 0x7FFFFFFFu;
static_assert(sizeof(size_t) == sizeof(unsigned long long), "the caller's offsets are 64-bit");

/* the first pair of segment k among the `count` pairs */
__device__ __forceinline__ unsigned int firstPairOf(const RulesArgs &a, unsigned int k)
{
    const int f = a.segFirstPairs[k];
    return f < 0 ? 0u : ((unsigned int)f < a.count ? (unsigned int)f : a.count);
}

/* segment bound k of a conditioned call: the caller's offset clamped to [0, size], as scan_batch.hip clamps it */
__device__ __forceinline__ int boundOf(const RulesArgs &a, unsigned int k)
{
    const unsigned long long o = a.offsets[k];
    return (int)(o < a.size ? (unsigned int)o : a.size);
}

template <bool EMIT, bool COND>
__global__ __launch_bounds__(kRulesBlockPairs) void pfac_rules_pass(RulesArgs a)
{
    __shared__ unsigned int mask[kRulesWindow];
    __shared__ unsigned int firedBits[kRulesWords];
    __shared__ unsigned short touched[kRulesTouched];
    __shared__ unsigned int waveSum[kRulesBlockPairs / 64];
    __shared__ unsigned int numTouched, anyFired, nextWindow;
    const unsigned int t = threadIdx.x;
    for (unsigned int i = t; i < kRulesWindow; i += kRulesBlockPairs) mask[i] = 0;
    firedBits[t] = 0;
    if (t == 0) {
        numTouched = 0;
        anyFired = 0;
        nextWindow = kNoWindow;
    }
    __syncthreads();

    for (unsigned int k = blockIdx.x; k < a.numSegments; k += gridDim.x) {          /* (numSegments < 2^31: k + gridDim.x does not wrap) */
        unsigned long long base = 0;
        if constexpr (EMIT) {
            base = a.segFirst[k];
            if (a.segFirst[k + 1] == base || base >= a.capacity) continue;          /* nothing fired here, or nothing of it fits: the whole block leaves */
        }
        unsigned int first = 0, last = a.count;
        if (a.segFirstPairs != nullptr) {
            first = firstPairOf(a, k);
            last = firstPairOf(a, k + 1);
            if (last < first) last = first;                                         /* hostile offsets: an empty segment */
        }
        int segStart = 0, segEnd = 0;                                               /* COND: the segment's bytes [segStart, segEnd) of the buffer (size < 2^31) */
        if constexpr (COND) {
            segEnd = (int)a.size;
            if (a.offsets != nullptr) {
                segStart = boundOf(a, k);
                segEnd = boundOf(a, k + 1);
            }
        }
        unsigned int fired = 0;                                                     /* of this segment so far: the same in every thread */
        unsigned int window = first < last ? 0u : kNoWindow;
        while (window != kNoWindow) {
            const unsigned int w0 = window << kRulesWindowLog2;
            for (unsigned int i = first + t; i < last; i += kRulesBlockPairs) {
                int q = a.pairIds[i];
                if (q < 1 || (unsigned int)q > a.numIds) continue;
                const int steps = a.table[q].y;                                     /* the patterns on the chain, q included: the walk ends there whatever the table says */
                int at = 0, room = 0;                                               /* COND: the pair's position in its segment, the bytes from there to the segment's end */
                if constexpr (COND) {
                    const int p = a.pairPos[i];
                    at = p - segStart;                                              /* (both in [-2^31, 2^31): no wrap) */
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
                    if (w0 != 0) {                                                  /* the first membership at or behind the window's first rule */
                        unsigned int hi = end;
                        while (lo < hi) {
                            const unsigned int mid = lo + (hi - lo) / 2;
                            if ((a.member[mid] >> 5) < w0) lo = mid + 1; else hi = mid;
                        }
                    }
                    for (; lo < end; lo++) {
                        const unsigned int m = a.member[lo], r = (m >> 5) - w0;
                        if (r >= kRulesWindow) {
                            atomicMin(&nextWindow, (m >> 5) >> kRulesWindowLog2);  /* whatever the window test says: the next window is visited */
                            break;
                        }
                        if constexpr (COND) {
                            const uint2 c = a.memberCond[lo];
                            const unsigned int from = (c.y & kCondFromEnd) ? (unsigned int)tail : (unsigned int)at;
                            if (tail < 0 || from < c.x || from + (unsigned int)len > (c.y & kCondEnd)) continue;
                        }
                        if (atomicOr(&mask[r], 1u << (m & 31u)) == 0u) {
                            const unsigned int slot = atomicAdd(&numTouched, 1u);
                            if (slot < kRulesTouched) touched[slot] = (unsigned short)r;
                        }
                    }
                    q = a.table[q].x;
                }
            }
            __syncthreads();
            const unsigned int n = numTouched, next = nextWindow;
            if (n != 0) {
                if (n <= kRulesTouched) {
                    for (unsigned int j = t; j < n; j += kRulesBlockPairs) {
                        const unsigned int r = touched[j];
                        if (mask[r] == a.need[w0 + r]) {
                            atomicOr(&firedBits[r >> 5], 1u << (r & 31u));
                            anyFired = 1u;
                        }
                        mask[r] = 0;
                    }
                } else {                                                            /* more entries than the list holds: every entry of the table */
                    for (unsigned int r = t; r < kRulesWindow; r += kRulesBlockPairs) {
                        const unsigned int m = mask[r];
                        if (m == 0) continue;                                       /* (need[] is never 0: an untouched entry cannot fire; w0 + r < numRules where m != 0) */
                        if (m == a.need[w0 + r]) {
                            atomicOr(&firedBits[r >> 5], 1u << (r & 31u));
                            anyFired = 1u;
                        }
                        mask[r] = 0;
                    }
                }
                __syncthreads();
                if (anyFired != 0) {                                                /* the same in every thread: read behind the barrier, reset behind the next */
                    unsigned int word = firedBits[t];
                    firedBits[t] = 0;
                    unsigned int total = 0;
                    const unsigned int before = blockExclusive<kRulesBlockPairs>((unsigned int)__popc(word), waveSum, total);
                    if constexpr (EMIT) {
                        unsigned long long o = base + fired + before;
                        while (word != 0 && o < a.capacity) {
                            const unsigned int bit = (unsigned int)__ffs((int)word) - 1u;
                            word &= word - 1u;
                            a.firedSeg[o] = (int)k;
                            a.firedRule[o] = (int)(w0 + t * 32u + bit);
                            o++;
                        }
                    }
                    fired += total;
                }
            }
            __syncthreads();                                                        /* everyone has read the three words */
            if (t == 0) {
                numTouched = 0;
                anyFired = 0;
                nextWindow = kNoWindow;
            }
            __syncthreads();
            window = next;
        }
        if constexpr (!EMIT) {
            if (t == 0) a.segFirst[k] = fired;
        }
    }
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
    a.pairIds = run->d_pairIds;
    a.count = (unsigned int)run->count;
    a.segFirstPairs = run->d_segFirstPairs;
    a.numSegments = (unsigned int)run->numSegments;
    a.table = static_cast<const pfac::Int2 *>(run->d_table);
    a.numIds = (unsigned int)run->numIds;
    a.memberOff = run->d_memberOff;
    a.member = run->d_member;
    a.need = run->d_need;
    a.numRules = (unsigned int)run->numRules;
    a.firedSeg = run->d_firedSeg;
    a.firedRule = run->d_firedRule;
    a.capacity = run->capacity;
    if (cond) {
        a.pairPos = run->d_pairPos;
        a.offsets = reinterpret_cast<const unsigned long long *>(run->d_offsets);
        a.size = (unsigned int)run->size;
        a.patternLen = run->d_patternLen;
        a.memberCond = reinterpret_cast<const uint2 *>(run->d_memberCond);
    }
    const PFAC_status_t carved = carveScratch(c->scratch.rules, [&](ScratchCarver &k) { a.segFirst = k.take<unsigned long long>(run->numSegments + 1); });
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    const unsigned int grid = a.numSegments < gridCap(c, 4) ? a.numSegments : gridCap(c, 4);
    const HostHandoff list(c, pfac::kHostRules);
    const auto count = cond ? pfac_rules_pass<false, true> : pfac_rules_pass<false, false>;       /* a plain set launches what it always has */
    const auto emit = cond ? pfac_rules_pass<true, true> : pfac_rules_pass<true, false>;
    hipLaunchKernelGGL(count, dim3(grid), dim3(kRulesBlockPairs), 0, 0, a);
    hipLaunchKernelGGL(pfac_array_scan<unsigned long long>, dim3(1), dim3(1024), 0, 0, a.segFirst, a.numSegments, a.segFirst + a.numSegments,
                       reinterpret_cast<unsigned long long *>(list.d_value));
    if (run->capacity) hipLaunchKernelGGL(emit, dim3(grid), dim3(kRulesBlockPairs), 0, 0, a);
    if (run->d_segFirst != nullptr &&
        hipMemcpyAsync(run->d_segFirst, a.segFirst, (run->numSegments + 1) * sizeof(unsigned long long), hipMemcpyDeviceToDevice, nullptr) != hipSuccess)
        return PFAC_STATUS_INTERNAL_ERROR;
    unsigned long long total = 0;
    if (!list.finish(&total, a.segFirst + a.numSegments)) return PFAC_STATUS_INTERNAL_ERROR;
    *h_total = (size_t)total;
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
