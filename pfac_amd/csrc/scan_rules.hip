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
 *
 * SETS WITH CHAINS (PFACX_rulesOpenSeq with a PFACX_RULE_RELATIVE member): pfac_rules_seq_pass<EMIT>, the conditioned pass plus a
 * verification between the decisions and the sweep (the frame's verify hook).  A relative member sets its bit like any conditioned one, so a rule with
 * mask == need is a CANDIDATE; one that has links (seqOff / seqLink, built by rules_api.cpp in the layout of pfac_context.h) is verified by the whole block over the segment's pairs,
 * link by link (chainsHold has the method and why it is exact), and its bit is cleared from the window's bitmap if a chain fails -- in both passes
 * alike, in front of the popcounts, so a failed candidate is an entry that never was and pass 2 writes where pass 1 counted.  Nothing is staged per
 * candidate or per fired entry.  The slots, the touched list and the bitmap return to their clean state on the frame's own paths; verification keeps
 * no state of its own between candidates but the two frontier arrays, which every link overwrites before it is read.
 * SCRATCH of such a call: 2 x round256(4 count) bytes behind segFirst, the two frontier arrays by pair.  LDS: 52 bytes more (a maximum per wave, a
 * ballot per wave): 35.08 KiB, still four blocks, sixteen waves, on a compute unit.  No input byte is read; the segment's bounds are the clamped ones
 * of the conditioned pass.  COST: in both passes candidates x links x pairs of the segment (a walk of the segment's pairs per link, a binary search
 * per occurrence): for records and packets, not for a common first member over a segment of many MiB.
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
    /* a set with chains (SEQ) only; all null for the others */
    const int *seqOff;                  /* [numRules + 1]: the links of rule r are seqLink[kSeqLinkWords seqOff[r], kSeqLinkWords seqOff[r + 1]) */
    const unsigned int *seqLink;        /* a link: id | kSeqFirst, the window as memberCond has it, distance, within */
    unsigned int *front[2];             /* [count] each: the frontier of the link in front and of the link at hand (chainsHold) */
};
using pfac::kCondFromEnd, pfac::kCondEnd, pfac::kSeqLinkWords, pfac::kSeqFirst;      /* pfac_context.h: the layout rules_api.cpp builds */
static_assert(sizeof(size_t) == sizeof(unsigned long long), "the caller's offsets are 64-bit");

/* segment bound k of a conditioned call: the caller's offset clamped to [0, size], as scan_batch.hip clamps it */
__device__ __forceinline__ int boundOf(const RulesArgs &a, unsigned int k)
{
    const unsigned long long o = a.offsets[k];
    return (int)(o < a.size ? (unsigned int)o : a.size);
}

/* SETS WITH CHAINS: does pair i's prefix chain hold pattern `id`?  (the walk of the pass: it ends after chainLen steps whatever the table says) */
__device__ __forceinline__ bool onPrefixChain(const RulesArgs &a, int q, int id)
{
    if (q < 1 || (unsigned int)q > a.numIds) return false;
    const int steps = a.table[q].y;
    for (int s = 0; s < (steps > 1 ? steps : 1) && q >= 1 && (unsigned int)q <= a.numIds; s++) {
        if (q == id) return true;
        q = a.table[q].x;
    }
    return false;
}

/* Do the chains a.seqLink[linkLo, linkHi) of one candidate rule all hold over the segment's pairs [first, last), bytes [segStart, segEnd)?  The
 * whole block calls it, behind a barrier, and gets the same answer.  Link by link, a walk over the pairs in trips of the block, pair per thread: an
 * occurrence of the link that satisfies its own window is REACHABLE if the link opens a chain or if, with hi = s - distance - lenPrev, the frontier
 * at the last pair whose position is <= hi (binary search: positions ascend) is >= s + len - within - lenPrev -- the frontier of pair j being the
 * largest start, plus 1, of a reachable occurrence of the link in front at or in front of pair j (0: none).  The largest start that is not too late
 * is the only one that needs asking: every other is further from s.  The link's own frontier -- a running maximum under the block prefix, with a
 * carry between the trips -- goes to the other of the two arrays a.front[], indexed by the pair: segments partition the pairs and a segment is one
 * block's, so no block meets another's entries.  A link nobody reaches fails its chain.  64-bit where distance and within enter: nothing wraps */
__device__ __forceinline__ bool chainsHold(const RulesArgs &a, unsigned int linkLo, unsigned int linkHi, unsigned int first, unsigned int last,
                                           int segStart, int segEnd, unsigned int *waveMax)
{
    const unsigned int t = threadIdx.x;
    unsigned int from = 0;                                                          /* a.front[from]: the frontier of the link in front */
    long long lenPrev = 0;
    for (unsigned int l = linkLo; l < linkHi; l++) {
        const unsigned int *link = a.seqLink + (size_t)l * kSeqLinkWords;
        const int id = (int)(link[0] & ~kSeqFirst);
        const bool opens = (link[0] & kSeqFirst) != 0;
        const unsigned int lo = link[1], hi = link[2];
        const long long distance = link[3], within = link[4];
        const int len = id >= 1 && (unsigned int)id <= a.numIds ? a.patternLen[id] : -1;
        const unsigned int *prev = a.front[from];
        unsigned int *next = a.front[from ^ 1u];
        unsigned int carry = 0;
        for (unsigned int i0 = first; i0 < last; i0 += kRulesBlockPairs) {          /* the same trip count for every thread */
            const unsigned int i = i0 + t;
            unsigned int v = 0;
            if (i < last && onPrefixChain(a, a.pairIds[i], id)) {
                const int p = a.pairPos[i], at = p - segStart, room = segEnd - p;
                const int tail = at < 0 || len < 0 || len > room ? -1 : room - len;
                const unsigned int w = (hi & kCondFromEnd) ? (unsigned int)tail : (unsigned int)at;
                if (tail >= 0 && w >= lo && w + (unsigned int)len <= (hi & kCondEnd)) {
                    if (opens) {
                        v = (unsigned int)p + 1u;
                    } else {
                        const long long high = (long long)p - distance - lenPrev;   /* the latest start of the link in front */
                        unsigned int x = first, y = i;                              /* the first pair of [first, i) behind high */
                        while (x < y) {
                            const unsigned int mid = x + (y - x) / 2;
                            if ((long long)a.pairPos[mid] <= high) x = mid + 1; else y = mid;
                        }
                        if (x > first) {
                            const long long low = within != 0 ? (long long)p + len - within - lenPrev : 0;
                            const long long reached = (long long)prev[x - 1u] - 1;
                            if (reached >= 0 && reached >= low) v = (unsigned int)p + 1u;
                        }
                    }
                }
            }
            unsigned int total = 0;
            const unsigned int before = blockExclusive<kRulesBlockPairs>(v, waveMax, total, OpMax());
            const unsigned int upTo = before > v ? before : v;
            if (i < last) next[i] = upTo > carry ? upTo : carry;
            carry = total > carry ? total : carry;
        }
        __syncthreads();                                                            /* the link's frontier is whole: the next link reads it */
        if (carry == 0) return false;                                               /* the same in every thread */
        from ^= 1u;
        lenPrev = len;
    }
    return true;
}

/* the frame of scan_passes.h (segmentWindows) over mask[]: a slot is a rule's mask, decided -- and cleared -- where it is compared with need[].
 * SEQ (with COND): the candidates of a window -- the bits of its bitmap -- that have links are verified in front of the sweep (chainsHold), the
 * words that are not zero found by a ballot, candidate after candidate by the whole block; thread 0 clears the bit of one that fails */
template <bool EMIT, bool COND, bool SEQ>
__device__ __forceinline__ void rulesPass(const RulesArgs &a, unsigned int *mask)
{
    int segStart = 0, segEnd = 0;                                                   /* COND: the segment's bytes [segStart, segEnd) of the buffer (size < 2^31) */
    const auto segment = [&](unsigned int k) {
        if constexpr (COND) {
            segStart = 0;
            segEnd = (int)a.size;
            if (a.offsets != nullptr) {
                segStart = boundOf(a, k);
                segEnd = boundOf(a, k + 1);
            }
        }
    };
    const auto pair = [&](unsigned int i, unsigned int w0, auto touch, auto beyond) {
        int q = a.pairIds[i];
        if (q < 1 || (unsigned int)q > a.numIds) return;
        const int steps = a.table[q].y;                                             /* the patterns on the chain, q included: the walk ends there whatever the table says */
        int at = 0, room = 0;                                                       /* COND: the pair's position in its segment, the bytes from there to the segment's end */
        if constexpr (COND) {
            const int p = a.pairPos[i];
            at = p - segStart;                                                      /* (both in [-2^31, 2^31): no wrap) */
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
            if (w0 != 0) {                                                          /* the first membership at or behind the window's first rule */
                unsigned int hi = end;
                while (lo < hi) {
                    const unsigned int mid = lo + (hi - lo) / 2;
                    if ((a.member[mid] >> 5) < w0) lo = mid + 1; else hi = mid;
                }
            }
            for (; lo < end; lo++) {
                const unsigned int m = a.member[lo], r = (m >> 5) - w0;
                if (r >= kRulesWindow) {
                    beyond((m >> 5) >> kRulesWindowLog2);                           /* whatever the window test says: the next window is visited */
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
    };
    /* (need[] is never 0: an untouched entry cannot fire; rule < numRules where the mask is not 0) */
    const auto decide = [&](unsigned int m, unsigned int rule) { return m == a.need[rule]; };
    const auto emit = [&](unsigned long long o, unsigned int k, unsigned int rule, unsigned int) {
        a.firedSeg[o] = (int)k;
        a.firedRule[o] = (int)rule;
    };
    if constexpr (SEQ) {
        __shared__ unsigned int waveMax[kRulesBlockPairs / 64];
        __shared__ unsigned long long wordsSet[kRulesBlockPairs / 64];
        const auto verify = [&](unsigned int *bits, unsigned int w0, unsigned int first, unsigned int last) {
            const unsigned int t = threadIdx.x;
            const unsigned long long set = __ballot(bits[t] != 0u);
            if ((t & 63u) == 0) wordsSet[t >> 6] = set;
            __syncthreads();
            for (unsigned int wave = 0; wave < kRulesBlockPairs / 64; wave++) {
                for (unsigned long long words = wordsSet[wave]; words != 0; words &= words - 1ull) {
                    const unsigned int w = wave * 64u + (unsigned int)__ffsll((long long)words) - 1u;
                    for (unsigned int word = bits[w]; word != 0; word &= word - 1u) {           /* read in front of chainsHold's barriers, cleared behind them */
                        const unsigned int b = (unsigned int)__ffs((int)word) - 1u, rule = w0 + w * 32u + b;
                        const unsigned int linkLo = (unsigned int)a.seqOff[rule], linkHi = (unsigned int)a.seqOff[rule + 1];
                        if (linkLo >= linkHi) continue;                             /* a candidate without chains: decided already */
                        if (!chainsHold(a, linkLo, linkHi, first, last, segStart, segEnd, waveMax) && t == 0) bits[w] &= ~(1u << b);
                    }
                }
            }
            __syncthreads();
        };
        segmentWindows<EMIT, kRulesWindowLog2, kRulesTouched, kRulesBlockPairs, false>(a.f, mask, segment, pair, decide, emit, verify);
    } else {
        segmentWindows<EMIT, kRulesWindowLog2, kRulesTouched, kRulesBlockPairs, false>(a.f, mask, segment, pair, decide, emit);
    }
}

template <bool EMIT, bool COND>
__global__ __launch_bounds__(kRulesBlockPairs) void pfac_rules_pass(RulesArgs a)
{
    __shared__ unsigned int mask[kRulesWindow];
    rulesPass<EMIT, COND, false>(a, mask);
}

/* what a set with chains launches */
template <bool EMIT>
__global__ __launch_bounds__(kRulesBlockPairs) void pfac_rules_seq_pass(RulesArgs a)
{
    __shared__ unsigned int mask[kRulesWindow];
    rulesPass<EMIT, true, true>(a, mask);
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
    const bool seq = run->d_seqOff != nullptr;
    if (seq && (!cond || !run->d_seqLink)) return PFAC_STATUS_INVALID_PARAMETER;
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
    if (seq) {
        a.seqOff = run->d_seqOff;
        a.seqLink = run->d_seqLink;
    }
    /* a set with chains: the two frontier arrays behind segFirst, 4 bytes per pair each; the others take what they always have */
    const PFAC_status_t carved = !seq ? carveSegFirst(c->scratch.rules, a.f, 0) : carveScratch(c->scratch.rules, [&](ScratchCarver &k) {
        a.f.segFirst = k.take<unsigned long long>((size_t)a.f.numSegments + 1);
        a.front[0] = k.take<unsigned int>(a.f.count);
        a.front[1] = k.take<unsigned int>(a.f.count);
    });
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    const HostHandoff list(c, pfac::kHostRules);
    /* a plain set and a conditioned one launch what they always have */
    const auto count = seq ? pfac_rules_seq_pass<false> : cond ? pfac_rules_pass<false, true> : pfac_rules_pass<false, false>;
    const auto emit = seq ? pfac_rules_seq_pass<true> : cond ? pfac_rules_pass<true, true> : pfac_rules_pass<true, false>;
    if (!segmentWindowPasses(c, a, count, emit, kRulesBlockPairs, list, run->d_segFirst)) return PFAC_STATUS_INTERNAL_ERROR;
    unsigned long long total = 0;
    if (!list.finish(&total, a.f.segFirst + a.f.numSegments)) return PFAC_STATUS_INTERNAL_ERROR;
    *h_total = (size_t)total;
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
