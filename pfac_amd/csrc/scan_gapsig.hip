/*
 * scan_gapsig.hip -- signatures with bounded gaps between parts (include/pfac_ext.h: PFACX_gapsig*): a signature is a sequence of
 * PARTS, each a fixed-length string of (value, mask) bytes as a signature of scan_sig.hip is, with a gap of lo .. hi arbitrary bytes between part j and part
 * j + 1; the handle's patterns are the ANCHORS -- one fully specified run inside one part of each signature --, and of the signatures whose anchor
 * a scan found, the (signature, start) for which a choice of gap widths exists under which every part holds in the caller's input, each listed
 * once, with the smallest end over all such choices.
 *
 * Every anchor that starts at p is a prefix of the longest one that starts there, so the candidates at p are the longest one's prefix chain
 * (scan_all.hip), and behind a member q stands its CLASS: the signatures that chose q as their anchor, highest signature id first, each {id, first
 * part, number of parts | anchor part << 16, offset of the anchor inside that part}; a part is {len, blobOff, lo, hi} (gapsig_api.cpp builds the
 * tables).  The passes work on an ordered list of LONGEST pairs -- the handle's pair scratch behind PFACX_allReduce, or a list of the caller's --
 * and look at the input again:
 *   pfac_gapsig_count    a thread per pair: the chain from the longest member down, for each member the signatures of its class in table order,
 *                        for each signature the search below.  The value of a pair is the number of (signature, start) it OWNS; the block's
 *                        total goes to blockBase[block] (scan_passes.h: expandCount)
 *   pfac_array_scan      exclusive scan of the block totals (one block; 64-bit), the length of the list to mapped host memory
 *   pfac_gapsig_write    the block's pairs again (expandWrite): each thread runs the same search once more -- one function, so both passes
 *                        decide alike -- and hands (signature id, start) to the frame (ExpandEmit with a position); the end goes to end[slot]
 *                        in front of the frame's store (scan_verify.h: emitWithAux)
 *   pfac_host_done       the call's sequence number to mapped host memory (scan_passes.h: HostHandoff)
 * The walk along the chain, both passes, the capacity-checked store and the launches are the expansion frame of scan_passes.h, shared with
 * scan_all.hip, scan_words.hip, scan_groups.hip and the other verify units; the class loop, the compare and the head of PFACX_gapsigRun are
 * scan_verify.h's; this unit's own is the search (searchSignature).
 * THE SEARCH.  The slack of a signature, the sum of hi - lo over its gaps, is at most 63, so where a part can lie relative to its TIGHTEST offset
 * (every gap in between at lo) is a set of at most 64 distances: one 64-bit mask.  A step from a part to its neighbour smears the mask by the
 * gap's hi - lo (shift-and-OR doubling: smear) and keeps the bits at which the neighbour holds (holdsWhere: a compare per set bit; a bit whose
 * part would leave [0, n) is dropped before any load).  With the anchor part a at x = p - anchorOff (x < 0: nothing, before any load):
 *   1. backwards from part a at {x} to part 0: bit t = t bytes in front of the tightest offset.  The bits of part 0 are the candidate starts
 *   2. for each start s, ascending: forwards from part 0 at {s} to part a: bit t = t bytes behind the tightest offset.  The bits A of part a are
 *      where part a can lie over a head that holds; x is among them
 *   3. forwards through the parts behind a, ONE walk with three masks over the same compares: `all` from A, `lt` from the bits of A below x, `eq`
 *      from x alone.  Behind the last part: eq empty -- no embedding at s has part a at x --, or lt not empty -- one has it at a smaller offset, and
 *      the pair there owns (id, s) --: nothing.  Else (id, s) is this pair's, and its end is the lowest bit of `all`: every embedding at s has part
 *      a at an offset of A, none below x completes, so `all` holds every end there is
 * Every loop is bounded by the tables' own limits: at most 64 parts, at most 64 bits, at most 64 starts.
 * THE COMPARE of a part is the bounds-safe masked dword compare that scan_sig.hip uses (scan_verify.h: maskedEqual): the input side composed
 * with v_alignbyte, edge dwords assembled from the bytes inside the buffer, the len & 3 bytes behind the last whole dword byte by byte.
 * Every index into the input is checked against [0, n) before the load; an id outside [1, F] is a pair that counts nothing, a walk ends after
 * chainLen steps whatever the table says, class and part ranges are clamped to their tables, a part whose dwords do not lie inside the blob
 * holds nowhere: a caller's list cannot make a pass read or write outside the buffers.  A thread per pair: DESIGN.md 5x says what that costs.
 * SCRATCH: 8 (blocks + 1) bytes rounded up to 256 (DeviceScratch::gapsigSet), blocks = one per 256 pairs, eight per compute unit at most.
 * Plain C++ and vector stores only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_gapsig.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"
#include "scan_verify.h"

namespace {

constexpr unsigned int kGapSigBlock = 256;
constexpr unsigned int kGapSigMaxParts = 64;      /* pfac_ext.h: a signature has at most this many parts */
constexpr unsigned int kGapSigMaxSlack = 63;      /* pfac_ext.h: PFACX_GAPSIG_MAX_SLACK */

struct GapSigArgs {
    ExpandFrame f;                      /* the pairs, the chain table, the block cut, the caller's arrays (scan_passes.h); f.all is not read */
    InputView v;                        /* the caller's bytes (scan_verify.h) */
    const unsigned int *sigOff;         /* [numIds + 2] by anchor id: the first signature of its class */
    const pfac::GapSigEntry *sigs;      /* {signature id, first part, parts | anchor part << 16, anchorOff} */
    unsigned int numSigs;
    const pfac::GapSigPart *parts;      /* {len, blobOff, lo, hi} */
    unsigned int numParts;
    const uint32_t *blob;               /* per part: (len + 3) / 4 value dwords, then as many mask dwords */
    unsigned int blobWords;
    int *end;                           /* the ends, capacity entries, or null */
};

/* the OR of m << k for k = 0 .. w (w <= 63; bits pushed past bit 63 are gone): what a gap of width lo .. lo + w does to the distances of a part */
__device__ __forceinline__ uint64_t smear(uint64_t m, unsigned int w)
{
    unsigned int c = 1;                                   /* m holds the shifts 0 .. c - 1 */
    while (2u * c <= w + 1u) {
        m |= m << c;
        c *= 2u;
    }
    return m | m << (w + 1u - c);                         /* w + 1 - c <= c: no hole */
}

/* is the gap behind part q one that a search may take?  (a table of the library's own: always) */
__device__ __forceinline__ bool gapUsable(const pfac::GapSigPart &q) { return q.hi >= q.lo && q.hi - q.lo <= kGapSigMaxSlack; }

/* the bits t of m at which part q holds at offset base + dir * t: inside [0, n) -- tested before any load -- and every masked byte equal.  A
 * part that is empty or whose dwords do not lie inside the blob holds nowhere */
__device__ __forceinline__ uint64_t holdsWhere(const GapSigArgs &a, const pfac::GapSigPart &q, long long base, int dir, uint64_t m)
{
    const unsigned int len = q.len, need = 2u * ((len + 3u) >> 2);
    if (len == 0u || len > 0xFFFFu || !inBlob(a.blobWords, q.blobOff, need)) return 0ull;
    uint64_t held = 0;
    while (m != 0ull) {                                   /* at most 64 rounds */
        const int t = __builtin_ctzll(m);
        m &= m - 1ull;
        const long long o = base + (long long)dir * t;
        if (o < 0 || o + (long long)len > (long long)a.v.n) continue;
        if (maskedEqual(a.v, a.blob + q.blobOff, (unsigned int)o, len)) held |= 1ull << t;
    }
    return held;
}

/* The (start, end) that the pair at p owns of signature e (the header says how): emit(e.id, start, end) for each, starts ascending; returns
 * their number */
template <class Emit>
__device__ __forceinline__ unsigned int searchSignature(const GapSigArgs &a, const pfac::GapSigEntry &e, int p, Emit emit)
{
    const unsigned int count = e.partsAnchor & 0xFFFFu, anchor = e.partsAnchor >> 16;
    if (count < 1u || count > kGapSigMaxParts || anchor >= count || e.firstPart >= a.numParts || a.numParts - e.firstPart < count) return 0u;
    if (e.anchorOff > (unsigned int)p) return 0u;                                                    /* x < 0: before any load */
    const pfac::GapSigPart *parts = a.parts + e.firstPart;
    const long long x = (long long)p - (long long)e.anchorOff;
    /* 1. backwards: bit t of `back` = the part lies t bytes in front of `tight`, its offset with every gap up to part a at lo */
    uint64_t back = holdsWhere(a, parts[anchor], x, -1, 1ull);
    long long tight = x;
    for (unsigned int j = anchor; j > 0u && back != 0ull; j--) {
        const pfac::GapSigPart q = parts[j - 1u];
        if (!gapUsable(q)) return 0u;
        tight -= (long long)q.len + (long long)q.lo;
        back = holdsWhere(a, q, tight, -1, smear(back, q.hi - q.lo));
    }
    unsigned int found = 0;
    while (back != 0ull) {                                                                           /* the starts, ascending: the highest bit first */
        const int tb = 63 - __builtin_clzll(back);
        back &= ~(1ull << tb);
        const long long s = tight - tb;
        /* 2. forwards to part a: bit t = the part lies t bytes behind `at`, its offset with every gap from part 0 at lo */
        uint64_t all = 1ull;
        long long at = s;
        for (unsigned int j = 0; j < anchor && all != 0ull; j++) {
            const pfac::GapSigPart q = parts[j];
            at += (long long)q.len + (long long)q.lo;
            all = holdsWhere(a, parts[j + 1u], at, 1, smear(all, q.hi - q.lo));
        }
        const long long tx = x - at;
        if (tx < 0 || tx > 63) continue;                                                             /* (x is reachable from s: never) */
        uint64_t eq = all & (1ull << tx), lt = all & ((1ull << tx) - 1ull);
        /* 3. forwards to the last part: all, below x, x alone */
        for (unsigned int j = anchor; j + 1u < count && eq != 0ull; j++) {
            const pfac::GapSigPart q = parts[j];
            if (!gapUsable(q)) { eq = 0ull; break; }
            const unsigned int w = q.hi - q.lo;
            at += (long long)q.len + (long long)q.lo;
            all = holdsWhere(a, parts[j + 1u], at, 1, smear(all, w));
            lt = smear(lt, w) & all;
            eq = smear(eq, w) & all;
        }
        if (eq == 0ull || lt != 0ull) continue;                                                      /* not on an embedding at s, or not the first */
        emit(e.id, (int)s, (int)(at + __builtin_ctzll(all) + (long long)parts[count - 1u].len));
        found++;
    }
    return found;
}

/* What pair k owns along its chain, longest anchor first, table order (signature id descending) within an anchor (scan_passes.h:
 * forEachChainMember), starts ascending within a signature: emit(signature id, start, end) for each; returns their number */
template <class Emit>
__device__ __forceinline__ unsigned int walkPair(const GapSigArgs &a, size_t k, Emit emit)
{
    const int id = a.f.pairIds[k], p = a.f.pairPos[k];
    if (p < 0 || (unsigned int)p >= a.v.n) return 0u;
    unsigned int found = 0;
    forEachChainMember(a.f.table, a.f.numIds, id, [&](int q) {
        forEachClassEntry(a.sigOff, a.numSigs, q, [&](unsigned int v) { found += searchSignature(a, a.sigs[v], p, emit); });
        return true;
    });
    return found;
}

__global__ __launch_bounds__(kGapSigBlock) void pfac_gapsig_count(GapSigArgs a)
{
    expandCount<kGapSigBlock>(a.f, [&](size_t k) -> unsigned long long { return walkPair(a, k, [](int, int, int) {}); });
}

__global__ __launch_bounds__(kGapSigBlock) void pfac_gapsig_write(GapSigArgs a)
{
    expandWrite<kGapSigBlock>(
        a.f, [&](size_t k) -> unsigned long long { return walkPair(a, k, [](int, int, int) {}); },
        [&](size_t k, auto emit) {
            (void)walkPair(a, k, [&](int id, int s, int end) { emitWithAux(emit, id, s, a.end, end); });
        });
}

} // namespace

extern "C" {

PFAC_status_t PFACX_gapsigRun(PFAC_handle_t handle, const PFACX_gapsigRun_t *run, size_t *h_total)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!run || !verifyRunOk(run->v, h_total) || !run->v.d_blob || !run->d_sigOff || !run->d_sigs || run->numSigs > (size_t)0x7fffffff || !run->d_parts ||
        run->numParts > (size_t)0x7fffffff)
        return PFAC_STATUS_INVALID_PARAMETER;
    *h_total = 0;
    if (run->v.count == 0) return PFAC_STATUS_SUCCESS;
    PFAC_context *c = handle;
    GapSigArgs a{};
    a.v = verifyInput(run->v);
    a.sigOff = run->d_sigOff;
    a.sigs = static_cast<const pfac::GapSigEntry *>(run->d_sigs);
    a.numSigs = (unsigned int)run->numSigs;
    a.parts = static_cast<const pfac::GapSigPart *>(run->d_parts);
    a.numParts = (unsigned int)run->numParts;
    a.blob = run->v.d_blob;
    a.blobWords = (unsigned int)run->v.blobWords;
    a.end = run->v.capacity ? run->d_end : nullptr;
    a.f = verifyFrame(run->v);
    return expandPasses(c, c->scratch.gapsigSet, pfac::kHostGapSig, a, pfac_gapsig_count, pfac_gapsig_write, kGapSigBlock, a.f.capacity != 0, h_total);
}

} /* extern "C" */
