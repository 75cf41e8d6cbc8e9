/*
 * scan_approx.hip -- patterns matched within k mismatches (include/pfac_ext.h: PFACX_approx*): a pattern of L bytes with budget k
 * occurs at s where at most k of its bytes differ from the caller's input (substitutions only); the handle's patterns are the PIECES -- the
 * pattern is cut into k + 1 disjoint parts, of which at least one is exact at any occurrence, and a piece is the head of a part --, and of the
 * patterns one of whose pieces a scan found, the ones whose distance holds in the caller's input.
 *
 * Every piece that starts at p is a prefix of the longest one that starts there, so the candidates at p are the longest one's prefix chain
 * (scan_all.hip), and behind a member q stands its CLASS: the (pattern, piece) entries whose piece string is q, highest pattern id first, then
 * highest piece index first (approx_api.cpp builds the tables).  The passes work on an ordered list of LONGEST pairs -- the handle's pair scratch
 * behind PFACX_allReduce, or a list of the caller's -- and look at the input again:
 *   pfac_approx_count    a thread per pair: the chain from the longest member down, for each member the entries of its class in table order;
 *                        entry {id, blobOff, start | L << 16, k | j << 8} starts at s = p - start, is dropped where s < 0 or s + L > n before
 *                        any load, and holds where d = #{t : in[s + t] != pattern[t]} <= k (distance) and no piece j' < j of the pattern is
 *                        exact at s (earlierPieceExact): an occurrence is found once per exact piece and kept by the LOWEST one alone.  The value
 *                        of a pair is the number of entries that hold; the block's total goes to blockBase[block] (scan_passes.h: expandCount)
 *   pfac_array_scan      exclusive scan of the block totals (one block; 64-bit), the length of the list to mapped host memory
 *   pfac_approx_write    the block's pairs again (expandWrite): each thread walks its chain once more and hands (pattern id, s) of every entry
 *                        that holds to the frame (ExpandEmit with a position), which writes them into consecutive slots; slots >= capacity are
 *                        skipped.  The distance d goes to mis[slot] in front of the frame's store (scan_verify.h: emitWithAux)
 *   pfac_host_done       the call's sequence number to mapped host memory (scan_passes.h: HostHandoff)
 * The walk along the chain (forEachChainMember), both passes, the capacity-checked store and the launches (expandPasses) are the expansion frame of
 * scan_passes.h, shared with scan_all.hip, scan_words.hip, scan_groups.hip and the other verify units; the class loop, the compare, the store of
 * the third array and the head of PFACX_approxRun are scan_verify.h's; this unit's own is the test of a member (walkPair) and the rule that keeps
 * an occurrence once.
 * THE COMPARE (scan_verify.h: byteDistance) works on dwords: the blob is dword-aligned and holds, per pattern, its bytes; x = in ^ pattern, the
 * non-zero bytes of x are folded to one bit each (differingBytes) and counted, and d > k is tested every 16 bytes: a candidate that is far off
 * ends early.
 * THE PARTS follow from L and k: part j' is [j' L / (k + 1), (j' + 1) L / (k + 1)), its piece the first min(part length, maxPiece) bytes; the
 * test of the earlier pieces runs only behind a distance that holds, byte by byte inside [s, s + L), which the bounds test has put inside [0, n).
 * Every index into the input is checked against [0, n) before the load; an id outside [1, F] is a pair that counts nothing, a walk ends after
 * chainLen steps whatever the table says, a class's range is clamped to the table and an entry whose dwords do not lie inside the blob is skipped:
 * a caller's list cannot make a pass read or write outside the buffers.  A thread per pair: a long pattern, or a class of many, keeps its lane
 * busy while the others of its wave wait, and short pieces over a small alphabet make candidates frequent (DESIGN.md 5w says what that costs).
 * SCRATCH: 8 (blocks + 1) bytes rounded up to 256 (DeviceScratch::approxSet), blocks = one per 256 pairs, eight per compute unit at most.
 * Plain C++ and vector stores only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_approx.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"
#include "scan_verify.h"

namespace {

constexpr unsigned int kApproxBlock = 256;
constexpr unsigned int kApproxMaxBudget = 7;      /* pfac_ext.h: PFACX_APPROX_MAX_MISMATCHES */

struct ApproxArgs {
    ExpandFrame f;                      /* the pairs, the chain table, the block cut, the caller's arrays (scan_passes.h); f.all is not read */
    InputView v;                        /* the caller's bytes (scan_verify.h) */
    const unsigned int *entryOff;       /* [numIds + 2] by piece id: the first entry of its class */
    const pfac::ApproxEntry *entries;   /* {pattern id, blobOff, start | L << 16, k | j << 8} */
    unsigned int numEntries;
    const uint32_t *blob;               /* per pattern: (L + 3) / 4 dwords of its bytes */
    unsigned int blobWords;
    unsigned int maxPiece;              /* a piece is the first min(part length, maxPiece) bytes of its part */
    int *mis;                           /* the distances, capacity entries, or null */
};

/* is a piece j' < j of the pattern {len, budget k, bytes at blob[off ...]} exact at start s?  [s, s + len) lies inside [0, n) */
__device__ __forceinline__ bool earlierPieceExact(const ApproxArgs &a, unsigned int s, unsigned int len, unsigned int k, unsigned int j, unsigned int off)
{
    const unsigned char *pat = reinterpret_cast<const unsigned char *>(a.blob + off);
    unsigned int from = 0;
    for (unsigned int e = 0; e < j; e++) {
        const unsigned int to = (e + 1u) * len / (k + 1u);
        unsigned int plen = to - from;
        if (plen > a.maxPiece) plen = a.maxPiece;
        unsigned int t = 0;
        while (t < plen && a.v.in[s + from + t] == pat[from + t]) t++;
        if (t == plen) return true;
        from = to;
    }
    return false;
}

/* The entries that hold along pair i's chain, longest piece first, table order (pattern id descending, then piece index descending) within a
 * piece (scan_passes.h: forEachChainMember): emit(pattern id, start, distance) for each of them; returns their number */
template <class Emit>
__device__ __forceinline__ unsigned int walkPair(const ApproxArgs &a, size_t i, Emit emit)
{
    const int id = a.f.pairIds[i], p = a.f.pairPos[i];
    if (p < 0 || (unsigned int)p >= a.v.n) return 0u;
    unsigned int found = 0;
    forEachChainMember(a.f.table, a.f.numIds, id, [&](int q) {
        forEachClassEntry(a.entryOff, a.numEntries, q, [&](unsigned int v) {
            const pfac::ApproxEntry e = a.entries[v];
            const unsigned int start = e.startLen & 0xFFFFu, len = e.startLen >> 16, k = e.budgetPiece & 0xFFu, j = (e.budgetPiece >> 8) & 0xFFu;
            if (k > kApproxMaxBudget || j > k || len <= k || start > (unsigned int)p) return;         /* s < 0: before any load */
            const unsigned int s = (unsigned int)p - start;
            if (len > a.v.n - s) return;                                                             /* s + len > n */
            const unsigned int off = (unsigned int)e.blobOff;
            if (e.blobOff < 0 || !inBlob(a.blobWords, off, (len + 3u) >> 2)) return;                 /* (a table of the library's own: never) */
            const unsigned int d = byteDistance(a.v, a.blob + off, s, len, k);
            if (d > k) return;
            if (j != 0u && earlierPieceExact(a, s, len, k, j, off)) return;                          /* a lower exact piece reports it */
            emit(e.id, (int)s, (int)d);
            found++;
        });
        return true;
    });
    return found;
}

__global__ __launch_bounds__(kApproxBlock) void pfac_approx_count(ApproxArgs a)
{
    expandCount<kApproxBlock>(a.f, [&](size_t i) -> unsigned long long { return walkPair(a, i, [](int, int, int) {}); });
}

__global__ __launch_bounds__(kApproxBlock) void pfac_approx_write(ApproxArgs a)
{
    expandWrite<kApproxBlock>(
        a.f, [&](size_t i) -> unsigned long long { return walkPair(a, i, [](int, int, int) {}); },
        [&](size_t i, auto emit) {
            (void)walkPair(a, i, [&](int id, int s, int d) { emitWithAux(emit, id, s, a.mis, d); });
        });
}

} // namespace

extern "C" {

PFAC_status_t PFACX_approxRun(PFAC_handle_t handle, const PFACX_approxRun_t *run, size_t *h_total)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!run || !verifyRunOk(run->v, h_total) || !run->v.d_blob || !run->d_entryOff || !run->d_entries || run->numEntries > (size_t)0x7fffffff ||
        run->maxPieceLen == 0)
        return PFAC_STATUS_INVALID_PARAMETER;
    *h_total = 0;
    if (run->v.count == 0) return PFAC_STATUS_SUCCESS;
    PFAC_context *c = handle;
    ApproxArgs a{};
    a.v = verifyInput(run->v);
    a.entryOff = run->d_entryOff;
    a.entries = static_cast<const pfac::ApproxEntry *>(run->d_entries);
    a.numEntries = (unsigned int)run->numEntries;
    a.blob = run->v.d_blob;
    a.blobWords = (unsigned int)run->v.blobWords;
    a.maxPiece = (unsigned int)(run->maxPieceLen < (size_t)0xFFFF ? run->maxPieceLen : (size_t)0xFFFF);    /* no part is longer than a pattern */
    a.mis = run->v.capacity ? run->d_mis : nullptr;
    a.f = verifyFrame(run->v);
    return expandPasses(c, c->scratch.approxSet, pfac::kHostApprox, a, pfac_approx_count, pfac_approx_write, kApproxBlock, a.f.capacity != 0, h_total);
}

} /* extern "C" */
