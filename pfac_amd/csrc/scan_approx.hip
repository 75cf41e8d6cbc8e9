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
 *                        skipped.  The distance d goes to mis[slot] here, in front of the frame's store: the emit's own slot and capacity
 *   pfac_host_done       the call's sequence number to mapped host memory (scan_passes.h: HostHandoff)
 * The walk along the chain (forEachChainMember), both passes, the capacity-checked store and the launches (expandPasses) are the expansion frame of
 * scan_passes.h, shared with scan_all.hip, scan_words.hip, scan_groups.hip, scan_case.hip and scan_sig.hip; this unit's own is the test of a
 * member (walkPair), the compare and the rule that keeps an occurrence once.
 * THE COMPARE works on dwords: the blob is dword-aligned and holds, per pattern, its bytes; the input side of dword w is composed from the two
 * aligned dwords around in[s + 4 w] with v_alignbyte, as in scan_sig.hip; x = in ^ pattern, the non-zero bytes of x are folded to one bit each
 * (differingBytes) and counted, and d > k is tested every 16 bytes: a candidate that is far off ends early.  An aligned dword that would reach
 * outside [0, n) -- in front of in[0] where the caller's pointer is misaligned and s < 3, behind in[n - 1] at the end -- is put together from its
 * bytes inside the buffer (three at most), and the L & 3 bytes behind the pattern's last whole dword are compared byte by byte.
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

namespace {

constexpr unsigned int kApproxBlock = 256;
constexpr unsigned int kApproxMaxBudget = 7;      /* pfac_ext.h: PFACX_APPROX_MAX_MISMATCHES */

struct ApproxArgs {
    ExpandFrame f;                      /* the pairs, the chain table, the block cut, the caller's arrays (scan_passes.h); f.all is not read */
    const unsigned char *in;            /* the caller's bytes */
    unsigned int n;
    const unsigned int *entryOff;       /* [numIds + 2] by piece id: the first entry of its class */
    const pfac::ApproxEntry *entries;   /* {pattern id, blobOff, start | L << 16, k | j << 8} */
    unsigned int numEntries;
    const uint32_t *blob;               /* per pattern: (L + 3) / 4 dwords of its bytes */
    unsigned int blobWords;
    unsigned int maxPiece;              /* a piece is the first min(part length, maxPiece) bytes of its part */
    int *mis;                           /* the distances, capacity entries, or null */
};

/* the aligned dword of the input whose first byte is in[o] (o: any sign; in + o is dword-aligned): one load where it lies inside [0, n), else its
 * bytes inside the buffer, zero for the others */
__device__ __forceinline__ uint32_t alignedDword(const ApproxArgs &a, long long o)
{
    if (o >= 0 && o + 4 <= (long long)a.n) return *reinterpret_cast<const uint32_t *>(a.in + o);
    uint32_t w = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const long long i = o + b;
        if (i >= 0 && i < (long long)a.n) w |= (uint32_t)a.in[i] << (8 * b);
    }
    return w;
}

/* the number of non-zero bytes of x: bit 7 of a byte is set iff its low seven bits carry into it or it is set itself, then a popcount */
__device__ __forceinline__ unsigned int differingBytes(uint32_t x)
{
    return (unsigned int)__popc((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u);
}

/* #{t < len : in[s + t] != pattern[t]}, or some value > budget where it is more than budget.  s + len <= n and the pattern's (len + 3) / 4
 * dwords at blob[off ...] lie inside the blob (the caller has checked both) */
__device__ __forceinline__ unsigned int distance(const ApproxArgs &a, unsigned int s, unsigned int len, unsigned int off, unsigned int budget)
{
    const unsigned int words = len >> 2, r = (unsigned int)(reinterpret_cast<uintptr_t>(a.in + s) & 3u);
    const uint32_t *val = a.blob + off;
    unsigned int d = 0;
    if (r == 0) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(a.in + s);       /* whole dwords inside [s, s + len) */
        for (unsigned int w = 0; w < words; w++) {
            d += differingBytes(src[w] ^ val[w]);
            if ((w & 3u) == 3u && d > budget) return d;
        }
    } else {
        const long long base = (long long)s - (long long)r;                     /* the aligned dword that holds in[s] */
        uint32_t lo = words ? alignedDword(a, base) : 0u;
        for (unsigned int w = 0; w < words; w++) {
            const uint32_t hi = alignedDword(a, base + 4ll * (w + 1u));
            d += differingBytes(__builtin_amdgcn_alignbyte(hi, lo, r) ^ val[w]);
            if ((w & 3u) == 3u && d > budget) return d;
            lo = hi;
        }
    }
    const unsigned int tail = len & 3u;
    if (tail) {
        const uint32_t v = val[words];
        for (unsigned int b = 0; b < tail; b++) d += ((uint32_t)a.in[s + 4u * words + b] ^ (v >> (8u * b))) & 0xFFu ? 1u : 0u;
    }
    return d;
}

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
        while (t < plen && a.in[s + from + t] == pat[from + t]) t++;
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
    if (p < 0 || (unsigned int)p >= a.n) return 0u;
    unsigned int found = 0;
    forEachChainMember(a.f.table, a.f.numIds, id, [&](int q) {
        const unsigned int first = a.entryOff[q];
        unsigned int end = a.entryOff[q + 1];
        if (end > a.numEntries) end = a.numEntries;
        for (unsigned int v = first; v < end; v++) {
            const pfac::ApproxEntry e = a.entries[v];
            const unsigned int start = e.startLen & 0xFFFFu, len = e.startLen >> 16, k = e.budgetPiece & 0xFFu, j = (e.budgetPiece >> 8) & 0xFFu;
            if (k > kApproxMaxBudget || j > k || len <= k || start > (unsigned int)p) continue;       /* s < 0: before any load */
            const unsigned int s = (unsigned int)p - start;
            if (len > a.n - s) continue;                                                             /* s + len > n */
            const unsigned int off = (unsigned int)e.blobOff, need = (len + 3u) >> 2;
            if (e.blobOff < 0 || off >= a.blobWords || a.blobWords - off < need) continue;           /* (a table of the library's own: never) */
            const unsigned int d = distance(a, s, len, off, k);
            if (d > k) continue;
            if (j != 0u && earlierPieceExact(a, s, len, k, j, off)) continue;                        /* a lower exact piece reports it */
            emit(e.id, (int)s, (int)d);
            found++;
        }
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
            (void)walkPair(a, i, [&](int id, int s, int d) {
                if (a.mis != nullptr && emit.o < emit.f.capacity) a.mis[emit.o] = d;                  /* the slot the frame's store takes next */
                emit(id, s);
            });
        });
}

} // namespace

extern "C" {

PFAC_status_t PFACX_approxRun(PFAC_handle_t handle, const PFACX_approxRun_t *run, size_t *h_total)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!run || !h_total || !run->d_input || run->size == 0 || run->size > (size_t)0x7fffffff || run->numIds > (size_t)0x7ffffffe || !run->d_entryOff ||
        !run->d_entries || run->numEntries > (size_t)0x7fffffff || run->blobWords > (size_t)0x7fffffff || !run->d_blob || run->maxPieceLen == 0 ||
        run->count > (size_t)0x7fffffff || (run->count && (!run->d_pairIds || !run->d_pairPos)) || (run->capacity && (!run->d_ids || !run->d_pos)))
        return PFAC_STATUS_INVALID_PARAMETER;
    *h_total = 0;
    if (run->count == 0) return PFAC_STATUS_SUCCESS;
    PFAC_context *c = handle;
    ApproxArgs a{};
    a.in = reinterpret_cast<const unsigned char *>(run->d_input);
    a.n = (unsigned int)run->size;
    a.entryOff = run->d_entryOff;
    a.entries = static_cast<const pfac::ApproxEntry *>(run->d_entries);
    a.numEntries = (unsigned int)run->numEntries;
    a.blob = run->d_blob;
    a.blobWords = (unsigned int)run->blobWords;
    a.maxPiece = (unsigned int)(run->maxPieceLen < (size_t)0xFFFF ? run->maxPieceLen : (size_t)0xFFFF);    /* no part is longer than a pattern */
    a.mis = run->capacity ? run->d_mis : nullptr;
    a.f = ExpandFrame{run->d_pairIds, run->d_pairPos, run->count, static_cast<const pfac::Int2 *>(run->d_table), (unsigned int)run->numIds,
                      1u, 0, nullptr, run->d_ids, run->d_pos, run->capacity};
    return expandPasses(c, c->scratch.approxSet, pfac::kHostApprox, a, pfac_approx_count, pfac_approx_write, kApproxBlock, a.f.capacity != 0, h_total);
}

} /* extern "C" */
