/*
 * scan_case.hip -- per-pattern case sensitivity over a caseless set (include/pfac_ext.h: PFACX_case*): of the lines whose folded
 * bytes a caseless handle found at a position, the ones that occur there by their own flag -- a caseless line always, a sensitive line where the
 * caller's bytes equal its original bytes.
 *
 * Every pattern of the caseless set that starts at p is a prefix of the longest one L that starts there, so the candidates at p are L's prefix
 * chain (scan_all.hip), and the lines behind a member q are the VARIANTS of its class: the caseless lines of that folded text as one variant, the
 * sensitive lines by their exact bytes, duplicates collapsed, highest line id first (case_api.cpp builds the tables).  The passes work on an ordered
 * list of LONGEST pairs -- the handle's pair scratch behind PFACX_allReduce, or a list of the caller's -- and look at the input again:
 *   pfac_case_count      a thread per pair: the chain from the longest member down, for each member its variants from the highest id down; a
 *                        caseless variant holds, a sensitive one where in[p, p + len) equals its bytes of the blob (bytesEqual).  The value of a
 *                        pair is 0 / 1 in list mode (the walk stops at the first variant that holds: the longest pattern, the highest id) and the
 *                        number of variants that hold in ALL mode; the block's total goes to blockBase[block] (scan_passes.h: expandCount)
 *   pfac_array_scan      exclusive scan of the block totals (one block; 64-bit), the length of the list to mapped host memory
 *   pfac_case_write      the block's pairs again (expandWrite): each thread walks its chain once more and hands the line id of every variant that
 *                        holds to the frame, which writes (id, p) into consecutive slots; slots >= capacity are skipped
 *   pfac_host_done       the call's sequence number to mapped host memory (scan_passes.h: HostHandoff)
 * The walk along the chain (forEachChainMember), both passes, the capacity-checked store and the launches (expandPasses) are the expansion frame of
 * scan_passes.h, shared with scan_all.hip, scan_words.hip and scan_groups.hip; this unit's own is the test of a member (walkPair) and the compare.
 * THE COMPARE works on dwords: the blob is dword-aligned, the input side of dword k is composed from the two aligned dwords around in[p + 4 k] with
 * v_alignbyte, the way pfac_fold<Q> composes a misaligned source; the differences are ORed up and tested every 16 bytes.  An aligned dword that
 * would reach outside [0, n) -- in front of in[0] where the caller's pointer is misaligned and p < 3, behind in[n - 1] at the end -- is put
 * together from its bytes inside the buffer (three at most), and so are the len & 3 bytes behind the pattern's last whole dword.
 * Every index into the input is checked against [0, n) before the load; an id outside [1, F] is a pair that counts nothing, a member that does not
 * lie inside the input is not kept, a walk ends after chainLen steps whatever the table says, and a class's variant range is clamped to the table:
 * a caller's list cannot make a pass read or write outside the buffers.  A thread per pair: a long sensitive pattern keeps its lane busy while
 * the others of its wave wait (DESIGN.md 5u says what would even that out).
 * SCRATCH: 8 (blocks + 1) bytes rounded up to 256 (DeviceScratch::caseSet), blocks = one per 256 pairs, eight per compute unit at most.
 * Plain C++ and vector stores only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_case.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"

namespace {

constexpr unsigned int kCaseBlock = 256;
constexpr unsigned int kCaseTrivial = 0x80000000u;      /* bit 31 of varOff[q]: one caseless variant, reported as q */

struct CaseArgs {
    ExpandFrame f;                      /* the pairs, the chain table, PFACX_CASE_ALL, the block cut, the caller's arrays (scan_passes.h) */
    const unsigned char *in;            /* the caller's bytes: never the folded copy */
    unsigned int n;
    const int *patternLen;              /* [numIds + 1] by id */
    const unsigned int *varOff;         /* [numIds + 2] by id: first variant | kCaseTrivial */
    const pfac::Int2 *vars;             /* {line id, dword index into blob or -1} */
    unsigned int numVars;
    const uint32_t *blob;
    unsigned int blobWords;
};

/* the aligned dword of the input whose first byte is in[o] (o: any sign; in + o is dword-aligned): one load where it lies inside [0, n), else its
 * bytes inside the buffer, zero for the others */
__device__ __forceinline__ uint32_t alignedDword(const CaseArgs &a, long long o)
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

/* in[p, p + len) == the len bytes at blob[off ...]?  p + len <= n and the pattern's dwords lie inside the blob (the caller has checked both) */
__device__ __forceinline__ bool bytesEqual(const CaseArgs &a, unsigned int p, unsigned int len, unsigned int off)
{
    const unsigned int words = len >> 2, r = (unsigned int)(reinterpret_cast<uintptr_t>(a.in + p) & 3u);
    const uint32_t *pat = a.blob + off;
    uint32_t diff = 0;
    if (r == 0) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(a.in + p);       /* whole dwords inside [p, p + len) */
        for (unsigned int k = 0; k < words; k++) {
            diff |= src[k] ^ pat[k];
            if ((k & 3u) == 3u && diff != 0) return false;
        }
    } else {
        const long long base = (long long)p - (long long)r;                     /* the aligned dword that holds in[p] */
        uint32_t lo = words ? alignedDword(a, base) : 0u;
        for (unsigned int k = 0; k < words; k++) {
            const uint32_t hi = alignedDword(a, base + 4ll * (k + 1u));
            diff |= __builtin_amdgcn_alignbyte(hi, lo, r) ^ pat[k];
            if ((k & 3u) == 3u && diff != 0) return false;
            lo = hi;
        }
    }
    if (diff != 0) return false;
    const unsigned int tail = len & 3u;
    if (tail) {
        const uint32_t last = pat[words];
        for (unsigned int b = 0; b < tail; b++)
            if (a.in[p + 4u * words + b] != (unsigned char)(last >> (8u * b))) return false;
    }
    return true;
}

/* The variants that hold along pair k's chain, longest member first, highest line id first within a member (scan_passes.h: forEachChainMember):
 * emit(line id) for each of them; returns their number (list mode: 0 or 1) */
template <class Emit>
__device__ __forceinline__ unsigned int walkPair(const CaseArgs &a, size_t k, Emit emit)
{
    const int id = a.f.pairIds[k], p = a.f.pairPos[k];
    if (p < 0 || (unsigned int)p >= a.n) return 0u;
    const unsigned int room = a.n - (unsigned int)p;
    unsigned int found = 0;
    forEachChainMember(a.f.table, a.f.numIds, id, [&](int q) {
        const int len = a.patternLen[q];
        if (len <= 0 || (unsigned int)len > room) return true;
        const unsigned int first = a.varOff[q];
        if (first & kCaseTrivial) {
            emit(q);
            found++;
            return a.f.all != 0u;
        }
        unsigned int end = a.varOff[q + 1] & ~kCaseTrivial;
        if (end > a.numVars) end = a.numVars;
        for (unsigned int v = first; v < end; v++) {
            const pfac::Int2 var = a.vars[v];
            if (var.y >= 0) {
                const unsigned int off = (unsigned int)var.y;
                if (off >= a.blobWords || a.blobWords - off < ((unsigned int)len + 3u) / 4u) continue;     /* (a table of the library's own: never) */
                if (!bytesEqual(a, (unsigned int)p, (unsigned int)len, off)) continue;
            }
            emit(var.x);
            found++;
            if (a.f.all == 0u) return false;
        }
        return true;
    });
    return found;
}

__global__ __launch_bounds__(kCaseBlock) void pfac_case_count(CaseArgs a)
{
    expandCount<kCaseBlock>(a.f, [&](size_t k) -> unsigned long long { return walkPair(a, k, [](int) {}); });
}

__global__ __launch_bounds__(kCaseBlock) void pfac_case_write(CaseArgs a)
{
    expandWrite<kCaseBlock>(
        a.f, [&](size_t k) -> unsigned long long { return walkPair(a, k, [](int) {}); },
        [&](size_t k, auto emit) { (void)walkPair(a, k, emit); });
}

} // namespace

extern "C" {

PFAC_status_t PFACX_caseRun(PFAC_handle_t handle, const PFACX_caseRun_t *run, size_t *h_total)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!run || !h_total || !run->d_input || run->size == 0 || run->size > (size_t)0x7fffffff || !run->d_patternLen || run->numIds > (size_t)0x7ffffffe ||
        !run->d_varOff || !run->d_vars || run->numVars > (size_t)0x7fffffff || run->blobWords > (size_t)0x7fffffff || (run->blobWords && !run->d_blob) ||
        run->count > (size_t)0x7fffffff || (run->count && (!run->d_pairIds || !run->d_pairPos)) || (run->capacity && (!run->d_ids || !run->d_pos)))
        return PFAC_STATUS_INVALID_PARAMETER;
    *h_total = 0;
    if (run->count == 0) return PFAC_STATUS_SUCCESS;
    PFAC_context *c = handle;
    CaseArgs a{};
    a.in = reinterpret_cast<const unsigned char *>(run->d_input);
    a.n = (unsigned int)run->size;
    a.patternLen = run->d_patternLen;
    a.varOff = run->d_varOff;
    a.vars = static_cast<const pfac::Int2 *>(run->d_vars);
    a.numVars = (unsigned int)run->numVars;
    a.blob = run->d_blob;
    a.blobWords = (unsigned int)run->blobWords;
    a.f = ExpandFrame{run->d_pairIds, run->d_pairPos, run->count, static_cast<const pfac::Int2 *>(run->d_table), (unsigned int)run->numIds,
                      run->all ? 1u : 0u, 0, nullptr, run->d_ids, run->d_pos, run->capacity};
    return expandPasses(c, c->scratch.caseSet, pfac::kHostCase, a, pfac_case_count, pfac_case_write, kCaseBlock, a.f.capacity != 0, h_total);
}

} /* extern "C" */
