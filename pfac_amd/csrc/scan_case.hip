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
 * scan_passes.h, shared with scan_all.hip, scan_words.hip, scan_groups.hip and the other verify units; the compare and the head of PFACX_caseRun
 * are scan_verify.h's; this unit's own is the test of a member (walkPair) with its class loop, which ends the whole walk in list mode.
 * THE COMPARE (scan_verify.h: bytesEqual) works on dwords: the blob is dword-aligned, the input side of dword k is composed from the two aligned
 * dwords around in[p + 4 k] with v_alignbyte, the way pfac_fold<Q> composes a misaligned source; the differences are ORed up and tested every 16
 * bytes.
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
#include "scan_verify.h"

namespace {

constexpr unsigned int kCaseBlock = 256;
constexpr unsigned int kCaseTrivial = 0x80000000u;      /* bit 31 of varOff[q]: one caseless variant, reported as q */

struct CaseArgs {
    ExpandFrame f;                      /* the pairs, the chain table, PFACX_CASE_ALL, the block cut, the caller's arrays (scan_passes.h) */
    InputView v;                        /* the caller's bytes (scan_verify.h) */
    const int *patternLen;              /* [numIds + 1] by id */
    const unsigned int *varOff;         /* [numIds + 2] by id: first variant | kCaseTrivial */
    const pfac::Int2 *vars;             /* {line id, dword index into blob or -1} */
    unsigned int numVars;
    const uint32_t *blob;
    unsigned int blobWords;
};

/* The variants that hold along pair k's chain, longest member first, highest line id first within a member (scan_passes.h: forEachChainMember):
 * emit(line id) for each of them; returns their number (list mode: 0 or 1) */
template <class Emit>
__device__ __forceinline__ unsigned int walkPair(const CaseArgs &a, size_t k, Emit emit)
{
    const int id = a.f.pairIds[k], p = a.f.pairPos[k];
    if (p < 0 || (unsigned int)p >= a.v.n) return 0u;
    const unsigned int room = a.v.n - (unsigned int)p;
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
                if (!inBlob(a.blobWords, off, ((unsigned int)len + 3u) / 4u)) continue;                    /* (a table of the library's own: never) */
                if (!bytesEqual(a.v, a.blob + off, (unsigned int)p, (unsigned int)len)) continue;
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
    if (!run || !verifyRunOk(run->v, h_total) || !run->d_patternLen || !run->d_varOff || !run->d_vars || run->numVars > (size_t)0x7fffffff)
        return PFAC_STATUS_INVALID_PARAMETER;
    *h_total = 0;
    if (run->v.count == 0) return PFAC_STATUS_SUCCESS;
    PFAC_context *c = handle;
    CaseArgs a{};
    a.v = verifyInput(run->v);
    a.patternLen = run->d_patternLen;
    a.varOff = run->d_varOff;
    a.vars = static_cast<const pfac::Int2 *>(run->d_vars);
    a.numVars = (unsigned int)run->numVars;
    a.blob = run->v.d_blob;
    a.blobWords = (unsigned int)run->v.blobWords;
    a.f = verifyFrame(run->v, run->all ? 1u : 0u);
    return expandPasses(c, c->scratch.caseSet, pfac::kHostCase, a, pfac_case_count, pfac_case_write, kCaseBlock, a.f.capacity != 0, h_total);
}

} /* extern "C" */
