/*
 * scan_sig.hip -- masked byte signatures (include/pfac_ext.h: PFACX_sig*): a signature is a fixed-length string of (value, mask)
 * bytes, the handle's patterns are the ANCHORS -- one fully specified run of each signature --, and of the signatures whose anchor a scan found,
 * the ones whose every masked byte holds in the caller's input.
 *
 * Every anchor that starts at p is a prefix of the longest one L that starts there, so the candidates at p are L's prefix chain (scan_all.hip), and
 * behind a member q stand the signatures of its CLASS: the signatures that chose q as their anchor, each with the offset of the anchor inside it,
 * highest signature id first (sig_api.cpp builds the tables).  The passes work on an ordered list of LONGEST pairs -- the handle's pair scratch
 * behind PFACX_allReduce, or a list of the caller's -- and look at the input again:
 *   pfac_sig_count       a thread per pair: the chain from the longest member down, for each member the signatures of its class in table order;
 *                        signature {id, anchorOff, len, blobOff} starts at s = p - anchorOff, is dropped where s < 0 or s + len > n before any
 *                        load, and holds where ((in[s + k] ^ value[k]) & mask[k]) == 0 for every k (maskedEqual).  The value of a pair is the
 *                        number of signatures that hold; the block's total goes to blockBase[block] (scan_passes.h: expandCount)
 *   pfac_array_scan      exclusive scan of the block totals (one block; 64-bit), the length of the list to mapped host memory
 *   pfac_sig_write       the block's pairs again (expandWrite): each thread walks its chain once more and hands (signature id, s) of every
 *                        signature that holds to the frame (ExpandEmit with a position), which writes them into consecutive slots; slots >=
 *                        capacity are skipped
 *   pfac_host_done       the call's sequence number to mapped host memory (scan_passes.h: HostHandoff)
 * The walk along the chain (forEachChainMember), both passes, the capacity-checked store and the launches (expandPasses) are the expansion frame of
 * scan_passes.h, shared with scan_all.hip, scan_words.hip, scan_groups.hip and the other verify units; the class loop, the compare and the head
 * of PFACX_sigRun are scan_verify.h's; this unit's own is the test of a member (walkPair).
 * THE COMPARE (scan_verify.h: maskedEqual) works on dwords: the blob is dword-aligned and holds, per signature, its value dwords and behind them
 * its mask dwords (values ANDed with their masks, the bytes behind len with mask 0); the masked differences are ORed up and tested every 16 bytes.
 * Every index into the input is checked against [0, n) before the load; an id outside [1, F] is a pair that counts nothing, a walk ends after
 * chainLen steps whatever the table says, a class's range is clamped to the table and an entry whose dwords do not lie inside the blob is skipped:
 * a caller's list cannot make a pass read or write outside the buffers.  A thread per pair: a long signature, or a class of many, keeps its lane
 * busy while the others of its wave wait (DESIGN.md 5v says what that costs).
 * SCRATCH: 8 (blocks + 1) bytes rounded up to 256 (DeviceScratch::sigSet), blocks = one per 256 pairs, eight per compute unit at most.
 * Plain C++ and vector stores only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_sig.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"
#include "scan_verify.h"

namespace {

constexpr unsigned int kSigBlock = 256;

struct SigArgs {
    ExpandFrame f;                      /* the pairs, the chain table, the block cut, the caller's arrays (scan_passes.h); f.all is not read */
    InputView v;                        /* the caller's bytes (scan_verify.h) */
    const unsigned int *sigOff;         /* [numIds + 2] by anchor id: the first signature of its class */
    const pfac::SigEntry *sigs;         /* {signature id, anchorOff, len, blobOff} */
    unsigned int numSigs;
    const uint32_t *blob;               /* per signature: (len + 3) / 4 value dwords, then as many mask dwords */
    unsigned int blobWords;
};

/* The signatures that hold along pair k's chain, longest anchor first, table order (signature id descending) within an anchor
 * (scan_passes.h: forEachChainMember): emit(signature id, start) for each of them; returns their number */
template <class Emit>
__device__ __forceinline__ unsigned int walkPair(const SigArgs &a, size_t k, Emit emit)
{
    const int id = a.f.pairIds[k], p = a.f.pairPos[k];
    if (p < 0 || (unsigned int)p >= a.v.n) return 0u;
    unsigned int found = 0;
    forEachChainMember(a.f.table, a.f.numIds, id, [&](int q) {
        forEachClassEntry(a.sigOff, a.numSigs, q, [&](unsigned int v) {
            const pfac::SigEntry e = a.sigs[v];
            if (e.anchorOff < 0 || e.anchorOff > p || e.len <= 0) return;                            /* s < 0: before any load */
            const unsigned int s = (unsigned int)(p - e.anchorOff), len = (unsigned int)e.len;
            if (len > a.v.n - s) return;                                                             /* s + len > n */
            const unsigned int off = (unsigned int)e.blobOff;
            if (e.blobOff < 0 || !inBlob(a.blobWords, off, 2u * ((len + 3u) >> 2))) return;          /* (a table of the library's own: never) */
            if (!maskedEqual(a.v, a.blob + off, s, len)) return;
            emit(e.id, (int)s);
            found++;
        });
        return true;
    });
    return found;
}

__global__ __launch_bounds__(kSigBlock) void pfac_sig_count(SigArgs a)
{
    expandCount<kSigBlock>(a.f, [&](size_t k) -> unsigned long long { return walkPair(a, k, [](int, int) {}); });
}

__global__ __launch_bounds__(kSigBlock) void pfac_sig_write(SigArgs a)
{
    expandWrite<kSigBlock>(
        a.f, [&](size_t k) -> unsigned long long { return walkPair(a, k, [](int, int) {}); },
        [&](size_t k, auto emit) { (void)walkPair(a, k, emit); });
}

} // namespace

extern "C" {

PFAC_status_t PFACX_sigRun(PFAC_handle_t handle, const PFACX_sigRun_t *run, size_t *h_total)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!run || !verifyRunOk(run->v, h_total) || !run->v.d_blob || !run->d_sigOff || !run->d_sigs || run->numSigs > (size_t)0x7fffffff)
        return PFAC_STATUS_INVALID_PARAMETER;
    *h_total = 0;
    if (run->v.count == 0) return PFAC_STATUS_SUCCESS;
    PFAC_context *c = handle;
    SigArgs a{};
    a.v = verifyInput(run->v);
    a.sigOff = run->d_sigOff;
    a.sigs = static_cast<const pfac::SigEntry *>(run->d_sigs);
    a.numSigs = (unsigned int)run->numSigs;
    a.blob = run->v.d_blob;
    a.blobWords = (unsigned int)run->v.blobWords;
    a.f = verifyFrame(run->v);
    return expandPasses(c, c->scratch.sigSet, pfac::kHostSig, a, pfac_sig_count, pfac_sig_write, kSigBlock, a.f.capacity != 0, h_total);
}

} /* extern "C" */
