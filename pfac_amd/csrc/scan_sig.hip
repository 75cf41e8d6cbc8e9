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
 * scan_passes.h, shared with scan_all.hip, scan_words.hip, scan_groups.hip and scan_case.hip; this unit's own is the test of a member (walkPair)
 * and the compare.
 * THE COMPARE works on dwords: the blob is dword-aligned and holds, per signature, its value dwords and behind them its mask dwords (values
 * ANDed with their masks, the bytes behind len with mask 0); the input side of dword k is composed from the two aligned dwords around in[s + 4 k]
 * with v_alignbyte, as in scan_case.hip; the masked differences are ORed up and tested every 16 bytes.  An aligned dword that would reach outside
 * [0, n) -- in front of in[0] where the caller's pointer is misaligned and s < 3, behind in[n - 1] at the end -- is put together from its bytes
 * inside the buffer (three at most), and the len & 3 bytes behind the signature's last whole dword are compared byte by byte.
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

namespace {

constexpr unsigned int kSigBlock = 256;

struct SigArgs {
    ExpandFrame f;                      /* the pairs, the chain table, the block cut, the caller's arrays (scan_passes.h); f.all is not read */
    const unsigned char *in;            /* the caller's bytes */
    unsigned int n;
    const unsigned int *sigOff;         /* [numIds + 2] by anchor id: the first signature of its class */
    const pfac::SigEntry *sigs;         /* {signature id, anchorOff, len, blobOff} */
    unsigned int numSigs;
    const uint32_t *blob;               /* per signature: (len + 3) / 4 value dwords, then as many mask dwords */
    unsigned int blobWords;
};

/* the aligned dword of the input whose first byte is in[o] (o: any sign; in + o is dword-aligned): one load where it lies inside [0, n), else its
 * bytes inside the buffer, zero for the others */
__device__ __forceinline__ uint32_t alignedDword(const SigArgs &a, long long o)
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

/* ((in[s + k] ^ value[k]) & mask[k]) == 0 for every k < len?  s + len <= n and the signature's 2 ((len + 3) / 4) dwords at blob[off ...] lie
 * inside the blob (the caller has checked both) */
__device__ __forceinline__ bool maskedEqual(const SigArgs &a, unsigned int s, unsigned int len, unsigned int off)
{
    const unsigned int words = len >> 2, r = (unsigned int)(reinterpret_cast<uintptr_t>(a.in + s) & 3u);
    const uint32_t *val = a.blob + off, *mask = val + ((len + 3u) >> 2);
    uint32_t diff = 0;
    if (r == 0) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(a.in + s);       /* whole dwords inside [s, s + len) */
        for (unsigned int k = 0; k < words; k++) {
            diff |= (src[k] ^ val[k]) & mask[k];
            if ((k & 3u) == 3u && diff != 0) return false;
        }
    } else {
        const long long base = (long long)s - (long long)r;                     /* the aligned dword that holds in[s] */
        uint32_t lo = words ? alignedDword(a, base) : 0u;
        for (unsigned int k = 0; k < words; k++) {
            const uint32_t hi = alignedDword(a, base + 4ll * (k + 1u));
            diff |= (__builtin_amdgcn_alignbyte(hi, lo, r) ^ val[k]) & mask[k];
            if ((k & 3u) == 3u && diff != 0) return false;
            lo = hi;
        }
    }
    if (diff != 0) return false;
    const unsigned int tail = len & 3u;
    if (tail) {
        const uint32_t v = val[words], m = mask[words];
        for (unsigned int b = 0; b < tail; b++)
            if ((((uint32_t)a.in[s + 4u * words + b] ^ (v >> (8u * b))) & (m >> (8u * b)) & 0xFFu) != 0u) return false;
    }
    return true;
}

/* The signatures that hold along pair k's chain, longest anchor first, table order (signature id descending) within an anchor
 * (scan_passes.h: forEachChainMember): emit(signature id, start) for each of them; returns their number */
template <class Emit>
__device__ __forceinline__ unsigned int walkPair(const SigArgs &a, size_t k, Emit emit)
{
    const int id = a.f.pairIds[k], p = a.f.pairPos[k];
    if (p < 0 || (unsigned int)p >= a.n) return 0u;
    unsigned int found = 0;
    forEachChainMember(a.f.table, a.f.numIds, id, [&](int q) {
        const unsigned int first = a.sigOff[q];
        unsigned int end = a.sigOff[q + 1];
        if (end > a.numSigs) end = a.numSigs;
        for (unsigned int v = first; v < end; v++) {
            const pfac::SigEntry e = a.sigs[v];
            if (e.anchorOff < 0 || e.anchorOff > p || e.len <= 0) continue;                          /* s < 0: before any load */
            const unsigned int s = (unsigned int)(p - e.anchorOff), len = (unsigned int)e.len;
            if (len > a.n - s) continue;                                                             /* s + len > n */
            const unsigned int off = (unsigned int)e.blobOff, need = 2u * ((len + 3u) >> 2);
            if (e.blobOff < 0 || off >= a.blobWords || a.blobWords - off < need) continue;           /* (a table of the library's own: never) */
            if (!maskedEqual(a, s, len, off)) continue;
            emit(e.id, (int)s);
            found++;
        }
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
    if (!run || !h_total || !run->d_input || run->size == 0 || run->size > (size_t)0x7fffffff || run->numIds > (size_t)0x7ffffffe || !run->d_sigOff ||
        !run->d_sigs || run->numSigs > (size_t)0x7fffffff || run->blobWords > (size_t)0x7fffffff || !run->d_blob || run->count > (size_t)0x7fffffff ||
        (run->count && (!run->d_pairIds || !run->d_pairPos)) || (run->capacity && (!run->d_ids || !run->d_pos)))
        return PFAC_STATUS_INVALID_PARAMETER;
    *h_total = 0;
    if (run->count == 0) return PFAC_STATUS_SUCCESS;
    PFAC_context *c = handle;
    SigArgs a{};
    a.in = reinterpret_cast<const unsigned char *>(run->d_input);
    a.n = (unsigned int)run->size;
    a.sigOff = run->d_sigOff;
    a.sigs = static_cast<const pfac::SigEntry *>(run->d_sigs);
    a.numSigs = (unsigned int)run->numSigs;
    a.blob = run->d_blob;
    a.blobWords = (unsigned int)run->blobWords;
    a.f = ExpandFrame{run->d_pairIds, run->d_pairPos, run->count, static_cast<const pfac::Int2 *>(run->d_table), (unsigned int)run->numIds,
                      1u, 0, nullptr, run->d_ids, run->d_pos, run->capacity};
    return expandPasses(c, c->scratch.sigSet, pfac::kHostSig, a, pfac_sig_count, pfac_sig_write, kSigBlock, a.f.capacity != 0, h_total);
}

} /* extern "C" */
