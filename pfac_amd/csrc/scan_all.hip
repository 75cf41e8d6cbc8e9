/*
 * scan_all.hip -- all matches (include/pfac_ext.h: PFACX_matchAll*): the expansion of the ordered list of longest matches into
 * the list of every (position, pattern) pair (DESIGN.md "all matches").
 *
 * Every pattern P that starts at p is a prefix of the longest one L that starts there (both match the bytes at p, P is not
 * longer), so P is a final state on the trie path to L.  The host derives per pattern id the longest proper prefix pattern
 * and the length of that chain (pattern_compiler.cpp: buildPrefixPatterns); the pairs at p are L, prefix(L), prefix(prefix(L)),
 * ... -- longest first.  The longest-match scan is the unchanged compacted-output path (scan_module.hip: PFACX_allReduce, whose
 * ordering writes the ordered pairs into the handle's scratch); behind it, on the default stream:
 *   pfac_all_count       blocks own consecutive ranges of the longest pairs; each lane reads chainLen[id] (a table of 8 bytes
 *                        per id: L2 resident for any real set), the block's total goes to blockBase[block]
 *   pfac_array_scan      exclusive scan of the block totals (one block; 64-bit; scan_passes.h), the grand total to mapped host memory
 *   pfac_all_scatter     the block's range again: lane prefix of the chain lengths, then each lane writes its pair and follows
 *                        prefixPattern into consecutive slots; slots >= capacity are skipped (the caller learns the full count)
 *   pfac_all_seg_first   batch form: one lane per segment boundary, the expanded offset of the first longest pair of the segment
 *   pfac_host_done       writes the call's sequence number to mapped host memory (the host polls it instead of a stream sync; scan_passes.h: HostHandoff)
 * Writes are plain vector stores; no kernel of the other units is touched.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_all.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"

namespace {

constexpr int kAllBlock = 256;

struct ExpandArgs {
    const int *pairIds;                 /* the ordered longest pairs */
    const int *pairPos;
    size_t count;
    const pfac::Int2 *table;            /* [numIds + 1] {prefixPattern, chainLen} by id */
    int numIds;
    size_t per;                         /* longest pairs per block: a multiple of kAllBlock */
    unsigned long long *blockBase;      /* [blocks + 1]: block totals -> their exclusive prefix; [blocks] = the grand total */
    unsigned int blocks;
    int *ids;                           /* the caller's arrays: capacity entries each */
    int *pos;
    size_t capacity;
    unsigned long long *pairOffset;     /* batch form: the expanded offset of every longest pair (else null) */
};

/* an id the scan cannot report (outside [1, numIds]) stands for itself alone */
__device__ __forceinline__ unsigned int chainOf(const ExpandArgs &x, int id)
{
    if (id < 1 || id > x.numIds) return 1u;
    const int c = x.table[id].y;
    return c > 0 ? (unsigned int)c : 1u;
}

__global__ __launch_bounds__(kAllBlock) void pfac_all_count(ExpandArgs x)
{
    __shared__ unsigned long long waveSum[kAllBlock / 64];
    const size_t first = (size_t)blockIdx.x * x.per;
    const size_t end = x.count - first < x.per ? x.count : first + x.per;
    unsigned long long own = 0;
    for (size_t i = first + threadIdx.x; i < end; i += kAllBlock) own += chainOf(x, x.pairIds[i]);
    unsigned long long total = 0;
    (void)blockExclusive<kAllBlock>(own, waveSum, total);
    if (threadIdx.x == 0) x.blockBase[blockIdx.x] = total;
}

__global__ __launch_bounds__(kAllBlock) void pfac_all_scatter(ExpandArgs x)
{
    __shared__ unsigned long long waveSum[kAllBlock / 64];
    const size_t first = (size_t)blockIdx.x * x.per;
    const size_t end = x.count - first < x.per ? x.count : first + x.per;
    unsigned long long base = x.blockBase[blockIdx.x];
    for (size_t i0 = first; i0 < end; i0 += kAllBlock) {        /* the same trip count for every thread of the block */
        const size_t i = i0 + threadIdx.x;
        const bool has = i < end;
        const int id = has ? x.pairIds[i] : 0;
        const int p = has ? x.pairPos[i] : 0;
        const unsigned int c = has ? chainOf(x, id) : 0u;
        unsigned long long stepTotal = 0;
        const unsigned long long o = base + blockExclusive<kAllBlock>((unsigned long long)c, waveSum, stepTotal);
        base += stepTotal;
        if (!has) continue;
        if (x.pairOffset != nullptr) x.pairOffset[i] = o;
        int q = id;
        for (unsigned int k = 0; k < c; k++) {
            if (o + k < x.capacity) {
                x.ids[o + k] = q;
                x.pos[o + k] = p;
            }
            q = q >= 1 && q <= x.numIds ? x.table[q].x : 0;
        }
    }
}

/* segFirst[k] for k in [0, numSegments]: first[k] (the first longest pair of segment k; clamped to count) through the expansion:
 * pairOffset[first[k]], or the total behind the last pair.  Without an expansion (no pairOffset: every chain has length 1) the
 * index is the same in both lists. */
__global__ __launch_bounds__(kAllBlock) void pfac_all_seg_first(const int *first, size_t numSegments, size_t count,
                                                               const unsigned long long *pairOffset, const unsigned long long *total,
                                                               size_t *segFirst)
{
    const size_t stride = (size_t)gridDim.x * kAllBlock;
    for (size_t k = (size_t)blockIdx.x * kAllBlock + threadIdx.x; k <= numSegments; k += stride) {
        const int f = first[k];
        const size_t j = f < 0 ? 0 : ((size_t)f < count ? (size_t)f : count);
        if (pairOffset == nullptr) segFirst[k] = j;
        else segFirst[k] = j < count ? (size_t)pairOffset[j] : (size_t)*total;
    }
}

} // namespace

extern "C" {

PFAC_status_t PFACX_allExpand(PFAC_handle_t handle, const int *d_pairIds, const int *d_pairPos, size_t count, const void *d_table,
                              int *d_ids, int *d_pos, size_t capacity, const int *d_segFirstPairs, size_t numSegments, size_t *d_segFirst,
                              size_t *h_total)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!h_total || (count && d_table && (!d_pairIds || !d_pairPos || !d_ids || !d_pos)) || (d_segFirst && !d_segFirstPairs))
        return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = handle;
    if (!d_table) {                                    /* chains of length 1: the list is the longest list, only segFirst changes type */
        if (d_segFirst) {
            const size_t lanes = numSegments + 1, b = (lanes + kAllBlock - 1) / kAllBlock;
            const unsigned int grid = b < gridCap(c, 8) ? (unsigned int)b : gridCap(c, 8);
            hipLaunchKernelGGL(pfac_all_seg_first, dim3(grid), dim3(kAllBlock), 0, 0, d_segFirstPairs, numSegments, count,
                               (const unsigned long long *)nullptr, (const unsigned long long *)nullptr, d_segFirst);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(0) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
        }
        *h_total = count;
        return PFAC_STATUS_SUCCESS;
    }
    ExpandArgs x{};
    x.pairIds = d_pairIds;
    x.pairPos = d_pairPos;
    x.count = count;
    x.table = static_cast<const pfac::Int2 *>(d_table);
    x.numIds = c->fa.numPatterns;
    x.ids = d_ids;
    x.pos = d_pos;
    x.capacity = capacity;
    x.blocks = offsetBlocks(c, count, kAllBlock, x.per);
    const size_t blocks = x.blocks;
    /* grow-only, half as much again where it grows: the block totals, then (batch form) the expanded offset of every longest pair */
    const PFAC_status_t carved = carveScratch(c->scratch.all, [&](ScratchCarver &k) {
        x.blockBase = k.take<unsigned long long>(blocks + 1);
        x.pairOffset = d_segFirst ? k.take<unsigned long long>(count) : nullptr;
    }, nullptr, true);
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    const HostHandoff list(c, pfac::kHostAll);
    if (blocks) hipLaunchKernelGGL(pfac_all_count, dim3((unsigned int)blocks), dim3(kAllBlock), 0, 0, x);
    hipLaunchKernelGGL(pfac_array_scan<unsigned long long>, dim3(1), dim3(1024), 0, 0, x.blockBase, (unsigned int)blocks, x.blockBase + blocks,
                       reinterpret_cast<unsigned long long *>(list.d_value));
    if (blocks) hipLaunchKernelGGL(pfac_all_scatter, dim3((unsigned int)blocks), dim3(kAllBlock), 0, 0, x);
    if (d_segFirst) {
        const size_t lanes = numSegments + 1, b = (lanes + kAllBlock - 1) / kAllBlock;
        const unsigned int grid = b < gridCap(c, 8) ? (unsigned int)b : gridCap(c, 8);
        hipLaunchKernelGGL(pfac_all_seg_first, dim3(grid), dim3(kAllBlock), 0, 0, d_segFirstPairs, numSegments, count, x.pairOffset,
                           x.blockBase + blocks, d_segFirst);
    }
    unsigned long long total = 0;
    if (!list.finish(&total, x.blockBase + blocks)) return PFAC_STATUS_INTERNAL_ERROR;
    *h_total = (size_t)total;
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
