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
 *                        per id: L2 resident for any real set), the block's total goes to blockBase[block] (scan_passes.h: expandCount)
 *   pfac_array_scan      exclusive scan of the block totals (one block; 64-bit; scan_passes.h), the grand total to mapped host memory
 *   pfac_all_scatter     the block's range again (expandWrite): lane prefix of the chain lengths, then each lane hands its pair and what
 *                        follows along prefixPattern to the frame, which writes consecutive slots; slots >= capacity are skipped (the
 *                        caller learns the full count); the batch form's pairOffset is the hook of the write pass
 *   pfac_all_seg_first   batch form: one lane per segment boundary, the expanded offset of the first longest pair of the segment
 *   pfac_host_done       writes the call's sequence number to mapped host memory (the host polls it instead of a stream sync; scan_passes.h: HostHandoff)
 * Both passes, the capacity-checked store and the launches (expandPasses) are the expansion frame of scan_passes.h, shared with scan_words.hip
 * and scan_groups.hip; the walk of a chain under a test of its members is forEachChainMember there (this unit keeps every member and writes a
 * fixed number of slots per pair: pfac_all_scatter says why).
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
    ExpandFrame f;                      /* the pairs, the chain table, the block cut, the caller's arrays (scan_passes.h); `all` is not read */
    unsigned long long *pairOffset;     /* batch form: the expanded offset of every longest pair (else null) */
};

/* an id the scan cannot report (outside [1, numIds]) stands for itself alone */
__device__ __forceinline__ unsigned int chainOf(const ExpandFrame &f, int id)
{
    if ((unsigned int)id - 1u >= f.numIds) return 1u;
    const int c = f.table[id].y;
    return c > 0 ? (unsigned int)c : 1u;
}

__global__ __launch_bounds__(kAllBlock) void pfac_all_count(ExpandArgs x)
{
    expandCount<kAllBlock>(x.f, [&](size_t k) -> unsigned long long { return chainOf(x.f, x.f.pairIds[k]); });
}

/* Every pair fills exactly the chainOf(id) slots that the count pass -- a lookup, not a walk -- gave it, an id outside the set its one: a
 * fixed-count loop, not forEachChainMember, which visits nothing for such an id and may end in front of chainLen */
__global__ __launch_bounds__(kAllBlock) void pfac_all_scatter(ExpandArgs x)
{
    const ExpandFrame &f = x.f;
    int id = 0;                                                 /* of the pair a thread has just valued: left to its store */
    unsigned int c = 0;
    expandWrite<kAllBlock>(
        f,
        [&](size_t k) -> unsigned long long {
            id = f.pairIds[k];
            c = chainOf(f, id);
            return c;
        },
        [&](size_t, auto emit) {
            int q = id;
            for (unsigned int j = 0; j < c; j++) {
                emit(q);
                q = (unsigned int)q - 1u < f.numIds ? f.table[q].x : 0;
            }
        },
        [&](size_t k, unsigned long long before) {
            if (x.pairOffset != nullptr) x.pairOffset[k] = before;
        });
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

inline void launchSegFirst(const PFAC_context *c, const int *first, size_t numSegments, size_t count, const unsigned long long *pairOffset,
                           const unsigned long long *total, size_t *segFirst)
{
    const size_t lanes = numSegments + 1, b = (lanes + kAllBlock - 1) / kAllBlock;
    const unsigned int grid = b < gridCap(c, 8) ? (unsigned int)b : gridCap(c, 8);
    hipLaunchKernelGGL(pfac_all_seg_first, dim3(grid), dim3(kAllBlock), 0, 0, first, numSegments, count, pairOffset, total, segFirst);
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
            launchSegFirst(c, d_segFirstPairs, numSegments, count, nullptr, nullptr, d_segFirst);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(0) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
        }
        *h_total = count;
        return PFAC_STATUS_SUCCESS;
    }
    ExpandArgs x{};
    x.f = ExpandFrame{d_pairIds, d_pairPos, count, static_cast<const pfac::Int2 *>(d_table), (unsigned int)c->fa.numPatterns, 1u, 0, nullptr,
                      d_ids, d_pos, capacity};
    /* grow-only, half as much again where it grows: the block totals, then (batch form) the expanded offset of every longest pair */
    return expandPasses(
        c, c->scratch.all, pfac::kHostAll, x, pfac_all_count, pfac_all_scatter, kAllBlock, true, h_total,
        [&](ScratchCarver &k) { x.pairOffset = d_segFirst ? k.take<unsigned long long>(count) : nullptr; }, true, ExpandNothing(),
        [&](const unsigned long long *d_total) {                /* behind the passes: the segments' first entries */
            if (d_segFirst) launchSegFirst(c, d_segFirstPairs, numSegments, count, x.pairOffset, d_total, d_segFirst);
        });
}

} /* extern "C" */
