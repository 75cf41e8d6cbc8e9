/*
 * scan_batch.hip -- segmented (batch) matching: the fix-ups that turn the result of ONE scan over the concatenation of many
 * independent segments (packets, records) into the concatenation of the per-segment results (include/pfac_ext.h:
 * PFACX_matchBatchFromDevice / ...Reduce; DESIGN.md "batch").
 *
 * The scan itself is the unchanged match path (scan_filter / scan_tiled).  Let U(p) be its result at p and e the end of p's
 * segment.  U(p) == 0: no pattern starts at p, so the segment's result is 0 too.  p + len(U(p)) <= e: the longest pattern at p
 * lies inside the segment, so it is the segment's answer.  Otherwise the answer is the longest pattern at p that ends by e:
 * one bounded walk (boundedWalk, scan_common.h -- what the ends of an input get).  Only p in [max(s, e - maxPatternLen + 1), e)
 * can have the last case: the ZONE of the segment.
 *
 *   pfac_batch_fixup          full result: G lanes per segment (G a power of two <= 64, picked by the host from the
 *                             zone length and the mean segment length), coalesced reads of the zone, a walk only where
 *                             the id found does not fit the segment
 *   pfac_batch_pair_fixup     compacted result: one lane per pair, its segment by binary search in the offsets; a pair
 *                             that crosses its segment's end is walked again (new id 0: the pair drops out); kept pairs per block
 *   pfac_array_scan           exclusive scan of the kept counts (one block; scan_passes.h) ...
 *   pfac_batch_compact        ... stable scatter of the kept pairs to scratch (only when some pair dropped)
 *   pfac_batch_seg_first      one lane per segment boundary: lower bound of offsets[k] among the pair positions
 *
 * Offsets on the device are the caller's contract (checking them would cost a sync): every offset is clamped to [0, size]
 * before it is used, a decreasing pair of offsets is an empty segment, so no offset can make a kernel read or write outside
 * the input, the result or the pair arrays.  Plain C++ stores only; no kernel of the other units is touched.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_batch.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"

namespace {

constexpr int kBatchBlock = 256;                       /* pfac_amd/api.py: PFACX_BATCH_BLOCK (tests/batch_edges.py builds its cases on it) */

struct BatchArgs {
    const unsigned char *in;
    size_t size;
    const size_t *offsets;                             /* numSegments + 1 entries, clamped to [0, size] where read */
    size_t numSegments;
    const int *patternLen;                             /* [numFinal + 1] by pattern id */
    int numFinal;
    uint32_t maxWalk;                                  /* maxPatternLen - 1: the zone length */
};

__device__ __forceinline__ size_t offsetAt(const BatchArgs &b, size_t k)
{
    const size_t o = b.offsets[k];
    return o < b.size ? o : b.size;
}

/* does id (found over the concatenation at p) run past e?  An id outside [1, numFinal] cannot come from the scan: walked again */
__device__ __forceinline__ bool crossesEnd(const BatchArgs &b, int id, size_t p, size_t e)
{
    if (id == 0) return false;
    if (id < 0 || id > b.numFinal) return true;
    return p + (size_t)b.patternLen[id] > e;
}

/* A group takes kSegsPerTrip consecutive segments per trip: their offsets, then the first zone position of each, are loaded as
 * independent loads -- one memory round trip per kSegsPerTrip segments instead of two per segment (a batch of 64-byte segments is
 * millions of them; DESIGN.md "batch" has what that bought: less than hoped) */
constexpr int kSegsPerTrip = 8;                        /* pfac_amd/api.py: PFACX_BATCH_SEGS_PER_TRIP */

template <bool TEX>
__global__ __launch_bounds__(kBatchBlock) void pfac_batch_fixup(BatchArgs b, ScanArgs a, int *out, uint32_t groupLog2)
{
    const ChainCtx<TEX> ctx(a);
    const size_t tid = (size_t)blockIdx.x * kBatchBlock + threadIdx.x;
    const uint32_t g = 1u << groupLog2, j = (uint32_t)tid & (g - 1u);
    const size_t groups = ((size_t)gridDim.x * kBatchBlock) >> groupLog2;
    for (size_t k0 = (tid >> groupLog2) * kSegsPerTrip; k0 < b.numSegments; k0 += groups * kSegsPerTrip) {
        size_t o[kSegsPerTrip + 1];
#pragma unroll
        for (int u = 0; u <= kSegsPerTrip; u++) o[u] = k0 + u <= b.numSegments ? offsetAt(b, k0 + u) : 0;
        size_t p[kSegsPerTrip];
        int id[kSegsPerTrip];
#pragma unroll
        for (int u = 0; u < kSegsPerTrip; u++) {
            const size_t s = o[u], e = k0 + u < b.numSegments ? o[u + 1] : 0;
            const size_t z = e > s && e - s > b.maxWalk ? e - b.maxWalk : s;
            p[u] = z + j;
            id[u] = e > s && p[u] < e ? out[p[u]] : 0;
        }
#pragma unroll
        for (int u = 0; u < kSegsPerTrip; u++) {
            const size_t s = o[u], e = k0 + u < b.numSegments ? o[u + 1] : 0;
            if (e <= s || p[u] >= e) continue;
            if (crossesEnd(b, id[u], p[u], e)) out[p[u]] = boundedWalk(ctx, b.in, p[u], e);
            for (size_t q = p[u] + g; q < e; q += g) {                 /* zones longer than the group */
                const int v = out[q];
                if (crossesEnd(b, v, q, e)) out[q] = boundedWalk(ctx, b.in, q, e);
            }
        }
    }
}

/* one lane per pair; blockKept[blockIdx.x] = pairs of this block that stay, *drops += those that go */
template <bool TEX>
__global__ __launch_bounds__(kBatchBlock) void pfac_batch_pair_fixup(BatchArgs b, ScanArgs a, int *ids, const int *pos, unsigned int count,
                                                                    unsigned int *blockKept, unsigned int *drops)
{
    __shared__ unsigned int kept[kBatchBlock / 64];
    const ChainCtx<TEX> ctx(a);
    const size_t i = (size_t)blockIdx.x * kBatchBlock + threadIdx.x;
    bool keep = false;
    if (i < count) {
        int id = ids[i];
        const size_t p = (size_t)(uint32_t)pos[i];
        if (p < b.size) {
            /* the segment of p: the last k < numSegments with offsets[k] <= p */
            size_t lo = 0, hi = b.numSegments - 1;
            while (lo < hi) {
                const size_t mid = lo + (hi - lo + 1) / 2;
                if (offsetAt(b, mid) <= p) lo = mid; else hi = mid - 1;
            }
            const size_t e = offsetAt(b, lo + 1);
            if (crossesEnd(b, id, p, e)) {
                id = boundedWalk(ctx, b.in, p, e);
                ids[i] = id;
            }
        } else {
            id = 0;                                    /* cannot come from the scan */
            ids[i] = 0;
        }
        keep = id != 0;
    }
    const uint64_t m = __ballot(keep);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) kept[wave] = (unsigned int)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int t = 0;
        for (int w = 0; w < kBatchBlock / 64; w++) t += kept[w];
        blockKept[blockIdx.x] = t;
        const unsigned int inBlock = count - (unsigned int)blockIdx.x * kBatchBlock;
        const unsigned int here = inBlock < (unsigned int)kBatchBlock ? inBlock : (unsigned int)kBatchBlock;
        if (here > t) atomicAdd(drops, here - t);
    }
}

/* kept pair i goes to slot blockBase[block] + (kept pairs in front of it inside the block): the order stays */
__global__ __launch_bounds__(kBatchBlock) void pfac_batch_compact(const int *ids, const int *pos, unsigned int count, const unsigned int *blockBase,
                                                                  int *idsOut, int *posOut)
{
    __shared__ unsigned int kept[kBatchBlock / 64];
    const size_t i = (size_t)blockIdx.x * kBatchBlock + threadIdx.x;
    const int id = i < count ? ids[i] : 0;
    const bool keep = id != 0;
    const uint64_t m = __ballot(keep);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) kept[wave] = (unsigned int)__popcll(m);
    __syncthreads();
    unsigned int at = blockBase[blockIdx.x] + laneRankIn(m);
    for (uint32_t w = 0; w < wave; w++) at += kept[w];
    if (keep) {
        idsOut[at] = id;
        posOut[at] = pos[i];
    }
}

/* segFirst[k] = first pair whose position is >= offsets[k], k in [0, numSegments]: pairs of segment k are [segFirst[k], segFirst[k + 1]) */
__global__ __launch_bounds__(kBatchBlock) void pfac_batch_seg_first(BatchArgs b, const int *pos, unsigned int count, int *segFirst)
{
    const size_t stride = (size_t)gridDim.x * kBatchBlock;
    for (size_t k = (size_t)blockIdx.x * kBatchBlock + threadIdx.x; k <= b.numSegments; k += stride) {
        const size_t o = offsetAt(b, k);
        unsigned int lo = 0, hi = count;
        while (lo < hi) {
            const unsigned int mid = lo + (hi - lo) / 2;
            if ((size_t)(uint32_t)pos[mid] < o) lo = mid + 1; else hi = mid;
        }
        segFirst[k] = (int)lo;
    }
}

uint32_t clampExtent32(size_t bytes) { return bytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)bytes; }

/* what ChainCtx reads of the kernel arguments: the WIDE chained table as scan_module.hip (fillArgs) describes it to the other kernels */
PFAC_status_t chainArgs(const PFAC_context *c, const char *d_input, ScanArgs &a)
{
    if (!c->tables.chainSlots || c->chainJumpLog2 <= 0) return PFAC_STATUS_INTERNAL_ERROR;
    const size_t chained = c->tables.chainSlots.bytes(), slots = c->tables.chainSlots.count();
    if (c->textureMode == PFAC_TEXTURE_ON && chained > 0xFFFFFFFFull) return PFAC_STATUS_CUDA_ALLOC_FAILED;   /* 32-bit buffer offsets */
    a = ScanArgs{};
    a.in = reinterpret_cast<const unsigned char *>(d_input);
    a.chainSlots = reinterpret_cast<const u32x4 *>(c->tables.chainSlots.get());
    a.jumpShift = 32u - (uint32_t)c->chainJumpLog2;
    a.extDelta = (uint32_t)(slots / 2);
    a.jumpBase = (uint32_t)(slots / 2 - (size_t(2) << c->chainJumpLog2));
    a.jumpLongBase = a.jumpBase + (uint32_t)(size_t(1) << c->chainJumpLog2);
    a.rootRow = a.jumpBase - (uint32_t)pfac::kCharSet;
    a.chainBytes = clampExtent32(chained);
    return PFAC_STATUS_SUCCESS;
}

BatchArgs batchArgs(const PFAC_context *c, const char *d_input, size_t size, const size_t *d_offsets, size_t numSegments, const int *d_patternLen)
{
    BatchArgs b;
    b.in = reinterpret_cast<const unsigned char *>(d_input);
    b.size = size;
    b.offsets = d_offsets;
    b.numSegments = numSegments;
    b.patternLen = d_patternLen;
    b.numFinal = c->fa.numPatterns;
    b.maxWalk = c->fa.maxPatternLen > 0 ? (uint32_t)c->fa.maxPatternLen - 1u : 0u;
    return b;
}

} // namespace

extern "C" {

PFAC_status_t PFACX_batchFixup(PFAC_handle_t handle, const char *d_input, size_t size, const size_t *d_offsets, size_t numSegments,
                               int *d_matched_result, const int *d_patternLen)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!d_input || !d_offsets || !d_matched_result || !d_patternLen || numSegments == 0) return PFAC_STATUS_INVALID_PARAMETER;
    const PFAC_context *c = handle;
    ScanArgs a;
    const PFAC_status_t st = chainArgs(c, d_input, a);
    if (st != PFAC_STATUS_SUCCESS) return st;
    const BatchArgs b = batchArgs(c, d_input, size, d_offsets, numSegments, d_patternLen);
    if (size == 0 || b.maxWalk == 0) return PFAC_STATUS_SUCCESS;      /* patterns of one byte never cross an end */
    /* lanes per segment: the zone, or the mean segment if that is shorter, rounded up to a power of two */
    const size_t mean = size / numSegments, want = mean < b.maxWalk ? (mean ? mean : 1) : b.maxWalk;
    uint32_t groupLog2 = 0;                            /* (the 6: pfac_amd/api.py: PFACX_BATCH_MAX_GROUP_LOG2; tests/batch_edges.py: group_log2 repeats this choice) */
    while (groupLog2 < 6 && (size_t(1) << groupLog2) < want) groupLog2++;
    const size_t perBlock = ((size_t)kBatchBlock >> groupLog2) * kSegsPerTrip;      /* segments a block takes per trip */
    const size_t blocks = numSegments / perBlock + 1;
    const unsigned int grid = blocks < gridCap(c, 16) ? (unsigned int)blocks : gridCap(c, 16);
    if (c->textureMode == PFAC_TEXTURE_ON)
        hipLaunchKernelGGL(pfac_batch_fixup<true>, dim3(grid), dim3(kBatchBlock), 0, 0, b, a, d_matched_result, groupLog2);
    else
        hipLaunchKernelGGL(pfac_batch_fixup<false>, dim3(grid), dim3(kBatchBlock), 0, 0, b, a, d_matched_result, groupLog2);
    return hipGetLastError() == hipSuccess ? PFAC_STATUS_SUCCESS : PFAC_STATUS_INTERNAL_ERROR;
}

PFAC_status_t PFACX_batchReduceFixup(PFAC_handle_t handle, const char *d_input, size_t size, const size_t *d_offsets, size_t numSegments,
                                     int *d_ids, int *d_pos, int *count, int *d_segFirst, const int *d_patternLen)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!d_input || !d_offsets || !d_ids || !d_pos || !count || !d_segFirst || !d_patternLen || numSegments == 0 || *count < 0)
        return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = handle;
    ScanArgs a;
    const PFAC_status_t st = chainArgs(c, d_input, a);
    if (st != PFAC_STATUS_SUCCESS) return st;
    const BatchArgs b = batchArgs(c, d_input, size, d_offsets, numSegments, d_patternLen);
    const bool tex = c->textureMode == PFAC_TEXTURE_ON;
    const unsigned int n = (unsigned int)*count;
    if (n > 0 && b.maxWalk > 0) {
        const size_t blocks = ((size_t)n + kBatchBlock - 1) / kBatchBlock;
        /* grow-only scratch of the compacted form: [0, 256) drop counter, then kept counts per block, then the compacted ids and positions */
        unsigned int *drops = nullptr, *blockKept = nullptr;
        int *idsOut = nullptr;
        const PFAC_status_t carved = carveScratch(c->scratch.batch, [&](ScratchCarver &k) {
            drops = k.take<unsigned int>(1);
            blockKept = k.take<unsigned int>(blocks);
            idsOut = k.take<int>(2 * (size_t)n);
        });
        if (carved != PFAC_STATUS_SUCCESS) return carved;
        int *posOut = idsOut + n;
        if (hipMemsetAsync(drops, 0, sizeof(unsigned int), 0) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
        if (tex)
            hipLaunchKernelGGL(pfac_batch_pair_fixup<true>, dim3((unsigned int)blocks), dim3(kBatchBlock), 0, 0, b, a, d_ids, d_pos, n, blockKept, drops);
        else
            hipLaunchKernelGGL(pfac_batch_pair_fixup<false>, dim3((unsigned int)blocks), dim3(kBatchBlock), 0, 0, b, a, d_ids, d_pos, n, blockKept, drops);
        unsigned int dropped = 0;
        if (hipGetLastError() != hipSuccess || hipMemcpy(&dropped, drops, sizeof(dropped), hipMemcpyDeviceToHost) != hipSuccess)
            return PFAC_STATUS_INTERNAL_ERROR;
        if (dropped > n) return PFAC_STATUS_INTERNAL_ERROR;
        if (dropped) {                                 /* rare: a pattern that straddled a segment end and nothing shorter inside */
            const unsigned int left = n - dropped;
            hipLaunchKernelGGL(pfac_array_scan<unsigned int>, dim3(1), dim3(1024), 0, 0, blockKept, (unsigned int)blocks, (unsigned int *)nullptr, (unsigned int *)nullptr);
            hipLaunchKernelGGL(pfac_batch_compact, dim3((unsigned int)blocks), dim3(kBatchBlock), 0, 0, d_ids, d_pos, n, blockKept, idsOut, posOut);
            if (hipGetLastError() != hipSuccess ||
                (left && (hipMemcpyAsync(d_ids, idsOut, left * sizeof(int), hipMemcpyDeviceToDevice, 0) != hipSuccess ||
                          hipMemcpyAsync(d_pos, posOut, left * sizeof(int), hipMemcpyDeviceToDevice, 0) != hipSuccess)))
                return PFAC_STATUS_INTERNAL_ERROR;
            *count = (int)left;
        }
    }
    const size_t lanes = numSegments + 1, blocks = (lanes + kBatchBlock - 1) / kBatchBlock;
    const unsigned int grid = blocks < gridCap(c, 16) ? (unsigned int)blocks : gridCap(c, 16);
    hipLaunchKernelGGL(pfac_batch_seg_first, dim3(grid), dim3(kBatchBlock), 0, 0, b, d_pos, (unsigned int)*count, d_segFirst);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(0) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
