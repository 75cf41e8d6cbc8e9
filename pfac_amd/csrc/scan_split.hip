/*
 * scan_split.hip -- split (include/pfac_ext.h: PFACX_split*): the offsets that cut a buffer into records at the bytes of a class D.
 *
 * The cut rule, the tiles of 16 KiB with their four regions, the class test, the walk of a region, the count pass and the start of a ...Run entry
 * (fillCutArgs, tileGrid, dispatchSingle) are scan_cuts.h, shared with scan_locate.hip and scan_capture.hip.
 * The offsets are 0, the cuts ascending, n.
 *
 *   pfac_split_count       (scan_cuts.h, with PARTS) grid-stride over the tiles: the tile's cuts (64-bit), the cuts of each region, the tile's
 *                          first and last cut (position in the tile + 1; 0: none) and its longest inner distance
 *   pfac_array_scan        (scan_passes.h) the exclusive prefix of the tiles' cuts in place, 64-bit; the total to the host
 *   pfac_split_longest     one block over the per-tile values, four tiles a thread: the last cut in front of each thread's tiles by a block prefix
 *                          under the maximum (blockExclusive), the distance from there to the tile's first cut, the tiles' inner distances, the
 *                          last segment: the longest segment, whatever the capacity, to the host
 *   pfac_split_write       the tiles again, where the caller has room for an entry: a cut's rank = the tile's prefix + the regions in front + the
 *                          lanes in front (a wave prefix of popcounts) + the set bits below it; offsets[1 + rank] = cut, 8-byte stores, dense and
 *                          ascending; every index is checked against the capacity, a region whose first entry lies behind it is left at once.
 *                          Thread 0 of block 0 writes entry 0 and the closing entry n
 *   pfac_host_done         the call's sequence number to mapped host memory (scan_passes.h: HostHandoff)
 * Two streaming reads of the input, 8 bytes written per segment.
 * SCRATCH, T = ceil(n / 16384) tiles: 8 (T + 1) + 16 T + 4 T + 4 T + 4 T + 8 bytes (the tiles' cuts and their prefix, the regions' cuts, first, last,
 * inner distance, the longest segment), each part rounded up to 256 bytes: 0.0022 bytes per input byte, whatever the data.
 * Plain C++ and vector stores only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_split.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_cuts.h"

namespace {

constexpr unsigned int kSplitPerThread = 4;                              /* tiles a thread of pfac_split_longest takes per trip */

struct SplitArgs : CutArgs {            /* scan_cuts.h: the input, the class, the flags, the per-tile values of the count pass */
    unsigned long long *longest;        /* one word */
    size_t *offsets;
    size_t capacity;
};

/* the longest segment from the per-tile values: one block, kSplitPerThread consecutive tiles a thread and trip */
__global__ __launch_bounds__(1024) void pfac_split_longest(SplitArgs a, unsigned long long *hostLongest)
{
    __shared__ unsigned long long waveMax[16];
    unsigned long long carry = 0, longest = 0;                          /* carry: the last cut so far (0: none yet -- the segment starts at 0) */
    for (size_t base = 0; base < a.tiles; base += (size_t)1024 * kSplitPerThread) {      /* the same trip count for every thread */
        const size_t i0 = base + (size_t)threadIdx.x * kSplitPerThread;
        unsigned long long own = 0;                                     /* the last cut of this thread's tiles: a cut is never 0 */
        for (unsigned int k = 0; k < kSplitPerThread; k++)
            if (i0 + k < a.tiles && a.tileLast[i0 + k] != 0) own = (unsigned long long)(i0 + k) * kSplitTile + a.tileLast[i0 + k] - 1u;
        unsigned long long total = 0;
        unsigned long long prev = OpMax()(carry, blockExclusive<1024>(own, waveMax, total, OpMax()));
        for (unsigned int k = 0; k < kSplitPerThread; k++) {
            const size_t i = i0 + k;
            if (i >= a.tiles || a.tileFirst[i] == 0) continue;
            const unsigned long long at = (unsigned long long)i * kSplitTile;
            longest = OpMax()(longest, OpMax()(at + a.tileFirst[i] - 1u - prev, (unsigned long long)a.tileGap[i]));
            prev = at + a.tileLast[i] - 1u;
        }
        carry = OpMax()(carry, total);
    }
    unsigned long long all = 0;
    (void)blockExclusive<1024>(longest, waveMax, all, OpMax());
    if (threadIdx.x == 0) {
        all = OpMax()(all, (unsigned long long)a.n - carry);            /* the last segment */
        *a.longest = all;
        storeToHost(hostLongest, all);
    }
}

template <bool SINGLE>
__global__ __launch_bounds__(kSplitThreads) void pfac_split_write(SplitArgs a)
{
    __shared__ uint32_t cls[8];
    stageClass<SINGLE>(a, cls);
    const unsigned int wave = threadIdx.x >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned long long closing = a.tileBase[a.tiles] + 1u;   /* the index of the entry n */
        a.offsets[0] = 0;                                               /* (capacity > 0: the launch's condition) */
        if (closing < a.capacity) a.offsets[closing] = a.n;
    }
    for (size_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const size_t r0 = tile * kSplitTile + (size_t)wave * kSplitRegion;
        if (r0 >= a.n) continue;
        unsigned long long at = 1u + a.tileBase[tile];                  /* the index of the region's first cut */
        for (unsigned int w = 0; w < wave; w++) at += a.regionCount[tile * kSplitWaves + w];
        if (at >= a.capacity) continue;                                 /* nothing of this region fits: the same in every lane */
        splitRegion<SINGLE>(a, cls, r0, [&](unsigned int o, uint32_t cut) {
            const uint32_t c = (uint32_t)__popc(cut);
            const uint32_t incl = waveInclusiveScan(c);
            unsigned long long i = at + (incl - c);
            for (uint32_t x = cut; x != 0 && i < a.capacity; x &= x - 1u, i++) a.offsets[i] = r0 + o + (uint32_t)__ffs((int)x) - 1u;
            at += (uint32_t)__shfl((int)incl, 63);
        });
    }
}

template <bool SINGLE>
void splitLaunches(const PFAC_context *c, const SplitArgs &a, const HostHandoff &counts)
{
    const unsigned int grid = tileGrid(c, a.tiles);
    unsigned long long *const hostValue = reinterpret_cast<unsigned long long *>(counts.d_value);
    hipLaunchKernelGGL((pfac_split_count<SINGLE, true>), dim3(grid), dim3(kSplitThreads), 0, 0, static_cast<const CutArgs &>(a));
    hipLaunchKernelGGL(pfac_array_scan<unsigned long long>, dim3(1), dim3(1024), 0, 0, a.tileBase, (unsigned int)a.tiles, a.tileBase + a.tiles, hostValue);
    hipLaunchKernelGGL(pfac_split_longest, dim3(1), dim3(1024), 0, 0, a, hostValue ? hostValue + 1 : nullptr);
    if (a.capacity) hipLaunchKernelGGL(pfac_split_write<SINGLE>, dim3(grid), dim3(kSplitThreads), 0, 0, a);
}

} // namespace

extern "C" {

PFAC_status_t PFACX_splitRun(PFAC_handle_t handle, const PFACX_splitRun_t *run, size_t *h_numSegments, size_t *h_longest)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!run || !h_numSegments || !run->d_input || run->size == 0 || (run->capacity && !run->d_offsets) ||
        (run->flags & ~(PFACX_SPLIT_BEFORE | PFACX_SPLIT_RUNS)))
        return PFAC_STATUS_INVALID_PARAMETER;
    const size_t tiles = tilesOf(run->size);
    if (tiles > (size_t)0x7fffffff) return PFAC_STATUS_INVALID_PARAMETER;              /* 2^45 bytes: the scan counts its values in 32 bits */
    PFAC_context *c = handle;
    SplitArgs a{};
    const unsigned int members = fillCutArgs(a, run->d_input, run->size, run->flags, run->cls);
    a.offsets = run->d_offsets;
    a.capacity = run->capacity;
    const PFAC_status_t carved = carveScratch(c->scratch.split, [&](ScratchCarver &k) {
        a.tileBase = k.take<unsigned long long>(tiles + 1);
        a.regionCount = k.take<uint32_t>(tiles * kSplitWaves);
        a.tileFirst = k.take<uint32_t>(tiles);
        a.tileLast = k.take<uint32_t>(tiles);
        a.tileGap = k.take<uint32_t>(tiles);
        a.longest = k.take<unsigned long long>(1);
    });
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    const HostHandoff counts(c, pfac::kHostSplit);                      /* the cuts, then the longest segment */
    dispatchSingle(members, [&](auto single) { splitLaunches<decltype(single)::value>(c, a, counts); });
    unsigned long long v[2] = {0, 0};
    if (!counts.finish(v, a.tileBase + tiles, a.longest)) return PFAC_STATUS_INTERNAL_ERROR;
    if (v[0] >= run->size || v[1] == 0 || v[1] > run->size) return PFAC_STATUS_INTERNAL_ERROR;
    *h_numSegments = (size_t)v[0] + 1;
    if (h_longest) *h_longest = (size_t)v[1];
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
