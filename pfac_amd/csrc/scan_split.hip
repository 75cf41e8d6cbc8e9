/*
 * scan_split.hip -- split (include/pfac_ext.h: PFACX_split*): the offsets that cut a buffer into records at the bytes of a class D.
 *
 * Let the input have n bytes, a = (in[c - 1] is in D), b = (in[c] is in D).  Position c of [1, n - 1] is a CUT if
 *   flags 0: a        PFACX_SPLIT_BEFORE: b        PFACX_SPLIT_RUNS: a and not b        both: b and not a
 * -- the four rules of the header in one form: a cut needs its own byte and the byte in front of it, nothing else.  The offsets are 0, the cuts
 * ascending, n.
 *
 * The input is cut into TILES of kSplitTile = 16 KiB, a tile into four REGIONS of 4 KiB, one per wave of a block of 256 threads; a wave takes its
 * region in four trips of 1 KiB, 16 bytes a lane (loadBytes16: any alignment of the caller's pointer; the 16 bytes that hang over the input's end
 * byte by byte).  16 bytes become 16 delimiter bits -- a class of one byte by the exact SWAR compare of scan_passes.h, any other class by a lookup
 * in the 256-bit table in LDS (eight words, eight banks: lanes that ask for the same word are served together) -- and, with the top bit of the
 * lane in front (a shuffle; lane 0: the top bit of the trip in front, carried in a register; trip 0: one byte read in front of the region, which
 * is how a run crosses a region's or a tile's edge), 16 cut bits.  Nothing passes from wave to wave but sums.
 *
 *   pfac_split_count       grid-stride over the tiles.  Per region: the cuts, the first and the last of them, the longest distance between two
 *                          neighbours; thread 0 joins the four regions of the tile in order.  Writes the tile's cuts (64-bit), the cuts of each
 *                          region, the tile's first and last cut (position in the tile + 1; 0: none) and its longest inner distance
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
#include "scan_passes.h"

namespace {

constexpr unsigned int kSplitThreads = 256;                              /* four waves, a region each */
constexpr unsigned int kSplitWaves = kSplitThreads / 64;
constexpr unsigned int kSplitTrips = 4;                                  /* 1 KiB a trip: 16 bytes a lane */
constexpr unsigned int kSplitRegion = kSplitTrips * 64 * 16;             /* 4 KiB */
constexpr unsigned int kSplitTile = kSplitWaves * kSplitRegion;          /* 16 KiB (pfac_amd/api.py: PFACX_SPLIT_TILE) */
constexpr unsigned int kSplitPerThread = 4;                              /* tiles a thread of pfac_split_longest takes per trip */
static_assert(kSplitTile == 16384, "the header's scratch formula and PFACX_SPLIT_TILE say 16384");

struct SplitArgs {
    const unsigned char *in;            /* the caller's bytes */
    size_t n;
    size_t tiles;
    uint32_t cls[8];                    /* bit b & 31 of cls[b >> 5]: byte b is a delimiter */
    uint32_t rep;                       /* a class of one byte: that byte in all four places */
    uint32_t flags;
    unsigned long long *tileBase;       /* [tiles + 1] cuts per tile -> the cuts in front of the tile; [tiles] = all cuts */
    uint32_t *regionCount;              /* [tiles * 4] cuts per region */
    uint32_t *tileFirst, *tileLast;     /* [tiles] position in the tile + 1 of its first / last cut; 0: none */
    uint32_t *tileGap;                  /* [tiles] the longest distance between two neighbouring cuts of the tile */
    unsigned long long *longest;        /* one word */
    size_t *offsets;
    size_t capacity;
};

/* is byte b a delimiter */
template <bool SINGLE>
__device__ __forceinline__ uint32_t isDelimiter(const SplitArgs &a, const uint32_t *cls, uint32_t b)
{
    if constexpr (SINGLE) return b == (a.rep & 0xFFu) ? 1u : 0u;
    else return (cls[b >> 5] >> (b & 31u)) & 1u;
}

/* bit k: byte k of the 16 in v is a delimiter */
template <bool SINGLE>
__device__ __forceinline__ uint32_t delimiterBits(const SplitArgs &a, const uint32_t *cls, pfacmod::u32x4 v)
{
    if constexpr (SINGLE) {
        return bytesEqual4(v.x, a.rep) | bytesEqual4(v.y, a.rep) << 4 | bytesEqual4(v.z, a.rep) << 8 | bytesEqual4(v.w, a.rep) << 12;
    } else {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t d = 0;
#pragma unroll
        for (unsigned int k = 0; k < 16; k++) d |= isDelimiter<false>(a, cls, (w[k >> 2] >> (8 * (k & 3))) & 0xFFu) << k;
        return d;
    }
}

/* The region that starts at input byte r0 < n, by one wave: visit(o, cut) once per trip in every lane -- o: the lane's first byte, counted from r0;
 * bit k of cut: r0 + o + k is a cut.  Bits are set for positions of [1, n - 1] only */
template <bool SINGLE, class Visit>
__device__ __forceinline__ void splitRegion(const SplitArgs &a, const uint32_t *cls, size_t r0, Visit visit)
{
    const unsigned int lane = threadIdx.x & 63u;
    /* loadBytes16 counts in 32 bits and reads aligned blocks around what it is asked for: it gets the region as a buffer of its own that starts up
     * to 16 bytes in front of r0 and ends up to 16 bytes behind the region, all of it inside the input */
    const unsigned int back = r0 < 16 ? (unsigned int)r0 : 16u;
    const unsigned char *const base = a.in + (r0 - back);
    const size_t left = a.n - r0;
    const unsigned int local = back + (left < kSplitRegion + 16u ? (unsigned int)left : kSplitRegion + 16u);
    uint32_t carry = r0 > 0 ? isDelimiter<SINGLE>(a, cls, a.in[r0 - 1]) : 0u;             /* the byte in front of the region: the neighbour's */
#pragma unroll
    for (unsigned int trip = 0; trip < kSplitTrips; trip++) {
        const unsigned int o = trip * 1024u + lane * 16u;
        const size_t have = left > o ? left - o : 0;                                       /* input bytes from the lane's first on */
        const uint32_t valid = have >= 16 ? 0xFFFFu : (1u << (unsigned int)have) - 1u;
        uint32_t d = 0;
        if (have >= 16) {
            d = delimiterBits<SINGLE>(a, cls, loadBytes16(base, local, back + o));
        } else {
            for (unsigned int k = 0; k < (unsigned int)have; k++) d |= isDelimiter<SINGLE>(a, cls, a.in[r0 + o + k]) << k;
        }
        const uint32_t top = d >> 15;
        const uint32_t up = (uint32_t)__shfl_up((int)top, 1);
        const uint32_t front = ((d << 1) | (lane == 0 ? carry : up)) & 0xFFFFu;            /* bit k: the byte in front of byte k is a delimiter */
        carry = (uint32_t)__shfl((int)top, 63);
        uint32_t cut = (a.flags & PFACX_SPLIT_RUNS) ? ((a.flags & PFACX_SPLIT_BEFORE) ? d & ~front : front & ~d)
                                                    : ((a.flags & PFACX_SPLIT_BEFORE) ? d : front);
        cut &= valid;
        if (r0 == 0 && o == 0) cut &= ~1u;                                                 /* position 0 is no cut */
        visit(o, cut);
    }
}

/* the class table in LDS (a class of one byte never reads it) */
template <bool SINGLE>
__device__ __forceinline__ void stageClass(const SplitArgs &a, uint32_t *cls)
{
    if constexpr (!SINGLE) {
        if (threadIdx.x < 8) cls[threadIdx.x] = a.cls[threadIdx.x];
        __syncthreads();
    }
}

template <bool SINGLE>
__global__ __launch_bounds__(kSplitThreads) void pfac_split_count(SplitArgs a)
{
    __shared__ uint32_t cls[8];
    __shared__ uint32_t region[kSplitWaves][4];                         /* count, first, last, gap of each region of the tile */
    stageClass<SINGLE>(a, cls);
    const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (size_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const size_t r0 = tile * kSplitTile + (size_t)wave * kSplitRegion;
        /* positions + 1 inside the region, 0: none.  count and gap per lane, first in the one lane that saw it, last the same in every lane */
        uint32_t count = 0, first = 0, last = 0, gap = 0;
        if (r0 < a.n) {
            splitRegion<SINGLE>(a, cls, r0, [&](unsigned int o, uint32_t cut) {
                count += (uint32_t)__popc(cut);
                const uint32_t lastHere = cut ? o + 32u - (uint32_t)__clz((int)cut) : 0u;
                const uint32_t incl = waveInclusive(lastHere, OpMax());
                const uint32_t prev = OpMax()(last, waveExclusiveOf(incl));                /* the last cut in front of this lane's bytes */
                if (cut) {
                    const uint32_t firstHere = o + (uint32_t)__ffs((int)cut);
                    if (prev) gap = OpMax()(gap, firstHere - prev);
                    else first = firstHere;
                    for (uint32_t x = cut; x & (x - 1u); x &= x - 1u)                      /* neighbours inside the lane's 16 bytes */
                        gap = OpMax()(gap, (uint32_t)(__ffs((int)(x & (x - 1u))) - __ffs((int)x)));
                }
                last = OpMax()(last, (uint32_t)__shfl((int)incl, 63));
            });
            count = waveReduce(count, OpSum());
            first = waveReduce(first, OpMax());
            gap = waveReduce(gap, OpMax());
        }
        if (lane == 0) {
            a.regionCount[tile * kSplitWaves + wave] = count;
            region[wave][0] = count; region[wave][1] = first; region[wave][2] = last; region[wave][3] = gap;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t tCount = 0, tFirst = 0, tLast = 0, tGap = 0;
            for (unsigned int w = 0; w < kSplitWaves; w++) {
                tCount += region[w][0];
                tGap = OpMax()(tGap, region[w][3]);
                if (region[w][1] != 0) {
                    const uint32_t f = w * kSplitRegion + region[w][1];
                    if (tLast) tGap = OpMax()(tGap, f - tLast);
                    else tFirst = f;
                    tLast = w * kSplitRegion + region[w][2];
                }
            }
            a.tileBase[tile] = tCount;
            a.tileFirst[tile] = tFirst;
            a.tileLast[tile] = tLast;
            a.tileGap[tile] = tGap;
        }
        __syncthreads();                                                /* region is rewritten by the next tile */
    }
}

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
    const size_t cap = gridCap(c, 8);
    const unsigned int grid = (unsigned int)(a.tiles < cap ? a.tiles : cap);
    unsigned long long *const hostValue = reinterpret_cast<unsigned long long *>(counts.d_value);
    hipLaunchKernelGGL(pfac_split_count<SINGLE>, dim3(grid), dim3(kSplitThreads), 0, 0, a);
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
    const size_t tiles = (run->size - 1) / kSplitTile + 1;
    if (tiles > (size_t)0x7fffffff) return PFAC_STATUS_INVALID_PARAMETER;              /* 2^45 bytes: the scan counts its values in 32 bits */
    PFAC_context *c = handle;
    SplitArgs a{};
    a.in = reinterpret_cast<const unsigned char *>(run->d_input);
    a.n = run->size;
    a.tiles = tiles;
    a.flags = run->flags;
    a.offsets = run->d_offsets;
    a.capacity = run->capacity;
    unsigned int members = 0, only = 0;
    for (unsigned int k = 0; k < 8; k++) {
        a.cls[k] = run->cls[k];
        members += (unsigned int)__builtin_popcount(run->cls[k]);
        if (run->cls[k]) only = k * 32u + (unsigned int)__builtin_ctz(run->cls[k]);
    }
    a.rep = only * 0x01010101u;
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
    if (members == 1) splitLaunches<true>(c, a, counts);
    else splitLaunches<false>(c, a, counts);
    unsigned long long v[2] = {0, 0};
    if (!counts.finish(v, a.tileBase + tiles, a.longest)) return PFAC_STATUS_INTERNAL_ERROR;
    if (v[0] >= run->size || v[1] == 0 || v[1] > run->size) return PFAC_STATUS_INTERNAL_ERROR;
    *h_numSegments = (size_t)v[0] + 1;
    if (h_longest) *h_longest = (size_t)v[1];
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
