/*
 * scan_locate.hip -- locate (include/pfac_ext.h: PFACX_locate*, PFACX_matchLocated*): the record and the column of every position of
 * a non-decreasing list, by the cuts of a class D as PFACX_split* defines them (scan_cuts.h: the rule, the tiles, the walk of a region, the count
 * pass; and what this unit shares with scan_capture.hip: kNoPair, firstPairOfItsTile).
 *
 * record(p) = the number of cuts c <= p, column(p) = p - the largest such cut (0: none).  The offsets array of the split is never made: a position
 * needs the cuts in front of its tile (a sum), the last cut in front of its tile (a maximum), and the cuts of its own tile, which only the tiles
 * that hold a position pay for.
 *
 *   pfac_split_count       (scan_cuts.h, without PARTS) grid-stride over the tiles: the tile's cuts (64-bit) and its last cut
 *   pfac_array_scan        (scan_passes.h) the exclusive prefix of the tiles' cuts in place; the total -- the records - 1 -- to the host
 *   pfac_locate_carry      one block over the tiles, one a thread and step: the tile's last cut becomes the last cut IN FRONT of the tile (a block
 *                          prefix under the maximum, blockExclusive, carried from step to step; a position in the input, 0: none -- a cut is never
 *                          0, and 0 is where a record without a cut in front starts); every tile's first pair is set to "none"
 *   pfac_locate_mark       a thread per pair: a position outside [0, n) gets record = column = -1; a pair whose neighbour in front is outside, or
 *                          in another tile, is its tile's FIRST PAIR (scan_cuts.h: firstPairOfItsTile, shared with scan_capture.hip)
 *   pfac_locate_pairs      grid-stride over the tiles.  A tile without a first pair costs that one word.  Else the block walks the tile once
 *                          (splitRegion) and leaves its cuts as a bitmap in LDS, 16 Ki bits = 256 words of 64; a thread per word gives the
 *                          words their exclusive popcount and the last cut in front of them (two block prefixes); then the threads stride over
 *                          the pairs from the first pair on while they lie in the tile: record = the tile's prefix + the word's + the bits of the
 *                          word up to the position; the start = the highest of those bits, else the word's carried cut, else the tile's
 *   pfac_host_done         the call's sequence number to mapped host memory (scan_passes.h: HostHandoff)
 * The list is the caller's and is never trusted: an index into it is below numPairs wherever it comes from, a position indexes a tile only when it
 * lies inside [0, n), and the walk over a tile's pairs ends at the first that lies outside the tile.  A list that is not non-decreasing gets
 * unspecified values (a tile may have several first pairs; one wins), nothing else.
 * One streaming read of the input, a second of the tiles that hold a pair; 4 bytes read and 8 written per pair.
 * SCRATCH, T = ceil(n / 16384) tiles: 8 (T + 1) + 4 T + 4 T bytes (the tiles' cuts and their prefix, the last cut of / in front of a tile, the first
 * pair), each part rounded up to 256 bytes.
 * Plain C++ and vector stores only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_locate.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_cuts.h"

namespace {

constexpr unsigned int kLocateWords = kSplitTile / 64;                   /* the 64-bit words of a tile's bitmap: one per thread */
static_assert(kLocateWords == kSplitThreads, "a thread per word of the bitmap");

struct LocateArgs : CutArgs {           /* n < 2^31: positions, cuts and pair indices fit 32 bits; tileLast: see pfac_locate_carry */
    uint32_t *tileFirstPair;            /* [tiles] the first pair of the list that lies in the tile; kNoPair: none */
    const int *pos;                     /* the caller's list */
    uint32_t numPairs;
    int *record, *column;               /* numPairs entries each; column may be null */
};

__global__ __launch_bounds__(1024) void pfac_locate_carry(LocateArgs a)
{
    __shared__ uint32_t waveMax[16];
    uint32_t carry = 0;                                                  /* the last cut of the steps in front */
    for (size_t base = 0; base < a.tiles; base += 1024) {                /* the same trip count for every thread */
        const size_t i = base + threadIdx.x;
        const uint32_t last = i < a.tiles ? a.tileLast[i] : 0u;
        const uint32_t own = last ? (uint32_t)(i * kSplitTile) + last - 1u : 0u;
        uint32_t total = 0;
        const uint32_t front = OpMax()(carry, blockExclusive<1024>(own, waveMax, total, OpMax()));
        if (i < a.tiles) {
            a.tileLast[i] = front;
            a.tileFirstPair[i] = kNoPair;
        }
        carry = OpMax()(carry, total);
    }
}

__global__ __launch_bounds__(256) void pfac_locate_mark(LocateArgs a)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < a.numPairs; i += (size_t)gridDim.x * 256) {
        const uint32_t p = (uint32_t)a.pos[i];                           /* a negative position is a large one */
        if (p >= a.n) {
            a.record[i] = -1;
            if (a.column != nullptr) a.column[i] = -1;
            continue;
        }
        const uint32_t front = i ? (uint32_t)a.pos[i - 1] : kNoPair;
        if (firstPairOfItsTile(front, p, a.n)) a.tileFirstPair[p / kSplitTile] = (uint32_t)i;
    }
}

template <bool SINGLE>
__global__ __launch_bounds__(kSplitThreads) void pfac_locate_pairs(LocateArgs a)
{
    __shared__ uint32_t cls[8];
    __shared__ unsigned long long words[kLocateWords];                  /* bit b of word w: position 64 w + b of the tile is a cut */
    __shared__ uint32_t wordRank[kLocateWords], wordFront[kLocateWords]; /* the cuts in front of the word; the last of them, position in the tile + 1, 0: none */
    __shared__ uint32_t waveSum[kSplitWaves];
    stageClass<SINGLE>(a, cls);
    unsigned short *const bits16 = reinterpret_cast<unsigned short *>(words);    /* a lane's 16 bits of a trip, where they lie in the words */
    const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (size_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const uint32_t first = a.tileFirstPair[tile];
        if (first >= a.numPairs) continue;                              /* no pair here: the whole block goes on */
        const size_t r0 = tile * kSplitTile + (size_t)wave * kSplitRegion;
        if (r0 < a.n) {
            splitRegion<SINGLE>(a, cls, r0, [&](unsigned int o, uint32_t cut) { bits16[(wave * kSplitRegion + o) >> 4] = (unsigned short)cut; });
        } else {
            for (unsigned int trip = 0; trip < kSplitTrips; trip++) bits16[(wave * kSplitRegion + trip * 1024u + lane * 16u) >> 4] = 0;
        }
        __syncthreads();
        const unsigned long long word = words[threadIdx.x];
        uint32_t total = 0;
        const uint32_t rank = blockExclusive<kSplitThreads>((uint32_t)__popcll(word), waveSum, total);
        const uint32_t lastHere = word ? threadIdx.x * 64u + 64u - (uint32_t)__clzll((long long)word) : 0u;
        const uint32_t front = blockExclusive<kSplitThreads>(lastHere, waveSum, total, OpMax());
        wordRank[threadIdx.x] = rank;
        wordFront[threadIdx.x] = front;
        __syncthreads();
        const uint32_t lo = (uint32_t)(tile * kSplitTile);
        const uint32_t span = a.n - lo < kSplitTile ? (uint32_t)(a.n - lo) : kSplitTile;
        const uint32_t base = (uint32_t)a.tileBase[tile], carried = a.tileLast[tile];
        for (uint32_t i = first + threadIdx.x; i < a.numPairs; i += kSplitThreads) {
            const uint32_t p = (uint32_t)a.pos[i], q = p - lo;
            if (q >= span) break;                                       /* the list has left the tile */
            const uint32_t w = q >> 6;
            const unsigned long long upTo = words[w] & (~0ull >> (63u - (q & 63u)));       /* the cuts of the word at or in front of p */
            a.record[i] = (int)(base + wordRank[w] + (uint32_t)__popcll(upTo));
            if (a.column != nullptr) {
                const uint32_t start = upTo ? lo + w * 64u + 63u - (uint32_t)__clzll((long long)upTo)
                                            : (wordFront[w] ? lo + wordFront[w] - 1u : carried);
                a.column[i] = (int)(p - start);
            }
        }
        __syncthreads();                                                /* the bitmap is rewritten by the next tile */
    }
}

template <bool SINGLE>
void locateLaunches(const PFAC_context *c, const LocateArgs &a, const HostHandoff &count)
{
    const unsigned int grid = tileGrid(c, a.tiles);
    hipLaunchKernelGGL((pfac_split_count<SINGLE, false>), dim3(grid), dim3(kSplitThreads), 0, 0, static_cast<const CutArgs &>(a));
    hipLaunchKernelGGL(pfac_array_scan<unsigned long long>, dim3(1), dim3(1024), 0, 0, a.tileBase, (unsigned int)a.tiles, a.tileBase + a.tiles,
                       reinterpret_cast<unsigned long long *>(count.d_value));
    if (a.numPairs == 0) return;                                         /* the count query */
    hipLaunchKernelGGL(pfac_locate_carry, dim3(1), dim3(1024), 0, 0, a);
    hipLaunchKernelGGL(pfac_locate_mark, dim3(gridFor(c, a.numPairs)), dim3(256), 0, 0, a);
    hipLaunchKernelGGL(pfac_locate_pairs<SINGLE>, dim3(grid), dim3(kSplitThreads), 0, 0, a);
}

} // namespace

extern "C" {

PFAC_status_t PFACX_locateRun(PFAC_handle_t handle, const PFACX_locateRun_t *run, size_t *h_numRecords)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!run || !h_numRecords || !run->d_input || run->size == 0 || run->size > (size_t)0x7fffffff || run->numPairs > (size_t)0x7fffffff ||
        (run->numPairs && (!run->d_pos || !run->d_record)) || (run->flags & ~(PFACX_SPLIT_BEFORE | PFACX_SPLIT_RUNS)))
        return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = handle;
    LocateArgs a{};
    const unsigned int members = fillCutArgs(a, run->d_input, run->size, run->flags, run->cls);
    const size_t tiles = a.tiles;
    a.pos = run->d_pos;
    a.numPairs = (uint32_t)run->numPairs;
    a.record = run->d_record;
    a.column = run->d_column;
    const PFAC_status_t carved = carveScratch(c->scratch.locate, [&](ScratchCarver &k) {
        a.tileBase = k.take<unsigned long long>(tiles + 1);
        a.tileLast = k.take<uint32_t>(tiles);
        a.tileFirstPair = k.take<uint32_t>(tiles);
    });
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    const HostHandoff count(c, pfac::kHostLocate);                      /* the cuts */
    dispatchSingle(members, [&](auto single) { locateLaunches<decltype(single)::value>(c, a, count); });
    unsigned long long cuts = 0;
    if (!count.finish(&cuts, a.tileBase + tiles)) return PFAC_STATUS_INTERNAL_ERROR;
    if (cuts >= run->size) return PFAC_STATUS_INTERNAL_ERROR;
    *h_numRecords = (size_t)cuts + 1;
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
