/*
 * scan_cuts.h -- the cuts of a buffer at the bytes of a class D, as scan_split.hip (PFACX_split*) and scan_locate.hip (PFACX_locate*) both need
 * them: the one statement of the cut rule on the device; and the tiles of a pair list, as scan_locate.hip and scan_capture.hip (PFACX_capture*)
 * both walk them.
 *
 * Let the input have n bytes, a = (in[c - 1] is in D), b = (in[c] is in D).  Position c of [1, n - 1] is a CUT if
 *   flags 0: a        PFACX_SPLIT_BEFORE: b        PFACX_SPLIT_RUNS: a and not b        both: b and not a
 * -- the four rules of the header in one form: a cut needs its own byte and the byte in front of it, nothing else.
 *
 * The input is cut into TILES of kSplitTile = 16 KiB, a tile into four REGIONS of 4 KiB, one per wave of a block of 256 threads; a wave takes its
 * region in four trips of 1 KiB, 16 bytes a lane (loadBytes16: any alignment of the caller's pointer; the 16 bytes that hang over the input's end
 * byte by byte).  16 bytes become 16 delimiter bits -- a class of one byte by the exact SWAR compare of scan_passes.h, any other class by a lookup
 * in the 256-bit table in LDS (eight words, eight banks: lanes that ask for the same word are served together) -- and, with the top bit of the
 * lane in front (a shuffle; lane 0: the top bit of the trip in front, carried in a register; trip 0: one byte read in front of the region, which
 * is how a run crosses a region's or a tile's edge), 16 cut bits.  Nothing passes from wave to wave but sums.
 *
 * Here, for all three units: the tile constants, the arguments every pass starts with and their fill (CutArgs, tilesOf, fillCutArgs), the grid of a
 * block-per-tile launch (tileGrid), the choice of the SINGLE form (dispatchSingle), the class test (isDelimiter, delimiterBits, stageClass).  THE
 * CUTS, split and locate: the walk of a region (splitRegion) and the count pass (pfac_split_count).  THE TILES OF A PAIR LIST, locate and capture:
 * kNoPair and the first-pair rule (firstPairOfItsTile); the mark and the pairs kernels themselves stay in the two units.  Like scan_passes.h,
 * everything is in an unnamed namespace: each unit its own copy.
 */
#ifndef PFAC_SCAN_CUTS_H_
#define PFAC_SCAN_CUTS_H_

#include <algorithm>
#include <type_traits>

#include "scan_passes.h"

namespace {

/* ------------------------------------------------------------------ the tiles and the class */

constexpr unsigned int kSplitThreads = 256;                              /* four waves, a region each */
constexpr unsigned int kSplitWaves = kSplitThreads / 64;
constexpr unsigned int kSplitTrips = 4;                                  /* 1 KiB a trip: 16 bytes a lane */
constexpr unsigned int kSplitRegion = kSplitTrips * 64 * 16;             /* 4 KiB */
constexpr unsigned int kSplitTile = kSplitWaves * kSplitRegion;          /* 16 KiB (pfac_amd/api.py: PFACX_SPLIT_TILE) */
static_assert(kSplitTile == 16384, "the header's scratch formulas and PFACX_SPLIT_TILE say 16384");

struct CutArgs {
    const unsigned char *in;            /* the caller's bytes */
    size_t n;
    size_t tiles;
    uint32_t cls[8];                    /* bit b & 31 of cls[b >> 5]: byte b is a delimiter */
    uint32_t rep;                       /* a class of one byte: that byte in all four places */
    uint32_t flags;
    unsigned long long *tileBase;       /* [tiles + 1] cuts per tile -> the cuts in front of the tile; [tiles] = all cuts */
    uint32_t *tileLast;                 /* [tiles] position in the tile + 1 of its last cut; 0: none */
    /* what only a pass with PARTS writes (the split) */
    uint32_t *regionCount;              /* [tiles * 4] cuts per region */
    uint32_t *tileFirst;                /* [tiles] position in the tile + 1 of its first cut; 0: none */
    uint32_t *tileGap;                  /* [tiles] the longest distance between two neighbouring cuts of the tile */
};

inline size_t tilesOf(size_t size) { return (size - 1) / kSplitTile + 1; }                /* size > 0 */

/* what every ...Run entry fills first: the input, its tiles, the flags, the class into a.cls and a.rep; returns the number of the class's members */
inline unsigned int fillCutArgs(CutArgs &a, const char *d_input, size_t size, unsigned int flags, const unsigned int *cls)
{
    a.in = reinterpret_cast<const unsigned char *>(d_input);
    a.n = size;
    a.tiles = tilesOf(size);
    a.flags = flags;
    const pfac::ByteClass d(cls);
    d.copyTo(a.cls);
    a.rep = d.only * 0x01010101u;
    return d.members;
}

/* the blocks of a launch that takes a block per tile, grid-stride: eight per compute unit at most */
inline unsigned int tileGrid(const PFAC_context *c, size_t tiles) { return (unsigned int)std::min<size_t>(tiles, gridCap(c, 8)); }

/* f(std::true_type) for a class of one member -- the SINGLE form of every pass --, f(std::false_type) for any other */
template <class F>
inline void dispatchSingle(unsigned int members, F f) { members == 1 ? f(std::true_type()) : f(std::false_type()); }

/* is byte b a delimiter */
template <bool SINGLE>
__device__ __forceinline__ uint32_t isDelimiter(const CutArgs &a, const uint32_t *cls, uint32_t b)
{
    if constexpr (SINGLE) return b == (a.rep & 0xFFu) ? 1u : 0u;
    else return (cls[b >> 5] >> (b & 31u)) & 1u;
}

/* bit k: byte k of the 16 in v is a delimiter */
template <bool SINGLE>
__device__ __forceinline__ uint32_t delimiterBits(const CutArgs &a, const uint32_t *cls, pfacmod::u32x4 v)
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

/* the class table in LDS (a class of one byte never reads it) */
template <bool SINGLE>
__device__ __forceinline__ void stageClass(const CutArgs &a, uint32_t *cls)
{
    if constexpr (!SINGLE) {
        if (threadIdx.x < 8) cls[threadIdx.x] = a.cls[threadIdx.x];
        __syncthreads();
    }
}

/* ------------------------------------------------------------------ the cuts */

/* The region that starts at input byte r0 < n, by one wave: visit(o, cut) once per trip in every lane -- o: the lane's first byte, counted from r0;
 * bit k of cut: r0 + o + k is a cut.  Bits are set for positions of [1, n - 1] only */
template <bool SINGLE, class Visit>
__device__ __forceinline__ void splitRegion(const CutArgs &a, const uint32_t *cls, size_t r0, Visit visit)
{
    const unsigned int lane = threadIdx.x & 63u;
    /* loadBytes16 counts in 32 bits and reads aligned blocks around what it is asked for: it gets the region as a buffer of its own that starts up
     * to 16 bytes in front of r0 and ends up to 16 bytes behind the region, all of it inside the input (scan_capture.hip: the same for a tile) */
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

/* The count pass, grid-stride over the tiles.  Per region: the cuts and the last of them and, with PARTS, the first and the longest distance
 * between two neighbours; thread 0 joins the four regions of the tile in order.  Writes the tile's cuts (64-bit) and its last cut (position in the
 * tile + 1; 0: none) and, with PARTS, the cuts of each region, the tile's first cut and its longest inner distance */
template <bool SINGLE, bool PARTS>
__global__ __launch_bounds__(kSplitThreads) void pfac_split_count(CutArgs a)
{
    __shared__ uint32_t cls[8];
    __shared__ uint32_t region[kSplitWaves][4];                         /* count, first, last, gap of each region of the tile */
    stageClass<SINGLE>(a, cls);
    const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (size_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const size_t r0 = tile * kSplitTile + (size_t)wave * kSplitRegion;
        /* positions + 1 inside the region, 0: none.  count and gap per lane, first in the one lane that saw it, last the same in every lane (without
         * PARTS: per lane until the region is through) */
        uint32_t count = 0, first = 0, last = 0, gap = 0;
        if (r0 < a.n) {
            splitRegion<SINGLE>(a, cls, r0, [&](unsigned int o, uint32_t cut) {
                count += (uint32_t)__popc(cut);
                const uint32_t lastHere = cut ? o + 32u - (uint32_t)__clz((int)cut) : 0u;
                if constexpr (PARTS) {
                    const uint32_t incl = waveInclusive(lastHere, OpMax());
                    const uint32_t prev = OpMax()(last, waveExclusiveOf(incl));            /* the last cut in front of this lane's bytes */
                    if (cut) {
                        const uint32_t firstHere = o + (uint32_t)__ffs((int)cut);
                        if (prev) gap = OpMax()(gap, firstHere - prev);
                        else first = firstHere;
                        for (uint32_t x = cut; x & (x - 1u); x &= x - 1u)                  /* neighbours inside the lane's 16 bytes */
                            gap = OpMax()(gap, (uint32_t)(__ffs((int)(x & (x - 1u))) - __ffs((int)x)));
                    }
                    last = OpMax()(last, (uint32_t)__shfl((int)incl, 63));
                } else {
                    last = OpMax()(last, lastHere);
                }
            });
            count = waveReduce(count, OpSum());
            if constexpr (PARTS) {
                first = waveReduce(first, OpMax());
                gap = waveReduce(gap, OpMax());
            } else {
                last = waveReduce(last, OpMax());
            }
        }
        if (lane == 0) {
            if constexpr (PARTS) a.regionCount[tile * kSplitWaves + wave] = count;
            region[wave][0] = count; region[wave][1] = first; region[wave][2] = last; region[wave][3] = gap;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t tCount = 0, tFirst = 0, tLast = 0, tGap = 0;
            for (unsigned int w = 0; w < kSplitWaves; w++) {
                tCount += region[w][0];
                if constexpr (PARTS) {
                    tGap = OpMax()(tGap, region[w][3]);
                    if (region[w][1] != 0) {
                        const uint32_t f = w * kSplitRegion + region[w][1];
                        if (tLast) tGap = OpMax()(tGap, f - tLast);
                        else tFirst = f;
                        tLast = w * kSplitRegion + region[w][2];
                    }
                } else if (region[w][2] != 0) {
                    tLast = w * kSplitRegion + region[w][2];
                }
            }
            a.tileBase[tile] = tCount;
            a.tileLast[tile] = tLast;
            if constexpr (PARTS) {
                a.tileFirst[tile] = tFirst;
                a.tileGap[tile] = tGap;
            }
        }
        __syncthreads();                                                /* region is rewritten by the next tile */
    }
}

/* ------------------------------------------------------------------ the tiles of a pair list */

/* A non-decreasing list of positions, tiled by position, as scan_locate.hip and scan_capture.hip walk one: a mark pass, a thread per pair, answers
 * the positions outside [0, n) and writes every tile's FIRST PAIR into a word per tile (kNoPair: none); a pairs kernel, a block per tile, reads the
 * word, goes on -- the whole block, in front of the tile's first barrier -- if it is >= numPairs, and strides over the list from there until a
 * position leaves the tile.  The list is the caller's and is never trusted: an index into it is below numPairs wherever it comes from, and a
 * position names a tile only inside [0, n).  Shared here are the constant and the rule; the loops stay in the kernels of both units, whose
 * generated code -- pfac_capture_pairs sits at the scalar-register limit -- is then the same as without this header
 * (profiles/pair_tiles_refactor_resources.txt) */
constexpr uint32_t kNoPair = 0xFFFFFFFFu;

/* is the pair at position p < n, whose neighbour in front in the list is at `front` (kNoPair: it has none; a negative position is a large one),
 * its tile's first pair: the neighbour lies outside the input, or in another tile */
__device__ __forceinline__ bool firstPairOfItsTile(uint32_t front, uint32_t p, size_t n) { return front >= n || front / kSplitTile != p / kSplitTile; }

} // namespace

#endif /* PFAC_SCAN_CUTS_H_ */
