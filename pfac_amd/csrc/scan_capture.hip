/*
 * scan_capture.hip -- capture (include/pfac_ext.h: PFACX_capture*, PFACX_matchCaptured*): the value behind every match of a
 * non-decreasing pair list -- from the end of the match over the bytes of a skip class S \ D to the first byte of a stop class D, inside a window.
 *
 * For pair (id, p) with p inside [0, n): b = min(p + len(id), n) (PFACX_CAPTURE_AT_POS: b = p), w = n or min(n, b + window); s = the first position of
 * [b, w) whose byte is not in S \ D, e = the first of [s, w) whose byte is in D, w where there is none; valStart = s, valLen = e - s.  Both searches
 * are "the first byte of a class": of GO = the complement of S \ D, then of D.
 *
 * A value needs nothing from in front of its tile, so there is no pass over the whole input: the list is tiled by p -- the non-decreasing quantity;
 * b is not, a long pattern at a lower position can end behind a short one at a higher position -- and only the tiles of 16 KiB (scan_cuts.h:
 * kSplitTile) that hold a pair are read.
 *
 *   pfac_capture_clear     every tile's first pair to "none", the slow-path count to 0
 *   pfac_capture_mark      a thread per pair (the pass of scan_locate.hip with the answers of this call): a position outside [0, n) gets (-1, 0);
 *                          the first pair of every tile is marked (scan_cuts.h: firstPairOfItsTile)
 *   pfac_capture_pairs     grid-stride over the tiles.  A tile without a first pair costs that one word.  Else the block reads the tile and the
 *                          kCaptureReach bytes behind it once, 16 bytes a thread and step (loadBytes16: any alignment; what hangs over the input's
 *                          end byte by byte), and leaves two bitmaps in LDS, "byte in D" and "byte in GO", 2 x (16 Ki + reach) bits; bits at and
 *                          beyond n read 1 in both, so the input's end is a stop byte like any other.  Then the threads stride over the pairs from
 *                          the first pair on while they lie in the tile: the length of the id (one gathered load, the id checked first), b and w,
 *                          s by find-first-set over the 64-bit words of the second bitmap from bit b, e over the first from s, both cut at w.
 *                          THE SLOW PATH: a pair whose b lies behind the bitmap, or whose search reaches the bitmap's last bit without an answer
 *                          while w lies beyond it, goes on over the input itself up to w, a lane alone, aligned 8 bytes a load, through the two
 *                          class tables in LDS.  Such pairs are counted
 *   pfac_capture_finish    the count to mapped host memory
 *   pfac_host_done         the call's sequence number behind it (scan_passes.h: HostHandoff)
 * The class walk is not splitRegion: that hands out the CUT bits of one class under the split's flags (never a bit for position 0, the byte in
 * front carried from lane to lane), this call wants the plain class bits of two classes out of one load and no neighbour.  From scan_cuts.h: the tile
 * constants, fillCutArgs, tileGrid, dispatchSingle, the class test (delimiterBits: the exact SWAR compare for a D of one byte, the 256-bit table in
 * LDS else; GO always through its table) and, of the tiles of a pair list, kNoPair and the first-pair rule (firstPairOfItsTile).
 * The list is the caller's and is never trusted: an index into it is below numPairs wherever it comes from, a position indexes a tile only when it
 * lies inside [0, n), an id indexes the lengths only when it lies inside [1, numLens), and the walk over a tile's pairs ends at the first that lies
 * outside the tile.  A list that is not non-decreasing gets unspecified values, nothing else.
 * SCRATCH, T = ceil(n / 16384) tiles: 4 T + 8 bytes (the first pairs, the slow-path count), each part rounded up to 256.
 * Plain C++ and vector stores only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_capture.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_cuts.h"

namespace {

constexpr unsigned int kCaptureReach = PFACX_CAPTURE_REACH;            /* the bytes behind a tile that its bitmaps cover: one more trip of the walk */
constexpr unsigned int kCaptureBits = kSplitTile + kCaptureReach;       /* the bits of a bitmap */
constexpr unsigned int kCaptureWords = kCaptureBits / 64;               /* ... its 64-bit words */
constexpr unsigned int kCaptureChunks = kCaptureBits / 16;              /* ... the 16 bytes of a thread and step */
static_assert(kCaptureReach % 64 == 0 && kCaptureReach >= 64, "whole words of the bitmap");

struct CaptureArgs : CutArgs {          /* in, n < 2^31, tiles; cls and rep: the stop class D */
    uint32_t go[8];                     /* the complement of S \ D: where the skip ends */
    unsigned long long window;          /* 0: none */
    uint32_t atPos;                     /* PFACX_CAPTURE_AT_POS */
    uint32_t *tileFirstPair;            /* [tiles] the first pair of the list that lies in the tile; kNoPair: none */
    unsigned long long *slowPairs;      /* the pairs that finished on the input itself */
    const int *ids, *pos;               /* the caller's list; ids null with atPos */
    uint32_t numPairs;
    const int *patternLen;              /* [numLens] by id */
    uint32_t numLens;
    int *valStart, *valLen;             /* numPairs entries each */
};

__global__ __launch_bounds__(256) void pfac_capture_clear(CaptureArgs a)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < a.tiles; i += (size_t)gridDim.x * 256) a.tileFirstPair[i] = kNoPair;
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.slowPairs = 0;
}

__global__ __launch_bounds__(256) void pfac_capture_mark(CaptureArgs a)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < a.numPairs; i += (size_t)gridDim.x * 256) {
        const uint32_t p = (uint32_t)a.pos[i];                           /* a negative position is a large one */
        if (p >= a.n) {
            a.valStart[i] = -1;
            a.valLen[i] = 0;
            continue;
        }
        const uint32_t front = i ? (uint32_t)a.pos[i - 1] : kNoPair;
        if (firstPairOfItsTile(front, p, a.n)) a.tileFirstPair[p / kSplitTile] = (uint32_t)i;
    }
}

/* the first set bit of [from, to) of a bitmap, to if there is none; from <= to <= kCaptureBits */
__device__ __forceinline__ uint32_t firstBit(const unsigned long long *words, uint32_t from, uint32_t to)
{
    if (from >= to) return to;
    uint32_t w = from >> 6;
    const uint32_t lastWord = (to - 1u) >> 6;
    unsigned long long x = words[w] & (~0ull << (from & 63u));
    while (x == 0 && w < lastWord) x = words[++w];
    if (x == 0) return to;
    const uint32_t at = w * 64u + (uint32_t)__ffsll((long long)x) - 1u;
    return at < to ? at : to;
}

/* the slow path: the first position of [x, w) of the input whose byte is in the class `table` (LDS), w if there is none; x <= w <= n.  A lane
 * alone: bytes up to an aligned address, aligned 8 bytes a load, bytes again */
__device__ uint32_t firstByteOf(const unsigned char *in, const uint32_t *table, uint32_t x, uint32_t w)
{
    const auto isIn = [&](uint32_t b) { return (table[b >> 5] >> (b & 31u)) & 1u; };
    while (x < w && (reinterpret_cast<uintptr_t>(in + x) & 7u) != 0) {
        if (isIn(in[x])) return x;
        x++;
    }
    while (w - x >= 8u) {
        const unsigned long long v = *reinterpret_cast<const unsigned long long *>(in + x);
#pragma unroll
        for (unsigned int k = 0; k < 8; k++)
            if (isIn((uint32_t)(v >> (8 * k)) & 0xFFu)) return x + k;
        x += 8u;
    }
    while (x < w) {
        if (isIn(in[x])) return x;
        x++;
    }
    return w;
}

template <bool SINGLE>
__global__ __launch_bounds__(kSplitThreads) void pfac_capture_pairs(CaptureArgs a)
{
    __shared__ uint32_t stopTable[8], goTable[8];
    __shared__ unsigned long long stopWords[kCaptureWords], goWords[kCaptureWords];     /* bit k: byte lo + k of the input is in D / in GO */
    __shared__ uint32_t slowHere;
    if (threadIdx.x < 8) {                                              /* both tables always: the slow path reads them whatever SINGLE says */
        stopTable[threadIdx.x] = a.cls[threadIdx.x];
        goTable[threadIdx.x] = a.go[threadIdx.x];
    }
    if (threadIdx.x == 0) slowHere = 0;
    __syncthreads();
    unsigned short *const stop16 = reinterpret_cast<unsigned short *>(stopWords);       /* a thread's 16 bits of a step, where they lie in the words */
    unsigned short *const go16 = reinterpret_cast<unsigned short *>(goWords);
    const uint32_t n = (uint32_t)a.n;
    for (size_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const uint32_t first = a.tileFirstPair[tile];
        if (first >= a.numPairs) continue;                              /* no pair here: the whole block goes on */
        const uint32_t lo = (uint32_t)(tile * kSplitTile);              /* < n */
        /* the window of splitRegion (scan_cuts.h has the reason) around the tile and its reach, in 32 bits */
        const uint32_t back = lo < 16u ? lo : 16u;
        const unsigned char *const base = a.in + (lo - back);
        const uint32_t left = n - lo;
        const uint32_t local = back + (left < kCaptureBits + 16u ? left : kCaptureBits + 16u);
        for (uint32_t chunk = threadIdx.x; chunk < kCaptureChunks; chunk += kSplitThreads) {
            const uint32_t o = chunk * 16u;
            const uint32_t have = left > o ? left - o : 0u;             /* input bytes from the thread's first on */
            uint32_t d = 0, g = 0;
            if (have >= 16u) {
                const pfacmod::u32x4 v = loadBytes16(base, local, back + o);
                d = delimiterBits<SINGLE>(a, stopTable, v);
                g = delimiterBits<false>(a, goTable, v);
            } else {
                for (uint32_t k = 0; k < have; k++) {
                    const uint32_t byte = a.in[lo + o + k];
                    d |= isDelimiter<SINGLE>(a, stopTable, byte) << k;
                    g |= isDelimiter<false>(a, goTable, byte) << k;
                }
                const uint32_t beyond = 0xFFFFu & ~((1u << have) - 1u); /* at and beyond n: a stop byte, and no skip byte */
                d |= beyond;
                g |= beyond;
            }
            stop16[chunk] = (unsigned short)d;
            go16[chunk] = (unsigned short)g;
        }
        __syncthreads();
        const uint32_t span = left < kSplitTile ? left : kSplitTile;
        const uint32_t hi = lo + kCaptureBits;                          /* the bitmaps cover [lo, hi); n < 2^31: no wrap */
        for (uint32_t i = first + threadIdx.x; i < a.numPairs; i += kSplitThreads) {
            const uint32_t p = (uint32_t)a.pos[i];
            if (p - lo >= span) break;                                  /* the list has left the tile */
            unsigned long long bWide = p;
            if (!a.atPos) {
                const int id = a.ids[i];
                if (id < 1 || (uint32_t)id >= a.numLens) {              /* no such pattern: nothing */
                    a.valStart[i] = -1;
                    a.valLen[i] = 0;
                    continue;
                }
                const int len = a.patternLen[id];
                bWide += len > 0 ? (unsigned long long)len : 0ull;
            }
            const uint32_t b = bWide < n ? (uint32_t)bWide : n;
            const uint32_t w = a.window == 0 || a.window >= (unsigned long long)(n - b) ? n : b + (uint32_t)a.window;
            const uint32_t mapEnd = w < hi ? w : hi;                    /* where the bitmaps answer up to */
            bool slow = false;
            uint32_t s;
            if (b >= hi) {                                              /* a pattern longer than the reach */
                slow = b < w;
                s = firstByteOf(a.in, goTable, b, w);
            } else {
                s = lo + firstBit(goWords, b - lo, mapEnd - lo);
                if (s == mapEnd && mapEnd < w) {
                    slow = true;
                    s = firstByteOf(a.in, goTable, mapEnd, w);
                }
            }
            uint32_t e;
            if (s >= hi) {
                slow = slow || s < w;
                e = firstByteOf(a.in, stopTable, s, w);
            } else {
                e = lo + firstBit(stopWords, s - lo, mapEnd - lo);
                if (e == mapEnd && mapEnd < w) {
                    slow = true;
                    e = firstByteOf(a.in, stopTable, mapEnd, w);
                }
            }
            a.valStart[i] = (int)s;
            a.valLen[i] = (int)(e - s);
            if (slow) atomicAdd(&slowHere, 1u);
        }
        __syncthreads();                                                /* the bitmaps are rewritten by the next tile */
    }
    __syncthreads();
    if (threadIdx.x == 0 && slowHere != 0) atomicAdd(a.slowPairs, (unsigned long long)slowHere);
}

__global__ void pfac_capture_finish(const unsigned long long *slowPairs, unsigned long long *hostValue) { storeToHost(hostValue, *slowPairs); }

template <bool SINGLE>
void captureLaunches(const PFAC_context *c, const CaptureArgs &a, const HostHandoff &count)
{
    const unsigned int grid = tileGrid(c, a.tiles);
    hipLaunchKernelGGL(pfac_capture_clear, dim3(gridFor(c, a.tiles)), dim3(256), 0, 0, a);
    hipLaunchKernelGGL(pfac_capture_mark, dim3(gridFor(c, a.numPairs)), dim3(256), 0, 0, a);
    hipLaunchKernelGGL(pfac_capture_pairs<SINGLE>, dim3(grid), dim3(kSplitThreads), 0, 0, a);
    hipLaunchKernelGGL(pfac_capture_finish, dim3(1), dim3(1), 0, 0, a.slowPairs, reinterpret_cast<unsigned long long *>(count.d_value));
}

} // namespace

extern "C" {

PFAC_status_t PFACX_captureRun(PFAC_handle_t handle, const PFACX_captureRun_t *run, size_t *h_slowPairs)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!run || !h_slowPairs || !run->d_input || run->size == 0 || run->size > (size_t)0x7fffffff || run->numPairs == 0 ||
        run->numPairs > (size_t)0x7fffffff || !run->d_pos || !run->d_valStart || !run->d_valLen || (run->flags & ~PFACX_CAPTURE_AT_POS))
        return PFAC_STATUS_INVALID_PARAMETER;
    const bool atPos = (run->flags & PFACX_CAPTURE_AT_POS) != 0;
    if (!atPos && (!run->d_ids || !run->d_patternLen || run->numLens > (size_t)0x7fffffff)) return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = handle;
    CaptureArgs a{};
    const unsigned int members = fillCutArgs(a, run->d_input, run->size, 0, run->stop);
    const size_t tiles = a.tiles;
    a.window = run->window;
    a.atPos = atPos ? 1u : 0u;
    a.ids = atPos ? nullptr : run->d_ids;
    a.pos = run->d_pos;
    a.numPairs = (uint32_t)run->numPairs;
    a.patternLen = atPos ? nullptr : run->d_patternLen;
    a.numLens = atPos ? 0u : (uint32_t)run->numLens;
    a.valStart = run->d_valStart;
    a.valLen = run->d_valLen;
    for (unsigned int k = 0; k < 8; k++) a.go[k] = ~run->skip[k];
    const PFAC_status_t carved = carveScratch(c->scratch.capture, [&](ScratchCarver &k) {
        a.tileFirstPair = k.take<uint32_t>(tiles);
        a.slowPairs = k.take<unsigned long long>(1);
    });
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    const HostHandoff count(c, pfac::kHostCapture);                     /* the slow pairs */
    dispatchSingle(members, [&](auto single) { captureLaunches<decltype(single)::value>(c, a, count); });
    unsigned long long slow = 0;
    if (!count.finish(&slow, a.slowPairs)) return PFAC_STATUS_INTERNAL_ERROR;
    if (slow > run->numPairs) return PFAC_STATUS_INTERNAL_ERROR;
    *h_slowPairs = (size_t)slow;
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
