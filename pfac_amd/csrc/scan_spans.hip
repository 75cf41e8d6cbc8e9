/*
 * scan_spans.hip -- covered spans and redaction (include/pfac_ext.h: PFACX_matchSpans* / PFACX_redactSpansFromDevice): the bytes of a
 * buffer that belong to a match, as maximal runs, and the buffer with those bytes overwritten.
 *
 * SELECT works in pair space, behind the compacted scan WITH its ordering launches (the pairs come in position order, one per position: the longest
 * match there, of which every other pattern at the position is a prefix).  Pair i ends at end_i = pos_i + len(id_i); E_i = max(end_j, j < i), E_0 = 0;
 * pair i HEADS a span iff i == 0 or pos_i > E_i (pos_i == E_i touches the run in front of it: one span); the span of a head ends at the E of the next
 * head, the last one at the maximum of all ends.  A BLOCK is 512 pairs, two per thread.
 *
 *   pfac_spans_reduce         the largest end of each block of pairs
 *   pfac_block_scan<max>      the exclusive prefix MAXIMUM of those (what every block carries in from all the blocks in front of it, however far back
 *                             the largest end lies); scan_passes.h: a block of 1024 threads per 8192 values that folds what lies in front of its
 *                             values itself: no block waits on another, no chain of steps for the 4 Mi values of 2^31 pairs
 *   pfac_spans_heads<0>       E_i by a max-scan over the wave (shuffles) and the block, the head flags, the heads of each block
 *   pfac_block_scan<sum>      their exclusive prefix sum: the first span of each block, the number of spans
 *   pfac_spans_heads<1>       the same walk again: head k writes start_k and end_(k-1) = E_i into handle scratch -- not over the pair list: span k may
 *                             land on a pair that another block has not read yet
 *   pfac_spans_emit           (start, len) of the spans over the caller's arrays, the sum of the lengths
 *   pfac_pairs_finish         (scan_passes.h) both counts as one 64-bit value to mapped host memory, then pfac_host_done (scan_passes.h: HostHandoff)
 * Nothing here touches the input: the work is proportional to the pairs.
 * SCRATCH of a select call with P pairs, S = min(P, (size + 1) / 2) (no more spans fit the buffer), B = (P + 511) / 512 blocks:
 * 2 x 4 S (starts and ends) + 4 B + 4 (B + 1) + 4 B + 4 (B + 1) (largest end, heads, and their scans) + 256 bytes, each part rounded up to 256:
 * 8 bytes per pair and 16 per block: 8.04 bytes per pair at most.  No pairs: none.
 *
 * REDACT is cut by OUTPUT tiles of 4 KiB, aligned on the output address: a tile finds the first span that ends behind its first byte and the first that
 * starts behind its last by a 64-ary search of one wave over the list (a probe per lane and round), stages the spans in between in LDS, 1024 at a time --
 * an ascending disjoint list has at most 2049 in a tile, so three trips is all a tile ever makes --, and every thread builds the 16-bit cover mask of
 * its 16 bytes from a binary search in the staged ends, blends and stores them as one aligned 16-byte store.  Source bytes that lie m bytes into an
 * aligned block come out of two aligned loads with v_alignbyte (scan_passes.h: funnel); whatever hangs over an end of either buffer goes byte by byte with
 * bounds.  Every (start, len) is clamped to [0, size] where it is read: a bad list gives wrong text, never an access outside the buffers.  In place,
 * only threads that cover something write.  No scratch.  Plain C++ and vector stores only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_spans.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"

namespace {

constexpr unsigned int kSpanThreads = 256;
constexpr unsigned int kSpanPer = 2;                                   /* consecutive pairs per thread */
constexpr unsigned int kSpanBlock = kSpanThreads * kSpanPer;           /* 512 pairs per block */
constexpr unsigned int kStage = 1024;                                  /* spans a tile stages at a time */
constexpr unsigned int kStageTrips = 3;                                /* kStage * kStageTrips >= kOutTile / 2 + 1 */
static_assert(kStage * kStageTrips >= kOutTile / 2 + 1, "a tile must be able to stage every span of an ascending disjoint list that meets it");

struct SpanArgs : PairArgs {           /* scan_passes.h: the scan's ordered pairs, pairOf */
    unsigned int blocks;
    unsigned int bound;                 /* entries of outStart / outEnd */
    unsigned int *blockMax, *blockTop;  /* [blocks] largest end of the block; [blocks + 1] largest end in front of the block, [blocks] = of all */
    unsigned int *headCount, *headBase; /* the same for the heads: [blocks] = the number of spans */
    unsigned int *outStart, *outEnd;    /* [bound] */
    unsigned int *covered;              /* one word: the sum of the lengths (zeroed by the first block scan) */
    unsigned long long *value;          /* numSpans | coveredBytes << 32 */
    int *spanStart, *spanLen;
};

__global__ __launch_bounds__(kSpanThreads) void pfac_spans_reduce(SpanArgs a)
{
    __shared__ unsigned int waveTop[kSpanThreads / 64];
    const unsigned int i0 = blockIdx.x * kSpanBlock + threadIdx.x * kSpanPer;
    unsigned int own = 0;
#pragma unroll
    for (unsigned int k = 0; k < kSpanPer; k++) {
        if (i0 + k < a.count) {
            unsigned int p, e;
            pairOf(a, i0 + k, p, e);
            own = OpMax()(own, e);
        }
    }
    unsigned int top = 0;
    (void)blockExclusive<kSpanThreads>(own, waveTop, top, OpMax());
    if (threadIdx.x == 0) a.blockMax[blockIdx.x] = top;
}

/* WRITE == 0: the heads of each block; WRITE == 1: start of span k, end of span k - 1 */
template <int WRITE>
__global__ __launch_bounds__(kSpanThreads) void pfac_spans_heads(SpanArgs a)
{
    __shared__ unsigned int waveTop[kSpanThreads / 64];
    __shared__ unsigned int waveSum[kSpanThreads / 64];
    const unsigned int i0 = blockIdx.x * kSpanBlock + threadIdx.x * kSpanPer;
    unsigned int p[kSpanPer], e[kSpanPer], own = 0;
#pragma unroll
    for (unsigned int k = 0; k < kSpanPer; k++) {
        p[k] = 0;
        e[k] = 0;
        if (i0 + k < a.count) pairOf(a, i0 + k, p[k], e[k]);
        own = OpMax()(own, e[k]);
    }
    unsigned int top = 0;
    const unsigned int carried = OpMax()(a.blockTop[blockIdx.x], blockExclusive<kSpanThreads>(own, waveTop, top, OpMax()));      /* E of the thread's first pair */
    unsigned int run = carried, heads = 0;
#pragma unroll
    for (unsigned int k = 0; k < kSpanPer; k++) {
        if (i0 + k < a.count && (i0 + k == 0 || p[k] > run)) heads |= 1u << k;
        run = OpMax()(run, e[k]);
    }
    const unsigned int nh = (unsigned int)__popc(heads);
    unsigned int total = 0;
    const unsigned int rank = blockExclusive<kSpanThreads>(nh, waveSum, total);
    if constexpr (WRITE == 0) {
        if (threadIdx.x == 0) a.headCount[blockIdx.x] = total;
    } else {
        unsigned int o = a.headBase[blockIdx.x] + rank;
        run = carried;
#pragma unroll
        for (unsigned int k = 0; k < kSpanPer; k++) {
            if ((heads >> k) & 1u) {
                if (o < a.bound) a.outStart[o] = p[k];
                if (o > 0 && o - 1 < a.bound) a.outEnd[o - 1] = run;
                o++;
            }
            run = OpMax()(run, e[k]);
        }
    }
}

__global__ __launch_bounds__(kSpanThreads) void pfac_spans_emit(SpanArgs a)
{
    __shared__ unsigned int waveSum[kSpanThreads / 64];
    const unsigned int all = a.headBase[a.blocks], spans = all < a.bound ? all : a.bound;
    const unsigned int last = a.blockTop[a.blocks];
    unsigned int own = 0;
    for (unsigned int k = blockIdx.x * kSpanThreads + threadIdx.x; k < spans; k += gridDim.x * kSpanThreads) {
        const unsigned int s = a.outStart[k], e = k + 1 == spans ? last : a.outEnd[k];
        const unsigned int len = e > s ? e - s : 0u;
        a.spanStart[k] = (int)s;
        a.spanLen[k] = (int)len;
        own += len;
    }
    unsigned int total = 0;
    (void)blockExclusive<kSpanThreads>(own, waveSum, total);
    if (threadIdx.x == 0 && total != 0) atomicAdd(a.covered, total);
}

/* ------------------------------------------------------------------ the redaction */

struct RedactArgs {
    const unsigned char *in;
    unsigned char *out;
    unsigned int n;
    const int *start, *len;             /* the caller's spans: clamped, never trusted */
    unsigned int count;
    uint32_t fill4;                     /* the fill byte four times */
    unsigned int misOut;                /* address of out & 15 */
    unsigned int inPlace;
};

/* span i as bytes [s, e) (a caller that wants only s never loads the length) */
__device__ __forceinline__ void spanOf(const RedactArgs &a, unsigned int i, unsigned int &s, unsigned int &e) { clampSpan(a.start[i], a.len[i], a.n, s, e); }

/* in[o, o + 16), o + 16 <= n (scan_passes.h: loadBytes16) */
__device__ __forceinline__ pfacmod::u32x4 load16(const RedactArgs &a, unsigned int o) { return loadBytes16(a.in, a.n, o); }

/* a nibble of the cover mask as the byte mask of a dword: bit i lands on bit 8 i and nothing carries */
__device__ __forceinline__ uint32_t byteMask(uint32_t nibble) { return ((nibble * 0x00204081u) & 0x01010101u) * 0xFFu; }

/* tiles are cut in v = o + misOut, the output offset counted from the aligned 16-byte block that holds out[0] */
__global__ __launch_bounds__(kSpanThreads) void pfac_spans_redact(RedactArgs a)
{
    __shared__ unsigned int sStart[kStage], sEnd[kStage];
    __shared__ unsigned int sFirst, sCount;
    const unsigned int t = threadIdx.x;
    const size_t vEnd = (size_t)a.n + a.misOut;
    for (size_t vLo = (size_t)blockIdx.x * kOutTile; vLo < vEnd; vLo += (size_t)gridDim.x * kOutTile) {
        const TileFrame<unsigned int> f = tileFrame(vLo, a.misOut, a.n);
        const unsigned int oLo = f.oLo, oHi = f.oHi;
        if (t < 64u) {
            /* the first span that ends behind oLo, and the first behind it that starts at or behind oHi */
            const unsigned int first = waveLowerBound(0u, a.count, [&](unsigned int i) { unsigned int s, e; spanOf(a, i, s, e); return e > oLo; });
            const unsigned int limit = a.count - first < kStage * kStageTrips ? a.count : first + kStage * kStageTrips;
            const unsigned int behind = waveLowerBound(first, limit, [&](unsigned int i) { unsigned int s, e; spanOf(a, i, s, e); return s >= oHi; });
            if (t == 0) { sFirst = first; sCount = behind - first; }
        }
        __syncthreads();
        const unsigned int first = sFirst, total = sCount;
        const unsigned int cLo = f.cLo, cHi = f.cLo + f.nb;
        const bool active = f.nb != 0;
        uint32_t mask = 0;                                        /* bit j: byte cLo + j is covered */
        for (unsigned int base = 0; base < total; base += kStage) {
            const unsigned int cnt = total - base < kStage ? total - base : kStage;
            if (base != 0) __syncthreads();                       /* the stage is rewritten */
            for (unsigned int j = t; j < cnt; j += kSpanThreads) {
                spanOf(a, first + base + j, sStart[j], sEnd[j]);
            }
            __syncthreads();
            if (active) {
                unsigned int lo = 0, hi = cnt;                    /* the first staged span that ends behind cLo */
                while (lo < hi) {
                    const unsigned int mid = (lo + hi) / 2;
                    if (sEnd[mid] > cLo) hi = mid; else lo = mid + 1;
                }
                for (unsigned int j = lo; j < cnt && sStart[j] < cHi; j++) {
                    const unsigned int s = sStart[j] > cLo ? sStart[j] - cLo : 0u;
                    const unsigned int e = (sEnd[j] < cHi ? sEnd[j] : cHi) - cLo;
                    if (sEnd[j] > cLo && e > s) mask |= ((1u << e) - 1u) & ~((1u << s) - 1u);
                }
            }
        }
        if (active && (!a.inPlace || mask != 0)) {                /* in place, only threads that cover something write */
            const pfacmod::u32x4 fill = {a.fill4, a.fill4, a.fill4, a.fill4};
            pfacmod::u32x4 x = fill;
            if (mask != 0xFFFFu) {                                /* the bytes as they are, blended with the fill */
                pfacmod::u32x4 src;
                if (f.whole) {
                    src = a.inPlace ? *reinterpret_cast<const pfacmod::u32x4 *>(a.out + cLo) : load16(a, cLo);
                } else {
                    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
                    for (unsigned int b = 0; b < 16; b++)
                        if (b < f.nb) w[b >> 2] |= (uint32_t)a.in[cLo + b] << (8 * (b & 3));
                    src = pfacmod::u32x4{w[0], w[1], w[2], w[3]};
                }
                const pfacmod::u32x4 m = {byteMask(mask & 15u), byteMask((mask >> 4) & 15u), byteMask((mask >> 8) & 15u), byteMask(mask >> 12)};
                x = (src & ~m) | (fill & m);
            }
            tileStore(a.out, f, x);
        }
        __syncthreads();                                          /* sFirst and the stage are rewritten by the next tile */
    }
}

} // namespace

extern "C" {

PFAC_status_t PFACX_spansSelect(PFAC_handle_t handle, char *d_scan, size_t size, int hashed, const int *d_patternLen, size_t numIds, int *d_spanStart,
                                int *d_spanLen, size_t *h_numSpans, size_t *h_coveredBytes)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!d_scan || !d_patternLen || !d_spanStart || !d_spanLen || !h_numSpans || !h_coveredBytes || size == 0 || size > (size_t)0x7fffffff)
        return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = handle;

    /* the ordered pairs: ids in d_spanStart, positions in d_spanLen */
    SpanArgs a{};
    const PFAC_status_t st = pairsSelectHead(handle, d_scan, size, hashed, d_patternLen, numIds, d_spanStart, d_spanLen, h_numSpans, h_coveredBytes, a);
    if (st != PFAC_STATUS_SUCCESS || a.count == 0) return st;
    const size_t count = a.count;
    const size_t blocks = (count + kSpanBlock - 1) / kSpanBlock;
    const size_t bound = count < (size + 1) / 2 ? count : (size + 1) / 2;
    a.blocks = (unsigned int)blocks;
    a.bound = (unsigned int)bound;
    const PFAC_status_t carved = carveScratch(c->scratch.spans, [&](ScratchCarver &k) {
        a.outStart = k.take<unsigned int>(bound);
        a.outEnd = k.take<unsigned int>(bound);
        a.blockMax = k.take<unsigned int>(blocks);
        a.blockTop = k.take<unsigned int>(blocks + 1);
        a.headCount = k.take<unsigned int>(blocks);
        a.headBase = k.take<unsigned int>(blocks + 1);
        a.value = k.take<unsigned long long>(1, 8);            /* and, behind it, the word `covered` */
    });
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    a.covered = reinterpret_cast<unsigned int *>(a.value + 1);
    a.spanStart = d_spanStart;
    a.spanLen = d_spanLen;

    hipLaunchKernelGGL(pfac_spans_reduce, dim3(a.blocks), dim3(kSpanThreads), 0, 0, a);
    blockScan<OpMax>({{a.blockMax}, {a.blockTop}}, a.blocks, nullptr, a.covered);
    hipLaunchKernelGGL(pfac_spans_heads<0>, dim3(a.blocks), dim3(kSpanThreads), 0, 0, a);
    blockScan<OpSum>({{a.headCount}, {a.headBase}}, a.blocks, nullptr, nullptr);
    hipLaunchKernelGGL(pfac_spans_heads<1>, dim3(a.blocks), dim3(kSpanThreads), 0, 0, a);
    hipLaunchKernelGGL(pfac_spans_emit, dim3(gridFor(c, bound)), dim3(kSpanThreads), 0, 0, a);
    return pairsSelectTail(c, pfac::kHostSpans, a.headBase + a.blocks, bound, size, a.value, h_numSpans, h_coveredBytes);
}

PFAC_status_t PFACX_spansRedact(PFAC_handle_t handle, const char *d_input, size_t size, const int *d_spanStart, const int *d_spanLen, size_t numSpans,
                                unsigned char fill, char *d_out)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!d_input || !d_out || size == 0 || size > (size_t)0x7fffffff || numSpans > (size_t)0x7fffffff || (numSpans && (!d_spanStart || !d_spanLen)))
        return PFAC_STATUS_INVALID_PARAMETER;
    const PFAC_context *c = handle;
    RedactArgs a{};
    a.in = reinterpret_cast<const unsigned char *>(d_input);
    a.out = reinterpret_cast<unsigned char *>(d_out);
    a.n = (unsigned int)size;
    a.start = d_spanStart;
    a.len = d_spanLen;
    a.count = (unsigned int)numSpans;
    a.fill4 = fill * 0x01010101u;
    a.misOut = (unsigned int)(reinterpret_cast<uintptr_t>(d_out) & 15u);
    a.inPlace = d_input == d_out ? 1u : 0u;
    if (a.inPlace && numSpans == 0) return PFAC_STATUS_SUCCESS;
    const size_t tiles = (size + a.misOut + kOutTile - 1) / kOutTile, cap = (size_t)gridCap(c, 8) * 4;
    hipLaunchKernelGGL(pfac_spans_redact, dim3((unsigned int)(tiles < cap ? tiles : cap)), dim3(kSpanThreads), 0, 0, a);
    return hipGetLastError() == hipSuccess ? PFAC_STATUS_SUCCESS : PFAC_STATUS_INTERNAL_ERROR;
}

} /* extern "C" */
