/*
 * scan_cover.hip -- covered spans of an unsorted interval list (include/pfac_ext.h: PFACX_coverSpans*): the maximal runs of the
 * positions of [0, size) that some interval of a caller's list holds, ascending, as PFACX_redactSpansFromDevice takes them.
 *
 * The list has no order, so the running maximum of scan_spans.hip does not apply.  The call works on a HIERARCHY OF BITMAPS with fan-out 32 in
 * handle scratch: level 0 has a bit per position; bit j of level k + 1 says "word j of level k is all ones"; the levels go on until one is a
 * single word -- at most 7 for size < 2^31 (2^26, 2^21, 2^16, 2^11, 64, 2, 1 words).
 *
 *   hipMemsetAsync            the levels and the word `covered`, one range
 *   pfac_cover_mark           a thread per interval, grid-stride: the interval clamped to [0, size]; at each level an atomicOr for the partial
 *                             head word, one for the partial tail word, and the whole words in between go up as an interval of bits of the next
 *                             level (an interval inside one word: one atomicOr, and it ends there).  The top level is one word, so the walk ends:
 *                             at most two atomics a level, 14 an interval, however long it is -- [0, size) a million times costs what a million
 *                             one-byte intervals cost.  There is no loop over the words of an interval anywhere in this unit
 *   pfac_cover_push           top down, one launch per level below the top: a word whose bit is set in the level above becomes all ones.
 *                             A thread takes four words of the child (one 16-byte store where all four are whole); it reads 1 / 32 of what it
 *                             covers and writes only whole words.  Behind the last launch level 0 IS the covered set
 *   pfac_cover_extract<0>     a block per 1024 words of level 0 (kCoverBlockBits = 32 Ki positions), a 16-byte load a thread: the span starts
 *                             w & ~(w << 1 | carry), carry = the top bit of the word in front (0 for word 0), counted per block; the popcount of
 *                             the words added to `covered`
 *   pfac_block_scan<sum>      (scan_passes.h) the first span of each block, the number of spans
 *   pfac_cover_extract<1>     the same walk: start k goes to spanStart[k], stop k -- w & ~(w >> 1 | low bit of the word behind << 31), plus one --
 *                             to spanLen[k], both only below `capacity`.  Starts and stops alternate, so a thread's first stop has the rank of
 *                             its first start, less one where a span runs into the thread (carry and the thread's first bit): no second scan
 *   pfac_cover_lengths        spanLen[k] -= spanStart[k] below min(spans, capacity)
 *   pfac_pairs_finish         (scan_passes.h) both counts as one 64-bit value to mapped host memory, then pfac_host_done (HostHandoff)
 * The write pass and the lengths are not launched for the count query.
 *
 * Why push down and not test the ancestors in the extract pass: the extract pass runs twice and would load up to six ancestor words per thread
 * each time; the push reads each level once, 1 / 32 of the level below, and leaves the extract passes a plain stream over one array.
 *
 * BOUNDS.  MARK clamps before anything else, so no bit at or above `size` is ever set: the word that holds bit size - 1 is only ever ORed with a
 * head, a tail or an inner mask, and it is whole only where size is a multiple of 32.  An interval of level k + 1 ends at e >> 5 <= the words of
 * level k, so every atomic lands inside its level.  Every level is a region of its own, rounded up to 256 bytes and zeroed: the quads of
 * pfac_cover_push and the 16-byte loads of the extract passes stay inside the region, and what lies behind a level's last word is zero.  The word
 * behind a thread's four is read only below the words of level 0.  Every span store is checked against `capacity`.
 * SCRATCH of a call with W_0 = (size + 31) / 32, W_(k+1) = (W_k + 31) / 32 down to one word, B = (W_0 + 1023) / 1024 blocks:
 * 4 W_0 + 4 W_1 + ... (about size / 8 x 32 / 31 bytes) + 4 B + 4 (B + 1) + 16, each part rounded up to 256; sized by `size` alone.
 * No LDS beyond the block prefixes, no scratch memory, plain C++, vector stores and ordinary atomics only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_cover.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "pfac_ext.h"
#include "scan_passes.h"

namespace {

constexpr unsigned int kCoverThreads = 256;
constexpr unsigned int kCoverPer = 4;                                        /* words of level 0 per thread: one 16-byte load */
constexpr unsigned int kCoverBlockWords = kCoverThreads * kCoverPer;         /* 1024 words per block */
constexpr unsigned int kCoverBlockBits = kCoverBlockWords * 32;              /* 32 Ki positions per block */
constexpr unsigned int kCoverLevels = 7;                                     /* 32^7 > 2^31 */
static_assert(kCoverBlockBits == PFACX_COVER_BLOCK_BYTES, "pfac_module.h tells the tests where the extract blocks end");

struct CoverArgs {
    const int *start, *second;          /* the caller's intervals: clamped, never trusted, never written */
    unsigned int count, n;
    unsigned int lengths;               /* PFACX_COVER_LENGTHS: `second` holds lengths */
    unsigned int levels;
    unsigned int *level[kCoverLevels];  /* level k: words[k] words, its region rounded up to 256 bytes */
    unsigned int words[kCoverLevels];
    unsigned int blocks;
    unsigned int *blockCount, *blockBase;   /* [blocks] the span starts of each block; [blocks + 1] their exclusive prefix, [blocks] = the spans */
    unsigned int *covered;              /* one word: the covered positions (zeroed with the levels) */
    unsigned long long *value;          /* numSpans | coveredBytes << 32 */
    int *spanStart, *spanLen;
    unsigned int capacity;
};

__global__ __launch_bounds__(kCoverThreads) void pfac_cover_mark(CoverArgs a)
{
    for (unsigned int i = blockIdx.x * kCoverThreads + threadIdx.x; i < a.count; i += gridDim.x * kCoverThreads) {
        const long long s0 = a.start[i];
        const long long e0 = a.lengths ? s0 + (long long)a.second[i] : (long long)a.second[i];
        if (e0 <= 0 || s0 >= (long long)a.n || e0 <= s0) continue;
        unsigned int s = s0 < 0 ? 0u : (unsigned int)s0;
        unsigned int e = e0 > (long long)a.n ? a.n : (unsigned int)e0;     /* 0 <= s < e <= n: bits of level 0 */
        for (unsigned int k = 0; k < a.levels && s < e; k++) {
            unsigned int *w = a.level[k];
            const unsigned int ws = s >> 5, we = (e - 1u) >> 5, hs = s & 31u, te = e & 31u;
            if (ws == we) {                                                /* inside one word (the top level always is) */
                const unsigned int upTo = te ? (1u << te) - 1u : 0xFFFFFFFFu;
                atomicOr(&w[ws], upTo & (0xFFFFFFFFu << hs));
                break;
            }
            if (hs) atomicOr(&w[ws], 0xFFFFFFFFu << hs);
            if (te) atomicOr(&w[e >> 5], (1u << te) - 1u);
            s = hs ? ws + 1u : ws;                                         /* the whole words in between: bits of the next level */
            e = e >> 5;
        }
    }
}

/* child word j becomes all ones where bit j of the parent level is set; a thread per four words of the child */
__global__ __launch_bounds__(kCoverThreads) void pfac_cover_push(const unsigned int *parent, unsigned int *child, unsigned int quads)
{
    for (unsigned int q = blockIdx.x * kCoverThreads + threadIdx.x; q < quads; q += gridDim.x * kCoverThreads) {
        const unsigned int nibble = (parent[q >> 3] >> ((q & 7u) * 4u)) & 15u;
        if (nibble == 0) continue;
        if (nibble == 15u) {
            reinterpret_cast<pfacmod::u32x4 *>(child)[q] = pfacmod::u32x4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        } else {
#pragma unroll
            for (unsigned int j = 0; j < 4; j++)
                if ((nibble >> j) & 1u) child[q * 4u + j] = 0xFFFFFFFFu;
        }
    }
}

/* WRITE == 0: the span starts of each block, the covered positions; WRITE == 1: start k to spanStart[k], stop k to spanLen[k] */
template <int WRITE>
__global__ __launch_bounds__(kCoverThreads) void pfac_cover_extract(CoverArgs a)
{
    __shared__ unsigned int waveSum[kCoverThreads / 64];
    const unsigned int W = a.words[0];
    const unsigned int *bits = a.level[0];
    const unsigned int w0 = blockIdx.x * kCoverBlockWords + threadIdx.x * kCoverPer;          /* the thread's first word */
    unsigned int w[kCoverPer] = {0, 0, 0, 0};
    unsigned int carry = 0;
    if (w0 < W) {                                                          /* the region is whole quads, zero behind word W - 1 */
        const pfacmod::u32x4 v = reinterpret_cast<const pfacmod::u32x4 *>(bits)[w0 >> 2];
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        if (w0 != 0) carry = bits[w0 - 1u] >> 31;
    }
    unsigned int starts[kCoverPer], own = 0, pop = 0, c = carry;
#pragma unroll
    for (unsigned int j = 0; j < kCoverPer; j++) {
        starts[j] = w[j] & ~((w[j] << 1) | c);
        c = w[j] >> 31;
        own += (unsigned int)__popc(starts[j]);
        pop += (unsigned int)__popc(w[j]);
    }
    unsigned int total = 0;
    const unsigned int rank = blockExclusive<kCoverThreads>(own, waveSum, total);
    if constexpr (WRITE == 0) {
        if (threadIdx.x == 0) a.blockCount[blockIdx.x] = total;
        unsigned int popTotal = 0;
        (void)blockExclusive<kCoverThreads>(pop, waveSum, popTotal);
        if (threadIdx.x == 0 && popTotal != 0) atomicAdd(a.covered, popTotal);
    } else {
        if (own == 0 && pop == 0) return;                                  /* (behind the block's last barrier) */
        const unsigned int first = a.blockBase[blockIdx.x] + rank;         /* of this thread's starts */
        const unsigned int open = carry & w[0] & 1u;                       /* a span runs into the thread: its stop, the thread's first, belongs to start first - 1 */
        if (first - open >= a.capacity) return;                            /* nothing of this thread fits */
        unsigned int o = first;
#pragma unroll
        for (unsigned int j = 0; j < kCoverPer; j++) {
            unsigned int m = starts[j];
            while (m != 0) {
                const unsigned int b = (unsigned int)__ffs((int)m) - 1u;
                m &= m - 1u;
                if (o < a.capacity) a.spanStart[o] = (int)((w0 + j) * 32u + b);
                o++;
            }
        }
        /* the low bit of the word behind each of the four: 0 behind the last word of level 0 */
        const unsigned int next[kCoverPer] = {w[1] & 1u, w[2] & 1u, w[3] & 1u, w0 + kCoverPer < W ? bits[w0 + kCoverPer] & 1u : 0u};
        o = first - open;
#pragma unroll
        for (unsigned int j = 0; j < kCoverPer; j++) {
            unsigned int m = w[j] & ~((w[j] >> 1) | (next[j] << 31));
            while (m != 0) {
                const unsigned int b = (unsigned int)__ffs((int)m) - 1u;
                m &= m - 1u;
                if (o < a.capacity) a.spanLen[o] = (int)((w0 + j) * 32u + b + 1u);
                o++;
            }
        }
    }
}

__global__ __launch_bounds__(kCoverThreads) void pfac_cover_lengths(CoverArgs a)
{
    const unsigned int all = a.blockBase[a.blocks], spans = all < a.capacity ? all : a.capacity;
    for (unsigned int k = blockIdx.x * kCoverThreads + threadIdx.x; k < spans; k += gridDim.x * kCoverThreads) a.spanLen[k] -= a.spanStart[k];
}

} // namespace

extern "C" {

PFAC_status_t PFACX_coverRun(PFAC_handle_t handle, const PFACX_coverRun_t *run, size_t *h_numSpans, size_t *h_coveredBytes)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!run || !h_numSpans || !h_coveredBytes || !run->d_start || !run->d_end || run->size == 0 || run->size > (size_t)0x7fffffff ||
        run->numIntervals == 0 || run->numIntervals > (size_t)0x7fffffff || (run->flags & ~PFACX_COVER_LENGTHS) ||
        (run->capacity && (!run->d_spanStart || !run->d_spanLen)))
        return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = handle;

    CoverArgs a{};
    a.start = run->d_start;
    a.second = run->d_end;
    a.count = (unsigned int)run->numIntervals;
    a.n = (unsigned int)run->size;
    a.lengths = (run->flags & PFACX_COVER_LENGTHS) ? 1u : 0u;
    const size_t most = (run->size + 1) / 2;                               /* no more spans fit [0, size) */
    a.capacity = (unsigned int)(run->capacity < most ? run->capacity : most);
    a.spanStart = run->d_spanStart;
    a.spanLen = run->d_spanLen;
    unsigned int units = a.n;
    do {
        units = (units + 31u) / 32u;
        a.words[a.levels++] = units;
    } while (units > 1u && a.levels < kCoverLevels);
    if (units != 1u) return PFAC_STATUS_INTERNAL_ERROR;
    a.blocks = (a.words[0] + kCoverBlockWords - 1u) / kCoverBlockWords;

    size_t zeroed = 0;                                                     /* the levels, the value and the word `covered`: the head of the scratch */
    const PFAC_status_t carved = carveScratch(c->scratch.cover, [&](ScratchCarver &k) {
        for (unsigned int l = 0; l < a.levels; l++) a.level[l] = k.take<unsigned int>(a.words[l]);
        a.value = k.take<unsigned long long>(1, 8);                        /* and, behind it, the word `covered` */
        zeroed = k.bytes;
        a.blockCount = k.take<unsigned int>(a.blocks);
        a.blockBase = k.take<unsigned int>((size_t)a.blocks + 1);
    });
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    a.covered = reinterpret_cast<unsigned int *>(a.value + 1);

    if (hipMemsetAsync(a.level[0], 0, zeroed, nullptr) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
    hipLaunchKernelGGL(pfac_cover_mark, dim3(gridFor(c, a.count)), dim3(kCoverThreads), 0, 0, a);
    for (unsigned int l = a.levels - 1u; l > 0; l--) {
        const unsigned int quads = (a.words[l - 1u] + 3u) / 4u;
        hipLaunchKernelGGL(pfac_cover_push, dim3(gridFor(c, quads)), dim3(kCoverThreads), 0, 0, a.level[l], a.level[l - 1u], quads);
    }
    hipLaunchKernelGGL(pfac_cover_extract<0>, dim3(a.blocks), dim3(kCoverThreads), 0, 0, a);
    blockScan<OpSum>({{a.blockCount}, {a.blockBase}}, a.blocks, nullptr, nullptr);
    if (a.capacity) {
        hipLaunchKernelGGL(pfac_cover_extract<1>, dim3(a.blocks), dim3(kCoverThreads), 0, 0, a);
        hipLaunchKernelGGL(pfac_cover_lengths, dim3(gridFor(c, a.capacity)), dim3(kCoverThreads), 0, 0, a);
    }
    const HostHandoff counts(c, pfac::kHostCover);
    hipLaunchKernelGGL(pfac_pairs_finish<unsigned int>, dim3(1), dim3(1), 0, 0, a.blockBase + a.blocks, 0xFFFFFFFFu, a.covered, a.value,
                       reinterpret_cast<unsigned long long *>(counts.d_value));
    unsigned long long v = 0;
    if (!counts.finish(&v, a.value)) return PFAC_STATUS_INTERNAL_ERROR;
    const size_t spans = (size_t)(v & 0xFFFFFFFFull), covered = (size_t)(v >> 32);
    if (spans > most || covered < spans || covered > run->size) return PFAC_STATUS_INTERNAL_ERROR;
    *h_numSpans = spans;
    *h_coveredBytes = covered;
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
