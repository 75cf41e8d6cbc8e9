/*
 * scan_disjoint.hip -- disjoint leftmost-longest matches and their replacement (include/pfac_ext.h: PFACX_matchDisjoint* / PFACX_replace*):
 * the input tokenised into matches that do not overlap, and the text with every token substituted by the string of its pattern.
 *
 * SELECT works in pair space, behind the compacted scan WITH its ordering launches (P pairs in position order, one per position: the longest match
 * there).  Pair i ends at end_i = pos_i + len(id_i); next(i) = the first j > i with pos_j >= end_i, P if there is none; the disjoint list is the orbit
 * of pair 0 under next.  Positions are distinct and ascending, so pos_(i + k) >= pos_i + k and next(i) <= i + len(id_i): a binary search over len(id_i)
 * pairs finds it.  A BLOCK is 512 pairs, one per thread.
 *
 *   pfac_disjoint_exit        next(i) by that search (in LDS inside the block, in global memory behind it), then nine rounds of pointer jumping in LDS:
 *                             J[i] = exit(i), the first pair OUTSIDE the block on the chain from i (<= P); mark[i] = (i == 0)
 *   pfac_disjoint_double      ceil(log2(B)) launches over all pairs, B = the blocks: mark[J[i]] = 1 for every marked i, J'[i] = J[J[i]] (J double
 *                             buffered; the marks in place, plain stores of 1 -- a mark set in the same round is an element of the orbit too, reading
 *                             it early only marks more of the orbit).  Every hop leaves its block, so the orbit of pair 0 under exit has at most B
 *                             elements: after the rounds the marks are exactly the pair through which the chain enters each block it visits
 *   pfac_disjoint_mark        the block finds its entry (if any), rebuilds next in LDS and marks the chain from the entry inside the block by the same
 *                             doubling in LDS; mark[i] = pair i is taken; the tokens of each block
 *   pfac_block_scan<sum>      their exclusive prefix sum (scan_passes.h): the first token of each block, the number of tokens
 *   pfac_disjoint_stage       token k = (id, pos) into handle scratch -- not over the pair list: token k may land on a pair that another block has
 *                             not read yet (the two arrays of J are free by now and take the staged tokens)
 *   pfac_disjoint_emit        the tokens over the caller's arrays, the sum of their lengths
 *   pfac_pairs_finish         (scan_passes.h) both counts as one 64-bit value to mapped host memory, then pfac_host_done (scan_passes.h: HostHandoff)
 * No block waits on another, nothing walks the blocks one after another, and nothing relies on chains merging: ab / ba over abab... has two chains
 * that never meet, and only the one through pair 0 is ever marked.  Nothing here touches the input.
 * SCRATCH of a select call with P pairs, B = (P + 511) / 512 blocks: 2 x 4 P (J, then the staged tokens) + P (marks) + 4 B + 4 (B + 1) (tokens of
 * the blocks and their scan) + 256 bytes, each part rounded up to 256: 9.02 bytes per pair at most.  No pairs: none.
 *
 * REPLACE.  Token k removes [s_k, s_k + len_k) of the input and inserts its replacement of r_k bytes; its bytes of the output start at
 * outStart_k = s_k + the sum of (r_j - len_j) over j < k, and the gap behind it -- input bytes from s_k + len_k on -- follows them up to outStart_(k + 1).
 *   pfac_replace_delta        the 64-bit sums of r - len over blocks of tokens
 *   pfac_array_scan<u64>      their exclusive prefix (scan_passes.h); the sum of all to the host: the size of the text is size + that
 *   pfac_replace_offsets      outStart_k, 64-bit
 *   pfac_replace_copy         cut by OUTPUT tiles of 4 KiB aligned on the output address, like the redaction: wave 0 finds the tokens that own a byte of
 *                             the tile by two 64-ary searches over outStart, the block stages them in LDS 1024 at a time, and every thread builds
 *                             its 16 output bytes: where they lie in one gap out of two aligned input loads and a funnel (loadBytes16) -- the case
 *                             that carries the traffic --, else byte by byte, every read checked against the end of its buffer; one aligned 16-byte
 *                             store, bytes where the 16 hang over an end of the text
 * Every (id, start) and every offset is clamped where it is read (tokenOf): a bad list gives unspecified text, never an access outside the buffers.
 * Tokens that own no output byte (deleted matches that touch each other) are staged and skipped: a tile pays for the ones that fall into it.
 * SCRATCH of a replace call with T tokens: 8 T (outStart) + 8 (blocks + 1), each rounded up to 256; the same allocation as the select's.
 * Plain C++ and vector stores only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_disjoint.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"

namespace {

constexpr unsigned int kDisjointBlock = 512;                           /* pairs per block, one per thread */
constexpr unsigned int kDisjointRounds = 9;                            /* a chain inside a block has at most 2^9 pairs */
static_assert((1u << kDisjointRounds) == kDisjointBlock, "the pointer jumping in LDS must cover a whole block");
constexpr unsigned int kPassThreads = 256;
constexpr unsigned int kReplaceStage = 1024;                           /* tokens a tile stages at a time */

struct DisjointArgs : PairArgs {       /* scan_passes.h: the scan's ordered pairs, pairOf */
    unsigned int blocks;
    unsigned int *jump[2];              /* [count] each: J and J'; behind pfac_disjoint_mark the staged ids and positions */
    unsigned char *mark;                /* [count] */
    unsigned int *tokCount, *tokBase;   /* [blocks] tokens of the block; [blocks + 1] tokens in front of the block, [blocks] = all */
    unsigned int *covered;              /* one word: the sum of the lengths (zeroed by the block scan) */
    unsigned long long *value;          /* numTokens | coveredBytes << 32 */
    int *outIds, *outPos;
};

/* next(i) of the thread's pair i = blockIdx.x * kDisjointBlock + threadIdx.x (count for a thread without a pair), inside (i, count] whatever the pairs
 * say; sPos: the positions of the block's pairs (every thread of the block calls this; synchronised on return) */
__device__ __forceinline__ unsigned int blockNext(const DisjointArgs &a, unsigned int *sPos)
{
    const unsigned int base = blockIdx.x * kDisjointBlock, i = base + threadIdx.x;
    const unsigned int blockEnd = a.count - base < kDisjointBlock ? a.count : base + kDisjointBlock;
    unsigned int p = 0, e = 0;
    if (i < a.count) pairOf(a, i, p, e);
    sPos[threadIdx.x] = p;
    __syncthreads();
    if (i >= a.count) return a.count;
    const unsigned int len = e > p ? e - p : 1u;
    unsigned int lo = i + 1, hi = a.count - i > len ? i + len : a.count;                 /* pos_(i + len) >= end_i: the answer lies in [lo, hi] */
    while (lo < hi) {
        const unsigned int mid = lo + (hi - lo) / 2;                                       /* < hi <= count */
        unsigned int pm;
        if (mid < blockEnd) {
            pm = sPos[mid - base];
        } else {
            const int raw = a.pos[mid];
            pm = raw < 0 ? 0u : ((unsigned int)raw > a.n ? a.n : (unsigned int)raw);
        }
        if (pm >= e) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(kDisjointBlock) void pfac_disjoint_exit(DisjointArgs a)
{
    __shared__ unsigned int sPos[kDisjointBlock], sJ[kDisjointBlock];
    const unsigned int base = blockIdx.x * kDisjointBlock, t = threadIdx.x, i = base + t;
    const unsigned int blockEnd = a.count - base < kDisjointBlock ? a.count : base + kDisjointBlock;
    unsigned int j = blockNext(a, sPos);
    sJ[t] = j;
    __syncthreads();
    for (unsigned int r = 0; r < kDisjointRounds; r++) {
        const unsigned int hop = j < blockEnd ? sJ[j - base] : j;
        __syncthreads();
        sJ[t] = hop;
        j = hop;
        __syncthreads();
    }
    if (i < a.count) {
        a.jump[0][i] = j;
        a.mark[i] = i == 0 ? 1 : 0;
    }
}

__global__ __launch_bounds__(kPassThreads) void pfac_disjoint_double(DisjointArgs a, unsigned int from)
{
    const unsigned int *in = a.jump[from];
    unsigned int *out = a.jump[from ^ 1u];
    for (unsigned int i = blockIdx.x * kPassThreads + threadIdx.x; i < a.count; i += gridDim.x * kPassThreads) {
        const unsigned int j = in[i];
        if (j < a.count) {
            if (a.mark[i]) a.mark[j] = 1;
            out[i] = in[j];
        } else {
            out[i] = a.count;
        }
    }
}

__global__ __launch_bounds__(kDisjointBlock) void pfac_disjoint_mark(DisjointArgs a)
{
    __shared__ unsigned int sPos[kDisjointBlock], sJ[kDisjointBlock];
    __shared__ unsigned char sTaken[kDisjointBlock];
    __shared__ unsigned int waveSum[kDisjointBlock / 64];
    const unsigned int base = blockIdx.x * kDisjointBlock, t = threadIdx.x, i = base + t;
    const unsigned int blockEnd = a.count - base < kDisjointBlock ? a.count : base + kDisjointBlock;
    unsigned int j = blockNext(a, sPos);
    sJ[t] = j;
    sTaken[t] = i < a.count && a.mark[i] != 0 ? 1 : 0;                  /* the entry */
    __syncthreads();
    for (unsigned int r = 0; r < kDisjointRounds; r++) {
        const bool inside = j < blockEnd, taken = sTaken[t] != 0;
        const unsigned int hop = inside ? sJ[j - base] : j;
        __syncthreads();
        if (taken && inside) sTaken[j - base] = 1;
        sJ[t] = hop;
        j = hop;
        __syncthreads();
    }
    const unsigned int taken = sTaken[t];
    if (i < a.count) a.mark[i] = (unsigned char)taken;                 /* only this block reads or writes the marks of its pairs in this launch */
    unsigned int total = 0;
    (void)blockExclusive<kDisjointBlock>(taken, waveSum, total);
    if (t == 0) a.tokCount[blockIdx.x] = total;
}

__global__ __launch_bounds__(kDisjointBlock) void pfac_disjoint_stage(DisjointArgs a)
{
    __shared__ unsigned int waveSum[kDisjointBlock / 64];
    const unsigned int i = blockIdx.x * kDisjointBlock + threadIdx.x;
    const unsigned int taken = i < a.count && a.mark[i] != 0 ? 1u : 0u;
    unsigned int total = 0;
    const unsigned int k = a.tokBase[blockIdx.x] + blockExclusive<kDisjointBlock>(taken, waveSum, total);
    if (taken && k < a.count) {                                        /* k <= i */
        a.jump[0][k] = (unsigned int)a.ids[i];
        a.jump[1][k] = (unsigned int)a.pos[i];
    }
}

__global__ __launch_bounds__(kPassThreads) void pfac_disjoint_emit(DisjointArgs a)
{
    __shared__ unsigned int waveSum[kPassThreads / 64];
    const unsigned int all = a.tokBase[a.blocks], tokens = all < a.count ? all : a.count;
    unsigned int own = 0;
    for (unsigned int k = blockIdx.x * kPassThreads + threadIdx.x; k < tokens; k += gridDim.x * kPassThreads) {
        const int id = (int)a.jump[0][k], at = (int)a.jump[1][k];
        a.outIds[k] = id;
        a.outPos[k] = at;
        unsigned int p, e;
        clampSpan(at, (unsigned int)id < a.numIds ? a.patternLen[id] : 0, a.n, p, e);
        own += e - p;
    }
    unsigned int total = 0;
    (void)blockExclusive<kPassThreads>(own, waveSum, total);
    if (threadIdx.x == 0 && total != 0) atomicAdd(a.covered, total);
}

/* ------------------------------------------------------------------ the replacement */

struct ReplaceArgs {
    const unsigned char *in;
    unsigned int n;
    const int *ids, *pos;               /* the caller's tokens: clamped, never trusted */
    unsigned int count;
    const int *patternLen;              /* by id */
    unsigned int numIds;                /* ids of [1, numIds) have a length AND two offsets */
    const int *replOff;
    const unsigned char *repl;
    unsigned int replBytes;
    size_t per;                         /* tokens per block of the delta / offsets passes: a multiple of kPassThreads */
    unsigned int blocks;
    unsigned long long *blockBase;      /* [blocks + 1] block sums of r - len -> their exclusive prefix; [blocks] = the sum of all (modulo 2^64) */
    long long *outStart;                /* [count] */
    unsigned char *out;
    size_t outCapacity;
    unsigned int misOut;                /* address of out & 15 */
};

/* token k: removes in[s, s + len), inserts repl[ro, ro + rlen); all inside their buffers whatever the arrays say */
struct Token { unsigned int s, len, ro, rlen; };
__device__ __forceinline__ Token tokenOf(const ReplaceArgs &a, size_t k)
{
    const int id = a.ids[k], at = a.pos[k];
    Token t;
    unsigned int e;
    clampSpan(at, id >= 1 && (unsigned int)id < a.numIds ? a.patternLen[id] : 0, a.n, t.s, e);
    t.len = e - t.s;
    t.ro = 0;
    t.rlen = 0;
    if (id >= 1 && (unsigned int)id < a.numIds) {
        unsigned int o0, o1, unused;
        clampSpan(a.replOff[id], 0, a.replBytes, o0, unused);
        clampSpan(a.replOff[id + 1], 0, a.replBytes, o1, unused);
        t.ro = o0;
        t.rlen = o1 > o0 ? o1 - o0 : 0u;
    }
    return t;
}

/* what a token adds to the size of the text, modulo 2^64 */
__device__ __forceinline__ unsigned long long deltaOf(const Token &t) { return (unsigned long long)t.rlen - (unsigned long long)t.len; }

__global__ __launch_bounds__(kPassThreads) void pfac_replace_delta(ReplaceArgs a)
{
    offsetsBlockTotal<kPassThreads>(a.count, a.per, a.blockBase, [&](size_t k) { return deltaOf(tokenOf(a, k)); });
}

__global__ __launch_bounds__(kPassThreads) void pfac_replace_offsets(ReplaceArgs a)
{
    Token t{};                                                         /* the token of the trip: from its value to its store */
    offsetsOfBlock<kPassThreads>(a.count, a.per, a.blockBase, [&](size_t k) { t = tokenOf(a, k); return deltaOf(t); },
                                 [&](size_t k, unsigned long long before) { a.outStart[k] = (long long)((unsigned long long)t.s + before); });
}

/* Tiles are cut in v = o + misOut, the output offset counted from the aligned 16-byte block that holds out[0].  SLOT q >= 1 is token q - 1; slot 0
 * stands in front of the first token: it starts at output byte 0, inserts nothing, and its gap starts at input byte 0.  Output byte o belongs to the
 * LAST slot that starts at or in front of it */
__global__ __launch_bounds__(kPassThreads) void pfac_replace_copy(ReplaceArgs a)
{
    __shared__ long long sOut[kReplaceStage + 1];                      /* [cnt]: where the slot behind the staged ones starts */
    __shared__ unsigned int sSrc[kReplaceStage], sRo[kReplaceStage], sRl[kReplaceStage];
    __shared__ unsigned int sFirst, sEnd;
    const unsigned long long total = (unsigned long long)a.n + a.blockBase[a.blocks];       /* a bad list: anything */
    const unsigned long long limit = total < a.outCapacity ? total : a.outCapacity;
    const unsigned int t = threadIdx.x;
    for (unsigned long long vLo = (unsigned long long)blockIdx.x * kOutTile; vLo < limit + a.misOut; vLo += (unsigned long long)gridDim.x * kOutTile) {
        const TileFrame<unsigned long long> f = tileFrame(vLo, a.misOut, limit);
        const unsigned long long oLo = f.oLo, oHi = f.oHi;
        if (t < 64u) {
            /* the first token that starts behind oLo -- the slot of the token in front of it owns oLo --, and the first that starts at or behind oHi */
            const unsigned int above = waveLowerBound(0u, a.count, [&](unsigned int k) { return a.outStart[k] > (long long)oLo; });
            const unsigned int behind = waveLowerBound(above, a.count, [&](unsigned int k) { return a.outStart[k] >= (long long)oHi; });
            if (t == 0) { sFirst = above; sEnd = behind + 1u; }
        }
        __syncthreads();
        const unsigned int qFirst = sFirst, qEnd = sEnd;
        const unsigned long long cLo = f.cLo, cHi = f.cLo + f.nb;
        const unsigned int nb = f.nb;
        const bool active = nb != 0;
        uint32_t w[4] = {0, 0, 0, 0};                                  /* byte b of the thread's bytes: bits 8 (b & 3) of w[b >> 2] */
        for (unsigned int qBase = qFirst; qBase < qEnd; qBase += kReplaceStage) {
            const unsigned int cnt = qEnd - qBase < kReplaceStage ? qEnd - qBase : kReplaceStage;
            if (qBase != qFirst) __syncthreads();                      /* the stage is rewritten */
            for (unsigned int j = t; j <= cnt; j += kPassThreads) {
                const unsigned int q = qBase + j;
                if (j == cnt) {
                    sOut[j] = q <= a.count ? a.outStart[q - 1] : LLONG_MAX;
                } else if (q == 0) {
                    sOut[j] = 0;
                    sSrc[j] = 0;
                    sRo[j] = 0;
                    sRl[j] = 0;
                } else {
                    const Token tk = tokenOf(a, q - 1);
                    sOut[j] = a.outStart[q - 1];
                    sSrc[j] = tk.s + tk.len;
                    sRo[j] = tk.ro;
                    sRl[j] = tk.rlen;
                }
            }
            __syncthreads();
            if (active) {
                unsigned int lo = 0, hi = cnt;                         /* the first staged slot that starts behind cLo */
                while (lo < hi) {
                    const unsigned int mid = (lo + hi) / 2;
                    if (sOut[mid] > (long long)cLo) hi = mid; else lo = mid + 1;
                }
                unsigned int j = lo ? lo - 1 : 0;
                bool whole = false;
                if (nb == 16u && sOut[j] <= (long long)cLo && sOut[j + 1] >= (long long)cHi) {
                    const unsigned long long d = cLo - (unsigned long long)sOut[j];
                    if (d >= sRl[j]) {                                 /* all sixteen in the gap behind slot j */
                        const unsigned long long src = (unsigned long long)sSrc[j] + (d - sRl[j]);
                        if (src + 16 <= a.n) {
                            const u32x4 x = loadBytes16(a.in, a.n, (unsigned int)src);
                            w[0] = x.x;
                            w[1] = x.y;
                            w[2] = x.z;
                            w[3] = x.w;
                            whole = true;
                        }
                    }
                }
                if (!whole) {
#pragma unroll
                    for (unsigned int b = 0; b < 16; b++) {
                        if (b < nb) {
                            const long long o = (long long)(cLo + b);
                            while (j + 1 < cnt && sOut[j + 1] <= o) j++;
                            if (sOut[j] <= o && o < sOut[j + 1]) {     /* else: a later trip's byte, or a bad list */
                                const unsigned long long d = (unsigned long long)(o - sOut[j]);
                                unsigned int byte = 0;
                                if (d < sRl[j]) {
                                    byte = a.repl[sRo[j] + (unsigned int)d];
                                } else {
                                    const unsigned long long src = (unsigned long long)sSrc[j] + (d - sRl[j]);
                                    if (src < a.n) byte = a.in[src];
                                }
                                w[b >> 2] |= byte << (8 * (b & 3));
                            }
                        }
                    }
                }
            }
        }
        if (active) tileStore(a.out, f, u32x4{w[0], w[1], w[2], w[3]});
        __syncthreads();                                               /* sFirst and the stage are rewritten by the next tile */
    }
}

} // namespace

extern "C" {

PFAC_status_t PFACX_disjointSelect(PFAC_handle_t handle, char *d_scan, size_t size, int hashed, const int *d_patternLen, size_t numIds, int *d_ids,
                                   int *d_pos, size_t *h_numTokens, size_t *h_coveredBytes)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!d_scan || !d_patternLen || !d_ids || !d_pos || !h_numTokens || !h_coveredBytes || size == 0 || size > (size_t)0x7fffffff)
        return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = handle;

    /* the ordered pairs, in the arrays that take the tokens */
    DisjointArgs a{};
    const PFAC_status_t st = pairsSelectHead(handle, d_scan, size, hashed, d_patternLen, numIds, d_ids, d_pos, h_numTokens, h_coveredBytes, a);
    if (st != PFAC_STATUS_SUCCESS || a.count == 0) return st;
    const size_t count = a.count;
    const size_t blocks = (count + kDisjointBlock - 1) / kDisjointBlock;
    a.blocks = (unsigned int)blocks;
    const PFAC_status_t carved = carveScratch(c->scratch.disjoint, [&](ScratchCarver &k) {
        a.jump[0] = k.take<unsigned int>(count);
        a.jump[1] = k.take<unsigned int>(count);
        a.mark = k.take<unsigned char>(count);
        a.tokCount = k.take<unsigned int>(blocks);
        a.tokBase = k.take<unsigned int>(blocks + 1);
        a.value = k.take<unsigned long long>(1, 8);            /* and, behind it, the word `covered` */
    });
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    a.covered = reinterpret_cast<unsigned int *>(a.value + 1);
    a.outIds = d_ids;
    a.outPos = d_pos;

    hipLaunchKernelGGL(pfac_disjoint_exit, dim3(a.blocks), dim3(kDisjointBlock), 0, 0, a);
    unsigned int from = 0;
    for (size_t reach = 1; reach < blocks; reach *= 2, from ^= 1u)     /* ceil(log2(blocks)) rounds; one block: none */
        hipLaunchKernelGGL(pfac_disjoint_double, dim3(gridFor(c, count)), dim3(kPassThreads), 0, 0, a, from);
    hipLaunchKernelGGL(pfac_disjoint_mark, dim3(a.blocks), dim3(kDisjointBlock), 0, 0, a);
    blockScan<OpSum>({{a.tokCount}, {a.tokBase}}, a.blocks, nullptr, a.covered);
    hipLaunchKernelGGL(pfac_disjoint_stage, dim3(a.blocks), dim3(kDisjointBlock), 0, 0, a);
    hipLaunchKernelGGL(pfac_disjoint_emit, dim3(gridFor(c, count)), dim3(kPassThreads), 0, 0, a);
    return pairsSelectTail(c, pfac::kHostDisjoint, a.tokBase + a.blocks, count, size, a.value, h_numTokens, h_coveredBytes);
}

PFAC_status_t PFACX_replaceRun(PFAC_handle_t handle, const char *d_input, size_t size, const int *d_ids, const int *d_pos, size_t numTokens,
                               const int *d_patternLen, size_t numIds, const int *d_replOff, size_t numOff, const char *d_replBytes, size_t replBytes,
                               char *d_out, size_t outCapacity, size_t *h_outBytes)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!h_outBytes || !d_input || size == 0 || size > (size_t)0x7fffffff || numTokens == 0 || numTokens > (size_t)0x7fffffff || !d_ids || !d_pos ||
        !d_patternLen || !d_replOff || numOff < 2 || (!d_replBytes && replBytes) || replBytes > (size_t)0x7fffffff || (!d_out && outCapacity))
        return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = handle;
    ReplaceArgs a{};
    a.in = reinterpret_cast<const unsigned char *>(d_input);
    a.n = (unsigned int)size;
    a.ids = d_ids;
    a.pos = d_pos;
    a.count = (unsigned int)numTokens;
    a.patternLen = d_patternLen;
    const size_t ids = numIds < numOff - 1 ? numIds : numOff - 1;      /* id + 1 < numOff */
    a.numIds = (unsigned int)(ids < (size_t)0x7fffffff ? ids : (size_t)0x7fffffff);
    a.replOff = d_replOff;
    a.repl = reinterpret_cast<const unsigned char *>(d_replBytes);
    a.replBytes = (unsigned int)replBytes;
    a.out = reinterpret_cast<unsigned char *>(d_out);
    a.outCapacity = outCapacity;
    a.misOut = (unsigned int)(reinterpret_cast<uintptr_t>(d_out) & 15u);
    a.blocks = offsetBlocks(c, numTokens, kPassThreads, a.per);
    const PFAC_status_t carved = carveScratch(c->scratch.disjoint, [&](ScratchCarver &k) {
        a.outStart = k.take<long long>(numTokens);
        a.blockBase = k.take<unsigned long long>((size_t)a.blocks + 1);
    });
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    const HostHandoff text(c, pfac::kHostReplace);
    hipLaunchKernelGGL(pfac_replace_delta, dim3(a.blocks), dim3(kPassThreads), 0, 0, a);
    hipLaunchKernelGGL(pfac_array_scan<unsigned long long>, dim3(1), dim3(1024), 0, 0, a.blockBase, a.blocks, a.blockBase + a.blocks,
                       reinterpret_cast<unsigned long long *>(text.d_value));
    hipLaunchKernelGGL(pfac_replace_offsets, dim3(a.blocks), dim3(kPassThreads), 0, 0, a);
    if (outCapacity) {                                                 /* whatever the size of the text, a launch never needs more tiles than outCapacity has */
        const unsigned long long tiles = ((unsigned long long)outCapacity + a.misOut + kOutTile - 1) / kOutTile, cap = gridCap(c, 8) * 4ull;
        hipLaunchKernelGGL(pfac_replace_copy, dim3((unsigned int)(tiles < cap ? tiles : cap)), dim3(kPassThreads), 0, 0, a);
    }
    unsigned long long sum = 0;
    if (!text.finish(&sum, a.blockBase + a.blocks)) return PFAC_STATUS_INTERNAL_ERROR;
    const unsigned long long total = (unsigned long long)size + sum;
    *h_outBytes = (size_t)total;
    return total > outCapacity ? PFACX_STATUS_OUTPUT_TRUNCATED : PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
