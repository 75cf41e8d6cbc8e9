/*
 * scan_flows.hip -- the device side of a flows call (include/pfac_ext.h: PFACX_flows*): many streams advanced at once.
 *
 * A flows call takes a buffer cut into pieces, each the next piece of one flow (a stream).  With M = maxPatternLen, a
 * position p of a piece [s, e) below e - (M - 1) is final, and the longest pattern at p ends by e: the unchanged compacted scan of the
 * WHOLE buffer as one input (flows_api.cpp: reduceOnDevice) is already exact there, and pairs inside a piece's last M - 1 bytes are
 * pending and drop out.  What is left is done here, behind that scan on the default stream:
 *
 *   pfac_flows_seam    every piece's seam: [carry of its flow | first min(len, M - 1) bytes of the piece] staged in LDS (the piece's
 *                      bytes folded for a caseless set), the carried start positions the piece makes final walked through the
 *                      chained table with every read checked against the staged bytes' end (boundedWalk), hits ranked by wave
 *                      ballot and written in position order to the piece's slots of the seam staging list, positions counted from
 *                      the piece's first byte (negative); the flow's NEXT carry goes to its other buffer, so a failed call leaves
 *                      every flow as it was.  Two shapes, picked on the host by M: M - 1 <= 64 -- one WAVE per piece, four pieces
 *                      per block, each wave its own LDS slice, a position per lane, no loop; larger M -- one BLOCK per piece,
 *                      looping like pfac_stream_seam, block and dynamic LDS stage sized by M (M = 243: 256 threads, 484 bytes), its
 *                      stage in device scratch where 2 (M - 1) bytes exceed the LDS stage.
 *                      The flush is this launch with empty pieces.
 *   pfac_flows_count   a thread per piece: its range among the scan's position-ordered pairs by lower bound on [s, e - (M - 1)),
 *                      plus the seam's count; a block's sum goes to blockSums.
 *   pfac_flows_sums    one block: exclusive scan of blockSums, the total.
 *   pfac_flows_first   a thread per piece: the exclusive scan over the pieces (its block's offset + a block scan) = pieceFirst; then
 *                      the block's waves scatter the seam pairs of its pieces to their final places.
 *   pfac_flows_place   a thread per pair of the scan: its piece by upper bound on the piece starts, dropped if pending, else
 *                      rebased to the piece's start and written behind the piece's seam pairs.
 *   pfac_flows_done    the total and the call's number into mapped host memory: the host's one wait behind the scan's.
 *
 * These launches write nothing at or beyond `capacity` or the total count (the scan in front of them uses the caller's arrays below
 * `size` as its pair list, like every compacted call).  Plain C++ and vector stores only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_flows.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_common.h"

namespace {

constexpr int kWaveSeamMax = 64;               /* M - 1 up to here: the wave shape */
constexpr int kWaveSeamBlock = 256;
constexpr int kWaveSeamWaves = kWaveSeamBlock / 64;
constexpr int kWaveSlice = 2 * kWaveSeamMax + 16;      /* bytes of LDS per wave: [carry | head], 16-byte aligned slices */
constexpr int kSeamBlock = 1024;
constexpr int kSeamWaves = kSeamBlock / 64;
constexpr size_t kSeamLdsBytes = pfac::kStreamSeamLdsBytes;
constexpr int kPieceBlock = 256;               /* pieces per block of the merge's per-piece launches */
constexpr int kPieceWaves = kPieceBlock / 64;

struct FlowsArgs {
    const unsigned char *in;
    const PFACX_flowPiece_t *pieces;
    uint32_t numPieces;
    unsigned char *carries;
    size_t carryStride;
    unsigned char *stage;                      /* or null: LDS */
    size_t stageStride;
    int *seamIds, *seamPos;
    unsigned int *seamCount;                   /* null: no seams (M == 1) */
    unsigned int *pairLo, *counts, *blockSums;
    const int *scanIds, *scanPos;
    uint32_t scanCount;
    int *ids, *pos;
    uint32_t capacity;
    int *pieceFirst;
    uint32_t span;                             /* M - 1 */
    uint32_t fold;
    uint32_t numBlocks;                        /* of kPieceBlock pieces; blockSums[numBlocks] = the total */
    unsigned int *hostCount;
    unsigned int seq;
};

__device__ __forceinline__ unsigned char flowFold(unsigned char b, uint32_t fold) { return (unsigned char)(b + ((fold != 0 && (unsigned)(b - 'A') < 26u) ? 32 : 0)); }

/* M - 1 <= 64: a wave per piece.  Every wave of the block runs the whole body (a wave without a piece has an empty one), so the
 * barrier and the ballot see all lanes */
__global__ __launch_bounds__(kWaveSeamBlock) void pfac_flows_seam_wave(ScanArgs a, FlowsArgs f)
{
    __shared__ __attribute__((aligned(16))) unsigned char slices[kWaveSeamWaves][kWaveSlice];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t k = blockIdx.x * kWaveSeamWaves + wave;
    const bool live = k < f.numPieces;
    PFACX_flowPiece_t d = PFACX_flowPiece_t{};
    if (live) d = f.pieces[k];
    const uint32_t head = d.len < f.span ? d.len : f.span;
    const uint32_t staged = d.carried + head;                     /* <= 2 * 64 */
    const unsigned char *carry = f.carries + ((size_t)2 * d.flow + d.cur) * f.carryStride;
    unsigned char *carryNext = f.carries + ((size_t)2 * d.flow + (d.cur ^ 1u)) * f.carryStride;
    const unsigned char *piece = f.in + d.start;
    unsigned char *stage = slices[wave];
    for (uint32_t i = lane; i < staged; i += 64u)
        stage[i] = i < d.carried ? carry[i] : flowFold(piece[i - d.carried], f.fold);
    /* the next carry: the last nextCarried bytes of [carry | piece] */
    const uint32_t all = d.carried + d.len;
    const uint32_t nextCarried = all < f.span ? all : f.span;
    if (lane < nextCarried) {
        const uint32_t j = all - nextCarried + lane;
        carryNext[lane] = j < d.carried ? carry[j] : flowFold(piece[j - d.carried], f.fold);
    }
    __syncthreads();

    const ChainCtx<false> ctx(a);
    const int m = lane < d.numFinal ? boundedWalk<false>(ctx, stage, lane, staged) : 0;
    const uint64_t hits = __ballot(m > 0);
    if (m > 0) {
        const uint32_t at = d.seamOff + laneRankIn(hits);
        f.seamIds[at] = m;
        f.seamPos[at] = (int)lane - (int)d.carried;
    }
    if (live && lane == 0) f.seamCount[k] = (uint32_t)__popcll(hits);
}

/* larger M: a block per piece, the loop of pfac_stream_seam.  There are as many blocks as pieces, so the block and its stage are sized by M on
 * the host: min(1024, M - 1 rounded up to a wave) threads, 2 (M - 1) bytes of dynamic LDS (none where the stage is device scratch) */
__global__ __launch_bounds__(kSeamBlock) void pfac_flows_seam_block(ScanArgs a, FlowsArgs f)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsStage[];
    __shared__ uint32_t waveCount[kSeamWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t kBlock = blockDim.x, waves = kBlock >> 6;
    const uint32_t k = blockIdx.x;
    const PFACX_flowPiece_t d = f.pieces[k];
    const uint32_t head = d.len < f.span ? d.len : f.span;
    const uint32_t staged = d.carried + head;
    const unsigned char *carry = f.carries + ((size_t)2 * d.flow + d.cur) * f.carryStride;
    unsigned char *carryNext = f.carries + ((size_t)2 * d.flow + (d.cur ^ 1u)) * f.carryStride;
    const unsigned char *piece = f.in + d.start;
    unsigned char *stage = f.stage != nullptr ? f.stage + (size_t)k * f.stageStride : ldsStage;

    for (uint32_t i = tid; i < staged; i += kBlock)
        stage[i] = i < d.carried ? carry[i] : flowFold(piece[i - d.carried], f.fold);
    const size_t all = (size_t)d.carried + d.len;
    const uint32_t nextCarried = (uint32_t)(all < f.span ? all : f.span);
    for (uint32_t i = tid; i < nextCarried; i += kBlock) {
        const size_t j = all - nextCarried + i;
        carryNext[i] = j < d.carried ? carry[j] : flowFold(piece[j - d.carried], f.fold);
    }
    __threadfence_block();
    __syncthreads();

    const ChainCtx<false> ctx(a);
    uint32_t written = 0;                      /* the same in every thread */
    for (uint32_t base = 0; base < d.numFinal; base += kBlock) {
        const uint32_t p = base + tid;
        const int m = p < d.numFinal ? boundedWalk<false>(ctx, stage, p, staged) : 0;
        const uint64_t hits = __ballot(m > 0);
        if (lane == 0) waveCount[wave] = (uint32_t)__popcll(hits);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < waves; w++) {
            const uint32_t cnt = waveCount[w];
            before += w < wave ? cnt : 0u;
            total += cnt;
        }
        if (m > 0) {
            const uint32_t at = d.seamOff + written + before + laneRankIn(hits);
            f.seamIds[at] = m;
            f.seamPos[at] = (int)p - (int)d.carried;
        }
        written += total;
        __syncthreads();                       /* waveCount is rewritten by the next trip */
    }
    if (tid == 0) f.seamCount[k] = written;
}

/* first index in pos[0, n) whose entry is >= x (pos ascending) */
__device__ __forceinline__ uint32_t lowerBound(const int *pos, uint32_t n, uint32_t x)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint32_t)pos[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

/* the block's exclusive scan of one value per thread (kPieceBlock threads); *blockTotal: the sum.  Every thread calls it */
__device__ __forceinline__ uint32_t blockExclusive(uint32_t v, uint32_t *waveTotals, uint32_t *blockTotal)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t inc = waveInclusiveScan(v);
    if (lane == 63u) waveTotals[wave] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kPieceWaves; w++) {
        const uint32_t t = waveTotals[w];
        before += (uint32_t)w < wave ? t : 0u;
        total += t;
    }
    __syncthreads();                           /* waveTotals may be used again */
    *blockTotal = total;
    return before + inc - v;
}

__global__ __launch_bounds__(kPieceBlock) void pfac_flows_count(FlowsArgs f)
{
    __shared__ uint32_t waveTotals[kPieceWaves];
    const uint32_t k = blockIdx.x * kPieceBlock + threadIdx.x;
    uint32_t count = 0;
    if (k < f.numPieces) {
        const PFACX_flowPiece_t d = f.pieces[k];
        uint32_t lo = 0, n = 0;
        if (d.len > f.span && f.scanCount) {
            lo = lowerBound(f.scanPos, f.scanCount, d.start);
            n = lowerBound(f.scanPos, f.scanCount, d.start + d.len - f.span) - lo;
        }
        f.pairLo[k] = lo;
        count = n + (f.seamCount != nullptr ? f.seamCount[k] : 0u);
        f.counts[k] = count;
    }
    uint32_t total;
    (void)blockExclusive(count, waveTotals, &total);
    if (threadIdx.x == 0) f.blockSums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kPieceBlock) void pfac_flows_sums(FlowsArgs f)
{
    __shared__ uint32_t waveTotals[kPieceWaves];
    uint32_t running = 0;                      /* the same in every thread */
    for (uint32_t base = 0; base < f.numBlocks; base += kPieceBlock) {
        const uint32_t b = base + threadIdx.x;
        const uint32_t v = b < f.numBlocks ? f.blockSums[b] : 0u;
        uint32_t total;
        const uint32_t ex = blockExclusive(v, waveTotals, &total);
        if (b < f.numBlocks) f.blockSums[b] = running + ex;
        running += total;
    }
    if (threadIdx.x == 0) {
        f.blockSums[f.numBlocks] = running;
        f.pieceFirst[f.numPieces] = (int)running;
    }
}

__global__ __launch_bounds__(kPieceBlock) void pfac_flows_first(FlowsArgs f)
{
    __shared__ uint32_t waveTotals[kPieceWaves];
    __shared__ uint32_t first[kPieceBlock], seams[kPieceBlock], from[kPieceBlock];
    const uint32_t k = blockIdx.x * kPieceBlock + threadIdx.x;
    const bool live = k < f.numPieces;
    uint32_t total;
    const uint32_t at = f.blockSums[blockIdx.x] + blockExclusive(live ? f.counts[k] : 0u, waveTotals, &total);
    if (live) f.pieceFirst[k] = (int)at;
    first[threadIdx.x] = at;
    seams[threadIdx.x] = live && f.seamCount != nullptr ? f.seamCount[k] : 0u;
    from[threadIdx.x] = live ? f.pieces[k].seamOff : 0u;
    __syncthreads();
    /* the seam pairs of this block's pieces to their places: a wave takes 64 of the pieces, one after the other, a lane per pair */
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t limit = f.blockSums[f.numBlocks] < f.capacity ? f.blockSums[f.numBlocks] : f.capacity;
    for (uint32_t j = wave * 64u; j < wave * 64u + 64u; j++) {
        const uint32_t n = seams[j], to = first[j], src = from[j];
        for (uint32_t i = lane; i < n; i += 64u) {
            if (to + i < limit) {
                f.ids[to + i] = f.seamIds[src + i];
                f.pos[to + i] = f.seamPos[src + i];
            }
        }
    }
}

__global__ __launch_bounds__(256) void pfac_flows_place(FlowsArgs f)
{
    const uint32_t limit = f.blockSums[f.numBlocks] < f.capacity ? f.blockSums[f.numBlocks] : f.capacity;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < f.scanCount; j += gridDim.x * 256u) {
        const uint32_t p = (uint32_t)f.scanPos[j];
        /* the last piece that starts at or before p: an empty piece shares its start with the piece behind it, which then is the one */
        uint32_t lo = 0, hi = f.numPieces;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (f.pieces[mid].start <= p) lo = mid + 1; else hi = mid;
        }
        if (lo == 0) continue;
        const uint32_t k = lo - 1;
        const PFACX_flowPiece_t d = f.pieces[k];
        if (d.len <= f.span || p - d.start >= d.len - f.span) continue;       /* pending: the next call's */
        const uint32_t to = (uint32_t)f.pieceFirst[k] + (f.seamCount != nullptr ? f.seamCount[k] : 0u) + (j - f.pairLo[k]);
        if (to < limit) {
            f.ids[to] = f.scanIds[j];
            f.pos[to] = (int)(p - d.start);
        }
    }
}

__global__ void pfac_flows_done(FlowsArgs f)
{
    if (threadIdx.x == 0) {
        __hip_atomic_store(f.hostCount, f.blockSums[f.numBlocks], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(f.hostCount + 1, f.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

} // namespace

extern "C" {

PFAC_status_t PFACX_flowsRun(PFAC_handle_t handle, const PFACX_flowsRun_t *run, int *h_total)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    PFAC_context *c = handle;
    if (!run || !h_total || !run->d_pieces || run->numPieces == 0 || run->numPieces > 0x7fffffffu || !run->d_pairLo || !run->d_counts ||
        !run->d_blockSums || !run->d_pieceFirst || run->capacity > 0x7fffffffu || run->scanCount > 0x7fffffffu)
        return PFAC_STATUS_INVALID_PARAMETER;
    if (run->scanCount && (!run->d_scanIds || !run->d_scanPos || !run->d_ids || !run->d_pos)) return PFAC_STATUS_INVALID_PARAMETER;
    const size_t M = (size_t)c->fa.maxPatternLen;
    if (M == 0) return PFAC_STATUS_INVALID_PARAMETER;
    const bool seams = M > 1;
    if (seams && (!run->d_carries || !run->d_seamCount || run->carryStride < M - 1)) return PFAC_STATUS_INVALID_PARAMETER;
    if (seams && 2 * (M - 1) > kSeamLdsBytes && (!run->d_stage || run->stageStride < 2 * (M - 1))) return PFAC_STATUS_INVALID_PARAMETER;
    if (!c->tables.chainSlots || c->chainJumpLog2 <= 0 || !c->d_modeHint || !c->h_modeHint) return PFAC_STATUS_INTERNAL_ERROR;

    ScanArgs a = ScanArgs{};
    fillChainArgs(c, a);                       /* the walk's view of the chained table (scan_common.h) */

    FlowsArgs f;
    f.in = reinterpret_cast<const unsigned char *>(run->d_input);
    f.pieces = run->d_pieces;
    f.numPieces = (uint32_t)run->numPieces;
    f.carries = reinterpret_cast<unsigned char *>(run->d_carries);
    f.carryStride = run->carryStride;
    f.stage = seams && 2 * (M - 1) > kSeamLdsBytes ? reinterpret_cast<unsigned char *>(run->d_stage) : nullptr;
    f.stageStride = run->stageStride;
    f.seamIds = run->d_seamIds;
    f.seamPos = run->d_seamPos;
    f.seamCount = seams ? run->d_seamCount : nullptr;
    f.pairLo = run->d_pairLo;
    f.counts = run->d_counts;
    f.blockSums = run->d_blockSums;
    f.scanIds = run->d_scanIds;
    f.scanPos = run->d_scanPos;
    f.scanCount = (uint32_t)run->scanCount;
    f.ids = run->d_ids;
    f.pos = run->d_pos;
    f.capacity = (uint32_t)run->capacity;
    f.pieceFirst = run->d_pieceFirst;
    f.span = (uint32_t)(M - 1);
    f.fold = c->caseInsensitive ? 1u : 0u;
    f.numBlocks = (f.numPieces + kPieceBlock - 1) / kPieceBlock;
    f.hostCount = c->d_modeHint + pfac::kHostFlowsCountWord;
    c->flowsSeq = c->flowsSeq + 1u ? c->flowsSeq + 1u : 1u;
    f.seq = c->flowsSeq;

    if (seams) {
        if (M - 1 <= (size_t)kWaveSeamMax)
            hipLaunchKernelGGL(pfac_flows_seam_wave, dim3((f.numPieces + kWaveSeamWaves - 1) / kWaveSeamWaves), dim3(kWaveSeamBlock), 0, 0, a, f);
        else {
            const size_t threads = ((M - 1) + 63) & ~size_t(63);
            const size_t lds = f.stage != nullptr ? 0 : (2 * (M - 1) + 15) & ~size_t(15);
            hipLaunchKernelGGL(pfac_flows_seam_block, dim3(f.numPieces), dim3((unsigned int)(threads < (size_t)kSeamBlock ? threads : (size_t)kSeamBlock)), lds, 0, a, f);
        }
    }
    hipLaunchKernelGGL(pfac_flows_count, dim3(f.numBlocks), dim3(kPieceBlock), 0, 0, f);
    hipLaunchKernelGGL(pfac_flows_sums, dim3(1), dim3(kPieceBlock), 0, 0, f);
    hipLaunchKernelGGL(pfac_flows_first, dim3(f.numBlocks), dim3(kPieceBlock), 0, 0, f);
    if (f.scanCount) hipLaunchKernelGGL(pfac_flows_place, dim3(gridFor(c, f.scanCount)), dim3(256), 0, 0, f);
    hipLaunchKernelGGL(pfac_flows_done, dim3(1), dim3(64), 0, 0, f);
    if (hipGetLastError() != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
    /* the last launch writes the call's number into host memory behind the total: polled for a while, like the compacted-output call's */
    volatile unsigned int *hostCount = c->h_modeHint + pfac::kHostFlowsCountWord, *hostDone = hostCount + 1;
    const HostWait w = waitHostSeq(hostDone, f.seq);
    if (w == HostWait::SyncFailed || (w == HostWait::Synced && __atomic_load_n(const_cast<unsigned int *>(hostDone), __ATOMIC_ACQUIRE) != f.seq))
        return PFAC_STATUS_INTERNAL_ERROR;
    const unsigned int total = *hostCount;
    if (total > run->capacity) return PFAC_STATUS_INTERNAL_ERROR;
    *h_total = (int)total;
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
