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
 *                      the body of pfac_stream_seam (scan_passes.h: seamBlock), block and dynamic LDS stage sized by M (M = 243: 256 threads, 484 bytes), its
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
#include "scan_passes.h"

namespace {

constexpr int kWaveSeamMax = 64;               /* M - 1 up to here: the wave shape */
constexpr int kWaveSeamBlock = 256;
constexpr int kWaveSeamWaves = kWaveSeamBlock / 64;
constexpr int kWaveSlice = 2 * kWaveSeamMax + 16;      /* bytes of LDS per wave: [carry | head], 16-byte aligned slices */
constexpr int kSeamBlock = 1024;
constexpr size_t kSeamLdsBytes = pfac::kStreamSeamLdsBytes;
constexpr int kPieceBlock = 256;               /* pieces per block of the merge's per-piece launches */

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

/* piece k of the call as its seam sees it (an empty descriptor: nothing staged, carried on or walked) */
__device__ __forceinline__ SeamPiece seamPieceOf(const FlowsArgs &f, const PFACX_flowPiece_t &d)
{
    SeamPiece s;
    s.carry = f.carries + ((size_t)2 * d.flow + d.cur) * f.carryStride;
    s.carryNext = f.carries + ((size_t)2 * d.flow + (d.cur ^ 1u)) * f.carryStride;
    s.piece = f.in + d.start;
    s.carried = d.carried;
    s.staged = d.carried + (d.len < f.span ? d.len : f.span);
    s.numFinal = d.numFinal;
    const uint32_t all = d.carried + d.len;                       /* below 2^31 (flows_api.cpp: checkPieces) */
    s.nextCarried = all < f.span ? all : f.span;
    s.fold = f.fold;
    s.size = d.len;
    return s;
}

/* M - 1 <= 64: a wave per piece, a position per lane, no loop.  Every wave of the block runs the whole body (a wave without a piece has an
 * empty one), so the barrier and the ballot see all lanes */
__global__ __launch_bounds__(kWaveSeamBlock) void pfac_flows_seam_wave(ScanArgs a, FlowsArgs f)
{
    __shared__ __attribute__((aligned(16))) unsigned char slices[kWaveSeamWaves][kWaveSlice];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t k = blockIdx.x * kWaveSeamWaves + wave;
    const bool live = k < f.numPieces;
    PFACX_flowPiece_t d = PFACX_flowPiece_t{};
    if (live) d = f.pieces[k];
    const SeamPiece s = seamPieceOf(f, d);                        /* staged <= 2 * 64, nextCarried <= 64 */
    unsigned char *stage = slices[wave];
    seamStage(s, stage, lane, 64u);
    if (lane < s.nextCarried) s.carryNext[lane] = seamByte(s, s.carried + d.len - s.nextCarried + lane);
    __syncthreads();

    const ChainCtx<false> ctx(a);
    const int m = lane < s.numFinal ? boundedWalk<false>(ctx, stage, lane, s.staged) : 0;
    const uint64_t hits = __ballot(m > 0);
    if (m > 0) seamEmit(s, f.seamIds, f.seamPos, d.seamOff + laneRankIn(hits), m, lane);
    if (live && lane == 0) f.seamCount[k] = (uint32_t)__popcll(hits);
}

/* larger M: a block per piece, the body of pfac_stream_seam (scan_passes.h: seamBlock).  There are as many blocks as pieces, so the block and its
 * stage are sized by M on the host: min(1024, M - 1 rounded up to a wave) threads, 2 (M - 1) bytes of dynamic LDS (none where the stage is device scratch) */
__global__ __launch_bounds__(kSeamBlock) void pfac_flows_seam_block(ScanArgs a, FlowsArgs f)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsStage[];
    __shared__ uint32_t waveCount[kSeamBlock / 64];
    const uint32_t k = blockIdx.x;
    const PFACX_flowPiece_t d = f.pieces[k];
    unsigned char *stage = f.stage != nullptr ? f.stage + (size_t)k * f.stageStride : ldsStage;
    const uint32_t written = seamBlock<0>(a, seamPieceOf(f, d), stage, f.seamIds + d.seamOff, f.seamPos + d.seamOff, waveCount);
    if (threadIdx.x == 0) f.seamCount[k] = written;
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

__global__ __launch_bounds__(kPieceBlock) void pfac_flows_count(FlowsArgs f)
{
    __shared__ uint32_t waveTotals[kPieceBlock / 64];
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
    (void)blockExclusive<kPieceBlock>(count, waveTotals, total);
    if (threadIdx.x == 0) f.blockSums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kPieceBlock) void pfac_flows_sums(FlowsArgs f)
{
    __shared__ uint32_t waveTotals[kPieceBlock / 64];
    uint32_t running = 0;                      /* the same in every thread */
    for (uint32_t base = 0; base < f.numBlocks; base += kPieceBlock) {
        const uint32_t b = base + threadIdx.x;
        const uint32_t v = b < f.numBlocks ? f.blockSums[b] : 0u;
        uint32_t total;
        const uint32_t ex = blockExclusive<kPieceBlock>(v, waveTotals, total);
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
    __shared__ uint32_t waveTotals[kPieceBlock / 64];
    __shared__ uint32_t first[kPieceBlock], seams[kPieceBlock], from[kPieceBlock];
    const uint32_t k = blockIdx.x * kPieceBlock + threadIdx.x;
    const bool live = k < f.numPieces;
    uint32_t total;
    const uint32_t at = f.blockSums[blockIdx.x] + blockExclusive<kPieceBlock>(live ? f.counts[k] : 0u, waveTotals, total);
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
    if (!c->tables.chainSlots || c->chainJumpLog2 <= 0 || !hostMapped(c)) return PFAC_STATUS_INTERNAL_ERROR;

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
    static_assert(pfac::kHostFlows.done == pfac::kHostFlows.value + 1, "pfac_flows_done stores the two words side by side");
    const HostHandoff pairs(c, pfac::kHostFlows);
    f.hostCount = pairs.d_value;
    f.seq = pairs.seq;

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
    /* the last launch writes the call's number into host memory behind the total: polled for a while, like the compacted-output call's */
    if (!pairs.wait()) return PFAC_STATUS_INTERNAL_ERROR;
    const unsigned int total = *pairs.h_value;
    if (total > run->capacity) return PFAC_STATUS_INTERNAL_ERROR;
    *h_total = (int)total;
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
