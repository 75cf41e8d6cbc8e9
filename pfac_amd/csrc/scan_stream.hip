/*
 * scan_stream.hip -- the seam of a stream call (include/pfac_ext.h: PFACX_stream*).
 *
 * A stream arrives in pieces.  A start position is final once maxPatternLen - 1 bytes behind it have been seen, so a stream keeps its
 * last M - 1 bytes (M = maxPatternLen), the CARRY, and every position in the carry is still pending when the next piece arrives.  The
 * piece itself is scanned in place by the unchanged compacted-output path (scan_module.hip: PFACX_streamReduce, which reports the
 * positions that are final and reads the M - 1 bytes behind them as read-ahead only).  What is left is the seam:
 *
 *   pfac_stream_seam   ONE block.  It stages [carry | first min(size, M - 1) bytes of the piece] -- at most 2 (M - 1) bytes -- in
 *                      LDS (in device scratch where a hostile set's M does not fit), folding the piece's bytes for a caseless set;
 *                      walks the carried start positions that this call makes final through the chained table, one position per
 *                      lane, every read checked against the end of the staged bytes (boundedWalk, scan_common.h: the walker the ends
 *                      of every input go through); and writes the (id, position) pairs in position order -- wave ballot, the
 *                      waves' counts added up through LDS -- with positions counted from the piece's first byte (negative).  The
 *                      same launch writes the stream's NEXT carry, the last min(M - 1, carried + size) bytes of [carry | piece], to
 *                      the stream's other carry buffer, and hands the number of pairs to the host in mapped memory.
 *
 * The flush of a stream is the same launch with an empty piece: every carried position, the staged bytes' end the end of the data.
 * Plain C++ and vector stores only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_stream.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_common.h"

namespace {

constexpr int kSeamBlock = 1024;
constexpr int kSeamWaves = kSeamBlock / 64;
constexpr size_t kSeamLdsBytes = pfac::kStreamSeamLdsBytes;

struct SeamArgs {
    const unsigned char *carry;                /* `carried` bytes */
    const unsigned char *piece;                /* `size` bytes (not read when size == 0) */
    unsigned char *carryNext;                  /* nextCarried bytes are written */
    unsigned char *stage;                      /* device scratch of `staged` bytes, or null: LDS */
    uint32_t carried, head, staged;            /* staged = carried + head, head = min(size, M - 1) */
    uint32_t numFinal;                         /* start positions [0, numFinal) of the staged bytes are walked, numFinal <= carried */
    uint32_t nextCarried;
    uint32_t fold;                             /* a caseless set: the piece's bytes are folded where they are staged or carried on */
    size_t size;
    int *ids, *pos;
    unsigned int *hostCount;                   /* mapped host memory: [0] the number of pairs, [1] seq, written behind it */
    unsigned int seq;
};

__device__ __forceinline__ unsigned char seamFold(unsigned char b, uint32_t fold) { return (unsigned char)(b + ((fold != 0 && (unsigned)(b - 'A') < 26u) ? 32 : 0)); }

__global__ __launch_bounds__(kSeamBlock) void pfac_stream_seam(ScanArgs a, SeamArgs s)
{
    __shared__ __attribute__((aligned(16))) unsigned char ldsStage[kSeamLdsBytes];
    __shared__ uint32_t waveCount[kSeamWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    unsigned char *stage = s.stage != nullptr ? s.stage : ldsStage;

    for (uint32_t i = tid; i < s.staged; i += kSeamBlock)
        stage[i] = i < s.carried ? s.carry[i] : seamFold(s.piece[i - s.carried], s.fold);
    /* the next carry: the last nextCarried bytes of [carry | piece] */
    const size_t all = (size_t)s.carried + s.size;
    for (uint32_t i = tid; i < s.nextCarried; i += kSeamBlock) {
        const size_t j = all - s.nextCarried + i;
        s.carryNext[i] = j < s.carried ? s.carry[j] : seamFold(s.piece[j - s.carried], s.fold);
    }
    __threadfence_block();
    __syncthreads();

    const ChainCtx<false> ctx(a);
    uint32_t written = 0;                      /* the same in every thread */
    for (uint32_t base = 0; base < s.numFinal; base += kSeamBlock) {
        const uint32_t p = base + tid;
        const int m = p < s.numFinal ? boundedWalk<false>(ctx, stage, p, s.staged) : 0;
        const uint64_t hits = __ballot(m > 0);
        if (lane == 0) waveCount[wave] = (uint32_t)__popcll(hits);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kSeamWaves; w++) {
            const uint32_t cnt = waveCount[w];
            before += (uint32_t)w < wave ? cnt : 0u;
            total += cnt;
        }
        if (m > 0) {
            const uint32_t at = written + before + laneRankIn(hits);
            s.ids[at] = m;
            s.pos[at] = (int)p - (int)s.carried;
        }
        written += total;
        __syncthreads();                       /* waveCount is rewritten by the next trip */
    }
    if (tid == 0) {
        __hip_atomic_store(s.hostCount, written, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(s.hostCount + 1, s.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

} // namespace

extern "C" {

PFAC_status_t PFACX_streamSeam(PFAC_handle_t handle, const char *d_carry, size_t carried, const char *d_piece, size_t size, size_t numFinal,
                               char *d_carryNext, char *d_stage, int *d_ids, int *d_pos, int *h_count)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    PFAC_context *c = handle;
    if (!h_count || !d_carryNext || (carried && !d_carry) || (size && !d_piece) || (numFinal && (!d_ids || !d_pos))) return PFAC_STATUS_INVALID_PARAMETER;
    const size_t M = (size_t)c->fa.maxPatternLen;
    if (M == 0 || carried > M - 1 || numFinal > carried) return PFAC_STATUS_INVALID_PARAMETER;
    if (!c->tables.chainSlots || c->chainJumpLog2 <= 0 || !c->d_modeHint || !c->h_modeHint) return PFAC_STATUS_INTERNAL_ERROR;
    const size_t head = size < M - 1 ? size : M - 1;
    const size_t staged = carried + head;
    if (staged > kSeamLdsBytes && !d_stage) return PFAC_STATUS_INVALID_PARAMETER;

    ScanArgs a = ScanArgs{};
    fillChainArgs(c, a);                       /* the walk's view of the chained table (scan_common.h) */

    SeamArgs s;
    s.carry = reinterpret_cast<const unsigned char *>(d_carry);
    s.piece = reinterpret_cast<const unsigned char *>(d_piece);
    s.carryNext = reinterpret_cast<unsigned char *>(d_carryNext);
    s.stage = staged > kSeamLdsBytes ? reinterpret_cast<unsigned char *>(d_stage) : nullptr;
    s.carried = (uint32_t)carried;
    s.head = (uint32_t)head;
    s.staged = (uint32_t)staged;
    s.numFinal = (uint32_t)numFinal;
    const size_t all = carried + size;
    s.nextCarried = (uint32_t)(all < M - 1 ? all : M - 1);
    s.fold = c->caseInsensitive ? 1u : 0u;
    s.size = size;
    s.ids = d_ids;
    s.pos = d_pos;
    s.hostCount = c->d_modeHint + pfac::kHostSeamCountWord;
    c->seamSeq = c->seamSeq + 1u ? c->seamSeq + 1u : 1u;
    s.seq = c->seamSeq;

    volatile unsigned int *hostCount = c->h_modeHint + pfac::kHostSeamCountWord, *hostDone = hostCount + 1;
    hipLaunchKernelGGL(pfac_stream_seam, dim3(1), dim3(kSeamBlock), 0, 0, a, s);
    if (hipGetLastError() != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
    /* the launch writes its number into host memory behind the count: polled for a while, like the compacted-output call's (scan_module.hip) */
    const HostWait w = waitHostSeq(hostDone, s.seq);
    if (w == HostWait::SyncFailed || (w == HostWait::Synced && __atomic_load_n(const_cast<unsigned int *>(hostDone), __ATOMIC_ACQUIRE) != s.seq))
        return PFAC_STATUS_INTERNAL_ERROR;
    const unsigned int count = *hostCount;
    if (count > numFinal) return PFAC_STATUS_INTERNAL_ERROR;
    *h_count = (int)count;
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
