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
 * The body is seamBlock (scan_passes.h), which the flows call's block kernel shares; the kernel adds the LDS stage and the hand-off.
 * The flush of a stream is the same launch with an empty piece: every carried position, the staged bytes' end the end of the data.
 * Plain C++ and vector stores only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_stream.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"

namespace {

constexpr int kSeamBlock = 1024;
constexpr size_t kSeamLdsBytes = pfac::kStreamSeamLdsBytes;

struct StreamSeamArgs {
    SeamPiece piece;
    unsigned char *stage;                      /* device scratch of `staged` bytes, or null: LDS */
    int *ids, *pos;
    unsigned int *hostCount;                   /* mapped host memory: [0] the number of pairs, [1] seq, written behind it */
    unsigned int seq;
};

__global__ __launch_bounds__(kSeamBlock) void pfac_stream_seam(ScanArgs a, StreamSeamArgs s)
{
    __shared__ __attribute__((aligned(16))) unsigned char ldsStage[kSeamLdsBytes];
    __shared__ uint32_t waveCount[kSeamBlock / 64];
    const uint32_t written = seamBlock<kSeamBlock>(a, s.piece, s.stage != nullptr ? s.stage : ldsStage, s.ids, s.pos, waveCount);
    if (threadIdx.x == 0) {
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
    if (!c->tables.chainSlots || c->chainJumpLog2 <= 0 || !hostMapped(c)) return PFAC_STATUS_INTERNAL_ERROR;
    const size_t head = size < M - 1 ? size : M - 1;
    const size_t staged = carried + head;
    if (staged > kSeamLdsBytes && !d_stage) return PFAC_STATUS_INVALID_PARAMETER;

    ScanArgs a = ScanArgs{};
    fillChainArgs(c, a);                       /* the walk's view of the chained table (scan_common.h) */

    StreamSeamArgs args;
    SeamPiece &s = args.piece;
    s.carry = reinterpret_cast<const unsigned char *>(d_carry);
    s.piece = reinterpret_cast<const unsigned char *>(d_piece);
    s.carryNext = reinterpret_cast<unsigned char *>(d_carryNext);
    s.carried = (uint32_t)carried;
    s.staged = (uint32_t)staged;
    s.numFinal = (uint32_t)numFinal;
    const size_t all = carried + size;
    s.nextCarried = (uint32_t)(all < M - 1 ? all : M - 1);
    s.fold = c->caseInsensitive ? 1u : 0u;
    s.size = size;
    args.stage = staged > kSeamLdsBytes ? reinterpret_cast<unsigned char *>(d_stage) : nullptr;
    args.ids = d_ids;
    args.pos = d_pos;

    /* the launch itself stores the count and, behind it, the call's number */
    static_assert(pfac::kHostSeam.done == pfac::kHostSeam.value + 1, "pfac_stream_seam stores the two words side by side");
    const HostHandoff pairs(c, pfac::kHostSeam);
    args.hostCount = pairs.d_value;
    args.seq = pairs.seq;
    hipLaunchKernelGGL(pfac_stream_seam, dim3(1), dim3(kSeamBlock), 0, 0, a, args);
    if (!pairs.wait()) return PFAC_STATUS_INTERNAL_ERROR;
    const unsigned int count = *pairs.h_value;
    if (count > numFinal) return PFAC_STATUS_INTERNAL_ERROR;
    *h_count = (int)count;
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
