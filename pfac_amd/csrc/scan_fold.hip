/*
 * scan_fold.hip -- the ASCII fold of a caseless pattern set's input (include/pfac_ext.h: PFACX_READ_NOCASE).
 *
 * A caseless handle matches the folded set over the folded input.  The fold runs once, where input enters the library, in front of
 * the unchanged scan: the caller's device bytes are folded into handle scratch, a staging piece of the host paths is folded in place
 * right behind its upload.  Every kernel of the other units then reads folded bytes and none of them is touched.
 *
 *   pfac_fold<Q>   a grid-stride streaming pass, 16 bytes per lane and step, non-temporal loads and stores.  The body is aligned on
 *                  the DESTINATION (handle scratch, a staging piece: both 256-byte aligned, so a misaligned caller pointer still
 *                  hands the scan an aligned one).  Its source bytes lie m = 0..15 bytes into an aligned 16-byte block: Q = -1 for
 *                  m == 0 (one load per step, the in-place case), else Q = m / 4 and the step takes its 16 bytes out of two
 *                  aligned source blocks with v_alignbyte (scan_passes.h: funnel; r = m % 4; the second block is the next lane's first: the extra load
 *                  hits the cache, HBM traffic stays one read and one write per byte).  Bytes in front of the body (head) and
 *                  behind it (tail), fewer than 32 each, are folded one by one by the first lanes of the grid.
 *
 * The fold of a dword is SWAR, no branch per byte: with t = x & 0x7F7F7F7F, bit 7 of a byte of t + 0x3F3F3F3F says low7 >= 'A',
 * of t + 0x25252525 that low7 >= '[' (no carry leaves a byte: t <= 0x7F); a capital has the first and neither the second nor bit 7
 * of x, and gets 0x20 (its bit 5 is clear, so OR is the addition).  Plain C++ and vector stores only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_fold.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"

namespace {

constexpr int kFoldBlock = 256;
constexpr int kFoldUnroll = 4;                 /* 16-byte steps a lane has in flight */

struct FoldArgs {
    const unsigned char *src;                  /* the caller's bytes */
    unsigned char *dst;
    size_t head;                               /* bytes folded one by one in front of the body */
    size_t chunks;                             /* 16-byte steps of the body: dst + head + 16 j <- src + head + 16 j */
    size_t tail;                               /* bytes folded one by one behind it */
    const u32x4 *srcBlocks;                    /* the aligned source block that holds src[head] (src + head - m) */
    uint32_t r;                                /* m % 4 */
};

__device__ __forceinline__ uint32_t foldWord(uint32_t x)
{
    const uint32_t t = x & 0x7F7F7F7Fu;
    const uint32_t ge = t + 0x3F3F3F3Fu, gt = t + 0x25252525u;
    return x | (((ge ^ gt) & ~x & 0x80808080u) >> 2);
}

__device__ __forceinline__ u32x4 foldVec(u32x4 v) { return u32x4{foldWord(v.x), foldWord(v.y), foldWord(v.z), foldWord(v.w)}; }

template <int Q>
__global__ __launch_bounds__(kFoldBlock) void pfac_fold(FoldArgs f)
{
    const size_t tid = (size_t)blockIdx.x * kFoldBlock + threadIdx.x;
    const size_t lanes = (size_t)gridDim.x * kFoldBlock;
    if (tid < f.head) f.dst[tid] = foldByte(f.src[tid], 1u);
    if (tid < f.tail) {
        const size_t at = f.head + f.chunks * 16 + tid;
        f.dst[at] = foldByte(f.src[at], 1u);
    }
    u32x4 *out = reinterpret_cast<u32x4 *>(f.dst + f.head);
    for (size_t j0 = tid; j0 < f.chunks; j0 += lanes * kFoldUnroll) {
        u32x4 v[kFoldUnroll];
#pragma unroll
        for (int k = 0; k < kFoldUnroll; k++) {
            const size_t j = j0 + (size_t)k * lanes;
            if (j < f.chunks) {
                if constexpr (Q < 0) {
                    v[k] = __builtin_nontemporal_load(&f.srcBlocks[j]);
                } else {
                    const u32x4 a = __builtin_nontemporal_load(&f.srcBlocks[j]);
                    const u32x4 b = __builtin_nontemporal_load(&f.srcBlocks[j + 1]);
                    v[k] = funnel<Q>(a, b, f.r);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kFoldUnroll; k++) {
            const size_t j = j0 + (size_t)k * lanes;
            if (j < f.chunks) __builtin_nontemporal_store(foldVec(v[k]), &out[j]);
        }
    }
}

} // namespace

extern "C" {

PFAC_status_t PFACX_foldInput(PFAC_handle_t handle, const char *src, char *dst, size_t n)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!src || !dst) return PFAC_STATUS_INVALID_PARAMETER;
    if (n == 0) return PFAC_STATUS_SUCCESS;
    const PFAC_context *c = handle;
    const uintptr_t S = reinterpret_cast<uintptr_t>(src), D = reinterpret_cast<uintptr_t>(dst);
    if (S != D && S < D + n && D < S + n) return PFAC_STATUS_INVALID_PARAMETER;       /* in place, or apart */
    /* the body: dst + head 16-byte aligned; its source lies m bytes into an aligned block.  With m != 0 a step reads the block
     * behind its own too, so the first block must not start before src and the last must end by src + n: the head takes one
     * more step where the first would, the tail what the last would */
    size_t head = (16 - (D & 15)) & 15;
    size_t m = (S + head) & 15;
    if (m && S + head - m < S) head += 16;
    FoldArgs f;
    f.src = reinterpret_cast<const unsigned char *>(src);
    f.dst = reinterpret_cast<unsigned char *>(dst);
    f.r = (uint32_t)(m & 3);
    if (head >= n) {
        f.head = n; f.chunks = 0; f.tail = 0;
        f.srcBlocks = nullptr;
    } else {
        f.head = head;
        const size_t avail = n - head;
        f.chunks = m == 0 ? avail / 16 : (avail + m >= 32 ? (avail + m - 16) / 16 : 0);
        f.tail = avail - f.chunks * 16;
        f.srcBlocks = reinterpret_cast<const u32x4 *>(S + head - m);
    }
    const size_t lanes = f.chunks > f.head + f.tail ? f.chunks : f.head + f.tail;
    const size_t blocks = (lanes + kFoldBlock - 1) / kFoldBlock;
    const size_t cap = gridCap(c, 8);
    const dim3 grid((unsigned int)(blocks < cap ? blocks : cap)), block(kFoldBlock);
    if (f.chunks == 0 || m == 0) hipLaunchKernelGGL(pfac_fold<-1>, grid, block, 0, 0, f);
    else if (m < 4) hipLaunchKernelGGL(pfac_fold<0>, grid, block, 0, 0, f);
    else if (m < 8) hipLaunchKernelGGL(pfac_fold<1>, grid, block, 0, 0, f);
    else if (m < 12) hipLaunchKernelGGL(pfac_fold<2>, grid, block, 0, 0, f);
    else hipLaunchKernelGGL(pfac_fold<3>, grid, block, 0, 0, f);
    return hipGetLastError() == hipSuccess ? PFAC_STATUS_SUCCESS : PFAC_STATUS_INTERNAL_ERROR;
}

} /* extern "C" */
