/*
 * batch_api.cpp -- PFACX_matchBatchFromDevice / ...FromHost / ...FromDeviceReduce (include/pfac_ext.h): many independent segments
 * of one buffer in one call, no match running from one segment into the next.
 *
 * The GPU forms scan the whole concatenation with the unchanged match path (matchDeviceLocked / the compacted-output kernels:
 * whatever kernel variant, walker, perf mode and texture mode the handle selects) and then correct the few positions near a
 * segment end that the end changes (scan_batch.hip says why that is exact).  The CPU platforms match segment by segment.
 * Argument checks and status codes follow PFAC_matchFromDevice / PFAC_matchFromDeviceReduce.
 */
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <shared_mutex>

#include "pfac_host.h"

namespace pfac_internal {

/* offsets[0] == 0, offsets[n] == size, never decreasing */
bool batchOffsetsValid(const size_t *offsets, size_t numSegments, size_t size)
{
    if (offsets[0] != 0 || offsets[numSegments] != size) return false;
    for (size_t k = 0; k < numSegments; k++)
        if (offsets[k + 1] < offsets[k]) return false;
    return true;
}

/* the device copy of the pattern lengths by id that the fix-up kernels read (uploaded on the first batch call) */
PFAC_status_t ensurePatternLen(PFAC_context *c)
{
    if (c->scratch.patternLen) return PFAC_STATUS_SUCCESS;
    return c->scratch.patternLen.upload(c->fa.patternLen.data(), c->fa.patternLen.size());
}

/* PFACX_matchBatchFromDevice behind the argument checks (size > 0, numSegments > 0): the scan of the concatenation, then the fix-up
 * of the segment ends behind it on the default stream */
PFAC_status_t matchBatchDeviceLocked(PFAC_context *c, char *d_input, size_t size, const size_t *d_offsets, size_t numSegments, int *d_matched_result)
{
    if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    PFAC_status_t st = ensurePatternLen(c);
    if (st != PFAC_STATUS_SUCCESS) return st;
    st = matchDeviceLocked(c, d_input, size, d_matched_result);
    if (st != PFAC_STATUS_SUCCESS) return st;
    return c->batch_fixup_ptr(c, d_input, size, d_offsets, numSegments, d_matched_result, c->scratch.patternLen.get());
}

/* the CPU platforms: one match per non-empty segment.  PFAC_PLATFORM_CPU_OMP (with OMP_NUM_THREADS set, as for PFAC_matchFromHost)
 * spreads many short segments over the threads and runs a long one on all of them */
static PFAC_status_t matchBatchOnCpu(PFAC_context *c, const char *in, const size_t *offsets, size_t numSegments, int *out)
{
    {
        std::lock_guard<std::mutex> guard(c->lock);
        const PFAC_status_t st = prepareCpuPlatformLocked(c);
        if (st != PFAC_STATUS_SUCCESS) return st;
    }
    const bool omp = c->platform == PFAC_PLATFORM_CPU_OMP && std::getenv("OMP_NUM_THREADS") != nullptr;
    std::shared_lock<std::shared_mutex> r(c->tablesInUse);
    if (c->perfMode == PFAC_TIME_DRIVEN && c->h_dense.empty()) return PFAC_STATUS_PATTERNS_NOT_READY;
    const unsigned char *u = reinterpret_cast<const unsigned char *>(in);
    const size_t size = offsets[numSegments];
    const bool perSegment = omp && numSegments >= 64 && size / numSegments < (size_t(64) << 10);
    std::atomic<int> failed{PFAC_STATUS_SUCCESS};
    const long long ns = (long long)numSegments;
#pragma omp parallel for schedule(dynamic, 16) if (perSegment)
    for (long long k = 0; k < ns; k++) {
        const size_t s = offsets[k], e = offsets[k + 1];
        if (e == s) continue;
        const PFAC_status_t st = pfac::matchOnCpu(c, u + s, e - s, out + s, omp && !perSegment);
        if (st != PFAC_STATUS_SUCCESS) failed.store((int)st);
    }
    return (PFAC_status_t)failed.load();
}

} // namespace pfac_internal
using namespace pfac_internal;

extern "C" {

PFAC_status_t PFACX_matchBatchFromDevice(PFAC_handle_t handle, char *d_input, size_t size, const size_t *d_offsets, size_t numSegments,
                                         int *d_matched_result)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!handle->isPatternsReady) return PFAC_STATUS_PATTERNS_NOT_READY;
    if (!d_input || !d_offsets || !d_matched_result) return PFAC_STATUS_INVALID_PARAMETER;
    if (size == 0) return PFAC_STATUS_SUCCESS;
    if (numSegments == 0 || numSegments >= SIZE_MAX / sizeof(size_t)) return PFAC_STATUS_INVALID_PARAMETER;
    std::lock_guard<std::mutex> guard(handle->lock);
    char *in = d_input;
    const PFAC_status_t st = foldDeviceInput(handle, d_input, size, &in);
    if (st != PFAC_STATUS_SUCCESS) return st;
    return matchBatchDeviceLocked(handle, in, size, d_offsets, numSegments, d_matched_result);
}

PFAC_status_t PFACX_matchBatchFromHost(PFAC_handle_t handle, char *h_input, size_t size, const size_t *h_offsets, size_t numSegments,
                                       int *h_matched_result)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!handle->isPatternsReady) return PFAC_STATUS_PATTERNS_NOT_READY;
    if (!h_input || !h_offsets || !h_matched_result) return PFAC_STATUS_INVALID_PARAMETER;
    if (size == 0) return PFAC_STATUS_SUCCESS;
    if (numSegments == 0 || numSegments >= SIZE_MAX / sizeof(size_t)) return PFAC_STATUS_INVALID_PARAMETER;
    if (!batchOffsetsValid(h_offsets, numSegments, size)) return PFAC_STATUS_INVALID_PARAMETER;
    if (handle->platform != PFAC_PLATFORM_GPU) return matchBatchOnCpu(handle, h_input, h_offsets, numSegments, h_matched_result);
    std::lock_guard<std::mutex> guard(handle->lock);
    return matchBatchHostOnGpu(handle, h_input, size, h_offsets, numSegments, h_matched_result);
}

PFAC_status_t PFACX_matchBatchFromDeviceReduce(PFAC_handle_t handle, char *d_input, size_t size, const size_t *d_offsets, size_t numSegments,
                                               int *d_matched_result, int *d_pos, int *d_segFirst, int *h_num_matched)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!handle->isPatternsReady) return PFAC_STATUS_PATTERNS_NOT_READY;
    if (!d_input || !d_offsets || !d_matched_result || !d_pos || !d_segFirst || !h_num_matched) return PFAC_STATUS_INVALID_PARAMETER;
    if (size == 0) return PFAC_STATUS_SUCCESS;
    if (numSegments == 0 || numSegments >= SIZE_MAX / sizeof(size_t)) return PFAC_STATUS_INVALID_PARAMETER;
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    if (size > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    std::lock_guard<std::mutex> guard(handle->lock);
    PFAC_status_t st = ensurePatternLen(handle);
    if (st != PFAC_STATUS_SUCCESS) return st;
    DeviceScan scan;                                                    /* a caseless set: the scan and the fix-up read the folded bytes */
    st = beginDeviceScan(handle, d_input, size, &scan);
    if (st != PFAC_STATUS_SUCCESS) return st;
    d_input = scan.d_scan;
    int count = 0;
    st = reduceOnDevice(handle, d_input, size, d_matched_result, d_pos, true, &count);
    if (st != PFAC_STATUS_SUCCESS) return st;
    st = handle->batch_reduce_fixup_ptr(handle, d_input, size, d_offsets, numSegments, d_matched_result, d_pos, &count, d_segFirst, handle->scratch.patternLen.get());
    if (st != PFAC_STATUS_SUCCESS) return st;
    *h_num_matched = count;
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
