/*
 * batch_api.cpp -- PFACX_matchBatchFromDevice / ...FromHost / ...FromDeviceReduce (include/pfac_ext.h): many independent segments
 * of one buffer in one call, no match running from one segment into the next; and what every later call over "the longest pairs of each
 * segment" starts with (pfac_host.h: batchReduceLocked and scratchBatchPairs on the device, HostBatchPairs on the host).
 *
 * The GPU forms scan the whole concatenation with the unchanged match path (matchDeviceLocked / the compacted-output kernels:
 * whatever kernel variant, walker, perf mode and texture mode the handle selects) and then correct the few positions near a
 * segment end that the end changes (scan_batch.hip says why that is exact).  The CPU platforms match segment by segment.
 * Argument checks and status codes follow PFAC_matchFromDevice / PFAC_matchFromDeviceReduce.
 */
#include <hip/hip_runtime_api.h>

#include <algorithm>
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

PFAC_status_t batchReduceLocked(PFAC_context *c, char *d_scan, size_t size, const size_t *d_offsets, size_t numSegments, int *d_ids, int *d_pos,
                                int *d_segFirstPairs, int *h_count)
{
    PFAC_status_t st = d_offsets ? ensurePatternLen(c) : PFAC_STATUS_SUCCESS;
    int count = 0;
    if (st == PFAC_STATUS_SUCCESS) st = reduceOnDevice(c, d_scan, size, d_ids, d_pos, true, &count);      /* ordered: the fix-up and the segments' first pairs search the positions */
    if (st == PFAC_STATUS_SUCCESS && d_offsets)
        st = c->batch_reduce_fixup_ptr(c, d_scan, size, d_offsets, numSegments, d_ids, d_pos, &count, d_segFirstPairs, c->scratch.patternLen.get());
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (count < 0) return PFAC_STATUS_INTERNAL_ERROR;
    *h_count = count;
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t scratchBatchPairs(PFAC_context *c, char *d_input, size_t size, const size_t *d_offsets, size_t numSegments, BatchPairs *out)
{
    PFAC_status_t st = d_offsets ? c->scratch.allSegFirst.reserve(numSegments + 1) : PFAC_STATUS_SUCCESS;
    pfac::DeviceBuffer<int> &pairs = c->scratch.allPairs;
    if (st == PFAC_STATUS_SUCCESS) st = pairs.reserve(2 * size);
    if (st != PFAC_STATUS_SUCCESS) return st;
    out->ids = pairs.get();
    out->pos = out->ids + pairs.count() / 2;                               /* one allocation: the ids, then as many positions */
    int *const segFirstPairs = d_offsets ? c->scratch.allSegFirst.get() : nullptr;
    out->segFirstPairs = segFirstPairs;
    DeviceScan scan;                                                     /* a caseless set: the scan and the fix-up read the folded bytes */
    st = beginDeviceScan(c, d_input, size, &scan);
    if (st != PFAC_STATUS_SUCCESS) return st;
    out->d_scan = scan.d_scan;
    int count = 0;
    st = batchReduceLocked(c, scan.d_scan, size, d_offsets, numSegments, out->ids, out->pos, segFirstPairs, &count);
    out->count = (size_t)count;
    return st;
}

PFAC_status_t zeroSegmentArrays(size_t *d_segFirst, unsigned long long *d_segGroups, size_t numSegments)
{
    if (d_segFirst && numSegments && hipMemset(d_segFirst, 0, (numSegments + 1) * sizeof(size_t)) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
    if (d_segGroups && numSegments && hipMemset(d_segGroups, 0, numSegments * sizeof(unsigned long long)) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
    return PFAC_STATUS_SUCCESS;
}

HostBatchPairs::HostBatchPairs(PFAC_context *c, char *h_input, size_t size, const size_t *h_offsets, size_t numSegments, bool keepPositions,
                               std::unique_lock<std::mutex> &guard)
    : offsets(h_offsets ? h_offsets : whole_), c_(c), whole_{0, size}
{
    status = scan(h_input, size, numSegments, keepPositions, guard);
}

PFAC_status_t HostBatchPairs::scan(char *h_input, size_t size, size_t numSegments, bool keepPositions, std::unique_lock<std::mutex> &guard)
{
    PFAC_context *c = c_;
    if (hostLacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    const bool onGpu = c->platform == PFAC_PLATFORM_GPU;
    size_t longest = 0;
    for (size_t k = 0; k < numSegments; k++) longest = std::max(longest, offsets[k + 1] - offsets[k]);
    pairs_.emplace(size, keepPositions ? size : (onGpu ? 0 : longest));         /* positions not kept: the room one segment's scan needs on the CPU platforms */
    try {
        numPairs.assign(numSegments, 0);
    } catch (const std::bad_alloc &) {
        return PFAC_STATUS_ALLOC_FAILED;
    }
    if (!*pairs_) return PFAC_STATUS_ALLOC_FAILED;
    ids = pairs_->ids;
    pos = pairs_->pos;
    if (onGpu) {
        /* the pipelined batch path: the full result of every segment, compacted in place (pair z of a segment comes from an entry at or behind z) */
        const PFAC_status_t st = matchBatchHostOnGpu(c, h_input, size, offsets, numSegments, ids);
        if (st != PFAC_STATUS_SUCCESS) return st;
        for (size_t k = 0; k < numSegments; k++) {
            int z = 0;
            for (size_t i = offsets[k]; i < offsets[k + 1]; i++)
                if (ids[i] > 0) {
                    if (keepPositions) pos[offsets[k] + (size_t)z] = (int)(i - offsets[k]);     /* the pair's index in the full result is its position */
                    ids[offsets[k] + (size_t)z++] = ids[i];
                }
            numPairs[k] = z;
        }
        return PFAC_STATUS_SUCCESS;
    }
    guard.unlock();
    for (size_t k = 0; k < numSegments; k++) {
        const size_t n = offsets[k + 1] - offsets[k];
        if (n == 0) continue;
        const PFAC_status_t st = hostLongestPairs(c, h_input + offsets[k], n, ids + offsets[k], pos + (keepPositions ? offsets[k] : 0), &numPairs[k], nullptr);
        if (st != PFAC_STATUS_SUCCESS) return st;
    }
    return PFAC_STATUS_SUCCESS;
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
    DeviceScan scan;                                                    /* a caseless set: the scan and the fix-up read the folded bytes */
    PFAC_status_t st = beginDeviceScan(handle, d_input, size, &scan);
    if (st != PFAC_STATUS_SUCCESS) return st;
    int count = 0;
    st = batchReduceLocked(handle, scan.d_scan, size, d_offsets, numSegments, d_matched_result, d_pos, d_segFirst, &count);
    if (st != PFAC_STATUS_SUCCESS) return st;
    *h_num_matched = count;
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
