/*
 * cover_api.cpp -- PFACX_coverSpansFromDevice / ...FromHost (include/pfac_ext.h): an unsorted list of intervals over [0, size) as the maximal
 * runs of the bytes they cover, in the format PFACX_redactSpansFromDevice takes.
 *
 * No matcher runs and no pattern set is read: the device form is the argument checks and one call into the module (scan_cover.hip:
 * PFACX_coverRun, a bitmap hierarchy in handle scratch); the host form clamps the intervals into a list of its own, sorts it by start and merges
 * with one running maximum -- memory proportional to the intervals, never to `size`.
 */
#include <hip/hip_runtime_api.h>

#include <mutex>
#include <utility>
#include <vector>

#include "pfac_host.h"

namespace pfac_internal {

/* what both forms refuse, in the order of the header */
static PFAC_status_t checkCoverArgs(PFAC_context *c, const int *start, const int *end, size_t numIntervals, size_t size, unsigned int flags,
                                    const int *spanStart, const int *spanLen, size_t capacity, const size_t *numSpans, const size_t *coveredBytes)
{
    if (!c) return PFAC_STATUS_INVALID_HANDLE;
    if (!numSpans || !coveredBytes) return PFAC_STATUS_INVALID_PARAMETER;
    if (numIntervals && (!start || !end)) return PFAC_STATUS_INVALID_PARAMETER;
    if (capacity && (!spanStart || !spanLen)) return PFAC_STATUS_INVALID_PARAMETER;
    if (size > kMaxInt || numIntervals > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    if (flags & ~PFACX_COVER_LENGTHS) return PFAC_STATUS_INVALID_PARAMETER;
    return PFAC_STATUS_SUCCESS;
}

/* interval i inside [0, size]: false where nothing of it is left */
static inline bool clampInterval(int s, int second, bool lengths, long long size, long long &lo, long long &hi)
{
    lo = s;
    hi = lengths ? (long long)s + (long long)second : (long long)second;
    if (lo < 0) lo = 0;
    if (hi > size) hi = size;
    return lo < hi;
}

} // namespace pfac_internal
using namespace pfac_internal;

extern "C" {

PFAC_status_t PFACX_coverSpansFromDevice(PFAC_handle_t handle, const int *d_start, const int *d_end, size_t numIntervals, size_t size,
                                         unsigned int flags, int *d_spanStart, int *d_spanLen, size_t capacity,
                                         size_t *h_numSpans, size_t *h_coveredBytes)
{
    const PFAC_status_t st = checkCoverArgs(handle, d_start, d_end, numIntervals, size, flags, d_spanStart, d_spanLen, capacity, h_numSpans, h_coveredBytes);
    if (st != PFAC_STATUS_SUCCESS) return st;
    /* no more than (size + 1) / 2 spans exist: what lies behind that many entries is never written, and does not count as the call's */
    const size_t written = capacity < (size + 1) / 2 ? capacity : (size + 1) / 2;
    for (const int *out : {d_spanStart, d_spanLen})
        for (const int *in : {d_start, d_end})
            if (overlap(out, capacity * sizeof(int), in, numIntervals * sizeof(int))) return PFAC_STATUS_INVALID_PARAMETER;
    if (size == 0) { *h_numSpans = 0; *h_coveredBytes = 0; return PFAC_STATUS_SUCCESS; }
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    if (numIntervals == 0) { *h_numSpans = 0; *h_coveredBytes = 0; return PFAC_STATUS_SUCCESS; }
    std::lock_guard<std::mutex> guard(handle->lock);
    PFACX_coverRun_t run{};
    run.d_start = d_start;
    run.d_end = d_end;
    run.numIntervals = numIntervals;
    run.size = size;
    run.flags = flags;
    run.d_spanStart = d_spanStart;
    run.d_spanLen = d_spanLen;
    run.capacity = written;
    size_t numSpans = 0, covered = 0;
    const PFAC_status_t ran = handle->cover_run_ptr(handle, &run, &numSpans, &covered);
    if (ran != PFAC_STATUS_SUCCESS) return ran;
    *h_numSpans = numSpans;
    *h_coveredBytes = covered;
    return truncatedIf(numSpans, capacity);
}

PFAC_status_t PFACX_coverSpansFromHost(PFAC_handle_t handle, const int *h_start, const int *h_end, size_t numIntervals, size_t size,
                                       unsigned int flags, int *h_spanStart, int *h_spanLen, size_t capacity,
                                       size_t *h_numSpans, size_t *h_coveredBytes)
{
    const PFAC_status_t st = checkCoverArgs(handle, h_start, h_end, numIntervals, size, flags, h_spanStart, h_spanLen, capacity, h_numSpans, h_coveredBytes);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0 || numIntervals == 0) { *h_numSpans = 0; *h_coveredBytes = 0; return PFAC_STATUS_SUCCESS; }
    std::lock_guard<std::mutex> guard(handle->lock);
    const bool lengths = (flags & PFACX_COVER_LENGTHS) != 0;
    std::vector<std::pair<int, int>> kept;                     /* the intervals that cover something, clamped: the caller's arrays stay as they are */
    try {
        for (size_t i = 0; i < numIntervals; i++) {
            long long lo, hi;
            if (clampInterval(h_start[i], h_end[i], lengths, (long long)size, lo, hi)) kept.emplace_back((int)lo, (int)hi);
        }
        std::stable_sort(kept.begin(), kept.end(), [](const std::pair<int, int> &a, const std::pair<int, int> &b) { return a.first < b.first; });
    } catch (const std::bad_alloc &) { return PFAC_STATUS_ALLOC_FAILED; }
    size_t spans = 0, covered = 0;
    const auto close = [&](int s, int e) {
        if (spans < capacity) { h_spanStart[spans] = s; h_spanLen[spans] = e - s; }
        spans++;
        covered += (size_t)(e - s);
    };
    int s = 0, e = 0;
    bool open = false;
    for (const std::pair<int, int> &iv : kept) {
        if (open && iv.first <= e) {                           /* overlaps or touches the run in front of it: one span */
            if (iv.second > e) e = iv.second;
            continue;
        }
        if (open) close(s, e);
        s = iv.first;
        e = iv.second;
        open = true;
    }
    if (open) close(s, e);
    *h_numSpans = spans;
    *h_coveredBytes = covered;
    return truncatedIf(spans, capacity);
}

} /* extern "C" */
