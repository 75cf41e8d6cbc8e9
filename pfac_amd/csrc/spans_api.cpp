/*
 * spans_api.cpp -- PFACX_matchSpansFromDevice / ...FromHost / PFACX_redactSpansFromDevice (include/pfac_ext.h): the bytes of a buffer that belong
 * to a match, as maximal runs, and the buffer with those bytes overwritten.
 *
 * Every pattern that occurs at a position is a prefix of the longest one there, so the covered bytes are the union of [p, p + len(r[p])) over the
 * non-zero positions of the longest-match result r.  The device form is the compacted scan with its ordering launches and a handful of passes over
 * the pairs behind it (scan_spans.hip: PFACX_spansSelect); the host form takes the longest pairs from hostLongestPairs and merges here with one
 * sequential running maximum, the list written in place over the arrays the pairs are in (span i comes from pair >= i, so entry i of either array
 * is free by the time span i is listed).
 */
#include <hip/hip_runtime_api.h>

#include <mutex>

#include "pfac_host.h"

namespace pfac_internal {

/* one running-maximum merge: next(p, e) yields the matches [p, e) in position order, false at the end */
template <class Next>
static void mergeSpans(Next next, int *spanStart, int *spanLen, size_t *numSpans, size_t *coveredBytes)
{
    size_t o = 0, covered = 0, start = 0, end = 0, p = 0, e = 0;
    bool open = false;
    while (next(p, e)) {
        if (open && p <= end) {
            if (e > end) end = e;
            continue;
        }
        if (open) { spanStart[o] = (int)start; spanLen[o] = (int)(end - start); covered += end - start; o++; }
        start = p;
        end = e;
        open = true;
    }
    if (open) { spanStart[o] = (int)start; spanLen[o] = (int)(end - start); covered += end - start; o++; }
    *numSpans = o;
    *coveredBytes = covered;
}

} // namespace pfac_internal
using namespace pfac_internal;

extern "C" {

PFAC_status_t PFACX_matchSpansFromDevice(PFAC_handle_t handle, char *d_input, size_t size, int *d_spanStart, int *d_spanLen, size_t capacity,
                                         size_t *h_numSpans, size_t *h_coveredBytes)
{
    PFAC_status_t st = checkSetAndPointers(handle, {d_input, d_spanStart, d_spanLen, h_numSpans, h_coveredBytes});
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0) { *h_numSpans = 0; *h_coveredBytes = 0; return PFAC_STATUS_SUCCESS; }
    if (capacity < size) return PFAC_STATUS_INVALID_PARAMETER;
    if (size > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(handle->lock);
    st = ensurePatternLen(handle);
    if (st != PFAC_STATUS_SUCCESS) return st;
    DeviceScan scan;                                                       /* a caseless set: the scan reads the folded copy */
    st = beginDeviceScan(handle, d_input, size, &scan);
    if (st != PFAC_STATUS_SUCCESS) return st;
    return handle->spans_select_ptr(handle, scan.d_scan, size, scan.hashed, handle->scratch.patternLen.get(), handle->scratch.patternLen.count(),
                                    d_spanStart, d_spanLen, h_numSpans, h_coveredBytes);
}

PFAC_status_t PFACX_matchSpansFromHost(PFAC_handle_t handle, char *h_input, size_t size, int *h_spanStart, int *h_spanLen, size_t capacity,
                                       size_t *h_numSpans, size_t *h_coveredBytes)
{
    PFAC_status_t st = checkSetAndPointers(handle, {h_input, h_spanStart, h_spanLen, h_numSpans, h_coveredBytes});
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0) { *h_numSpans = 0; *h_coveredBytes = 0; return PFAC_STATUS_SUCCESS; }
    if (capacity < size) return PFAC_STATUS_INVALID_PARAMETER;
    if (size > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    const PinnedPairs scan(handle, h_input, size, h_spanStart, h_spanLen);                          /* ids, positions: in position order */
    if (scan.status != PFAC_STATUS_SUCCESS) return scan.status;
    size_t j = 0;
    mergeSpans([&](size_t &p, size_t &e) {
        if (j >= (size_t)scan.count) return false;
        p = (size_t)h_spanLen[j];
        e = p + patternLenOf(handle->fa, h_spanStart[j]);
        j++;
        return true;
    }, h_spanStart, h_spanLen, h_numSpans, h_coveredBytes);
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_redactSpansFromDevice(PFAC_handle_t handle, const char *d_input, size_t size, const int *d_spanStart, const int *d_spanLen,
                                          size_t numSpans, unsigned char fill, char *d_out)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (size == 0) return PFAC_STATUS_SUCCESS;
    if (!d_input || !d_out || (numSpans && (!d_spanStart || !d_spanLen))) return PFAC_STATUS_INVALID_PARAMETER;
    if (size > kMaxInt || numSpans > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    const uintptr_t I = reinterpret_cast<uintptr_t>(d_input), O = reinterpret_cast<uintptr_t>(d_out);
    if (I != O && I < O + size && O < I + size) return PFAC_STATUS_INVALID_PARAMETER;        /* in place, or apart */
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(handle->lock);
    return handle->spans_redact_ptr(handle, d_input, size, d_spanStart, d_spanLen, numSpans, fill, d_out);
}

} /* extern "C" */
