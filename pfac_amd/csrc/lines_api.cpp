/*
 * lines_api.cpp -- PFACX_matchLinesFromDevice / ...FromHost / PFACX_gatherLinesFromDevice (include/pfac_ext.h): the lines of a buffer that
 * contain a pattern (PFACX_LINES_INVERT: that contain none), grep -F -f.
 *
 * No pattern contains '\n', so the longest-match result of the whole buffer is exact per line.  The device form is the compacted scan with a
 * line index in front of it and a mark / select pass behind it (scan_lines.hip: PFACX_linesSelect); the host form takes the longest pairs from
 * hostLongestPairs and does the line work here: memchr for the line ends, one bit per line for the hits (one walk over lines and pairs together),
 * then the list, written in place over the arrays the pairs were in (the bits are complete by then).
 */
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <mutex>
#include <vector>

#include "pfac_host.h"

namespace pfac_internal {

/* f(k, start, end) for every line k of in[0, n): its bytes are [start, end), end == n for an unterminated last line.  Returns the number of lines */
template <class F>
static size_t forEachLine(const char *in, size_t n, F f)
{
    size_t k = 0, s = 0;
    while (s < n) {
        const void *q = std::memchr(in + s, '\n', n - s);
        const size_t e = q ? (size_t)(static_cast<const char *>(q) - in) : n;
        f(k, s, e);
        k++;
        s = e + 1;
    }
    return k;
}

/* the selected lines of in[0, n) from one bit per line, into arrays that may be the ones the bits were made from */
static void listLines(const char *in, size_t n, const std::vector<uint64_t> &hit, bool invert, int *lineStart, int *lineLen, int *lineIndex,
                      size_t *numLines, size_t *numSelected)
{
    size_t o = 0;
    *numLines = forEachLine(in, n, [&](size_t k, size_t s, size_t e) {
        if ((((hit[k >> 6] >> (k & 63)) & 1u) != 0) == invert) return;
        lineStart[o] = (int)s;
        lineLen[o] = (int)(e - s);
        if (lineIndex) lineIndex[o] = (int)k;
        o++;
    });
    *numSelected = o;
}

static PFAC_status_t checkLinesArgs(PFAC_handle_t handle, const char *input, unsigned int flags, const int *lineStart, const int *lineLen,
                                    const size_t *h_numLines, const size_t *h_numSelected)
{
    const PFAC_status_t st = checkSetAndPointers(handle, {input, lineStart, lineLen, h_numLines, h_numSelected});
    return st == PFAC_STATUS_SUCCESS && (flags & ~PFACX_LINES_INVERT) ? PFAC_STATUS_INVALID_PARAMETER : st;
}

} // namespace pfac_internal
using namespace pfac_internal;

extern "C" {

PFAC_status_t PFACX_matchLinesFromDevice(PFAC_handle_t handle, char *d_input, size_t size, unsigned int flags, int *d_lineStart, int *d_lineLen,
                                         int *d_lineIndex, size_t capacity, size_t *h_numLines, size_t *h_numSelected)
{
    PFAC_status_t st = checkLinesArgs(handle, d_input, flags, d_lineStart, d_lineLen, h_numLines, h_numSelected);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0) { *h_numLines = 0; *h_numSelected = 0; return PFAC_STATUS_SUCCESS; }
    if (capacity < size) return PFAC_STATUS_INVALID_PARAMETER;
    if (size > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(handle->lock);
    DeviceScan scan;                                                       /* a caseless set: the scan reads the folded copy, the line ends are the caller's */
    st = beginDeviceScan(handle, d_input, size, &scan);
    if (st != PFAC_STATUS_SUCCESS) return st;
    return handle->lines_select_ptr(handle, d_input, scan.d_scan, size, (flags & PFACX_LINES_INVERT) ? 1 : 0, scan.hashed, d_lineStart, d_lineLen,
                                    d_lineIndex, h_numLines, h_numSelected);
}

PFAC_status_t PFACX_matchLinesFromHost(PFAC_handle_t handle, char *h_input, size_t size, unsigned int flags, int *h_lineStart, int *h_lineLen,
                                       int *h_lineIndex, size_t capacity, size_t *h_numLines, size_t *h_numSelected)
{
    PFAC_status_t st = checkLinesArgs(handle, h_input, flags, h_lineStart, h_lineLen, h_numLines, h_numSelected);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0) { *h_numLines = 0; *h_numSelected = 0; return PFAC_STATUS_SUCCESS; }
    if (capacity < size) return PFAC_STATUS_INVALID_PARAMETER;
    if (size > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    const bool invert = (flags & PFACX_LINES_INVERT) != 0;
    std::vector<uint64_t> hit;
    try {
        hit.assign(size / 64 + 1, 0);                                     /* numLines <= size */
    } catch (const std::bad_alloc &) {
        return PFAC_STATUS_ALLOC_FAILED;
    }
    int count = 0;
    st = hostLongestPairs(handle, h_input, size, h_lineStart, h_lineLen, &count, nullptr);      /* ids, positions: in position order */
    if (st != PFAC_STATUS_SUCCESS) return st;
    size_t j = 0;                                                         /* one walk over lines and positions together */
    forEachLine(h_input, size, [&](size_t k, size_t, size_t e) {
        if (j < (size_t)count && (size_t)h_lineLen[j] < e) hit[k >> 6] |= uint64_t(1) << (k & 63);
        while (j < (size_t)count && (size_t)h_lineLen[j] < e) j++;
    });
    listLines(h_input, size, hit, invert, h_lineStart, h_lineLen, h_lineIndex, h_numLines, h_numSelected);
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_gatherLinesFromDevice(PFAC_handle_t handle, const char *d_input, size_t size, const int *d_lineStart, const int *d_lineLen,
                                          size_t numSelected, char *d_out, size_t outCapacity, size_t *h_outBytes)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!h_outBytes) return PFAC_STATUS_INVALID_PARAMETER;
    if (numSelected == 0) { *h_outBytes = 0; return PFAC_STATUS_SUCCESS; }
    if (!d_lineStart || !d_lineLen || (!d_input && size) || (!d_out && outCapacity)) return PFAC_STATUS_INVALID_PARAMETER;
    if (size > kMaxInt || numSelected > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(handle->lock);
    return handle->lines_gather_ptr(handle, d_input, size, d_lineStart, d_lineLen, numSelected, d_out, outCapacity, h_outBytes);
}

} /* extern "C" */
