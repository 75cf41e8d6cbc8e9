/*
 * lines_api.cpp -- PFACX_matchLinesFromDevice / ...FromHost / PFACX_gatherLinesFromDevice (include/pfac_ext.h): the lines of a buffer that
 * contain a pattern (PFACX_LINES_INVERT: that contain none), grep -F -f.
 *
 * No pattern contains '\n', so the longest-match result of the whole buffer is exact per line.  The device form is the compacted scan with a
 * line index in front of it and a mark / select pass behind it (scan_lines.hip: PFACX_linesSelect); the host form takes the longest pairs from
 * hostLongestPairs and does the line work here: memchr for the line ends, one bit per line for the hits (one walk over lines and pairs together),
 * then the list, written in place over the arrays the pairs were in (the bits are complete by then).
 * PFACX_matchLinesContext* (grep -A / -B / -C) are the same two with the selected lines widened: on the device by the context stage of
 * PFACX_linesSelectContext, on the host by one forward and one backward pass over the line bits into a second bit per line.
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

/* one bit per line of in[0, n) that holds a match, into the zeroed `hit`: the longest pairs from hostLongestPairs -- ids and pos, `n` entries each,
 * are its room -- and one walk over lines and positions together.  *numLines where given */
static PFAC_status_t hostHitBits(PFAC_handle_t handle, char *in, size_t n, int *ids, int *pos, std::vector<uint64_t> &hit, size_t *numLines)
{
    int count = 0;
    const PFAC_status_t st = hostLongestPairs(handle, in, n, ids, pos, &count, nullptr);      /* ids, positions: in position order */
    if (st != PFAC_STATUS_SUCCESS) return st;
    size_t j = 0;
    const size_t lines = forEachLine(in, n, [&](size_t k, size_t, size_t e) {
        if (j < (size_t)count && (size_t)pos[j] < e) hit[k >> 6] |= uint64_t(1) << (k & 63);
        while (j < (size_t)count && (size_t)pos[j] < e) j++;
    });
    if (numLines) *numLines = lines;
    return PFAC_STATUS_SUCCESS;
}

static PFAC_status_t checkContextArgs(PFAC_handle_t handle, const char *input, unsigned int flags, const int *lineStart, const int *lineLen,
                                      const size_t *h_numLines, const size_t *h_numSelected, const size_t *h_numMatching, const size_t *h_numGroups)
{
    const PFAC_status_t st = checkSetAndPointers(handle, {input, lineStart, lineLen, h_numLines, h_numSelected, h_numMatching, h_numGroups});
    return st == PFAC_STATUS_SUCCESS && (flags & ~PFACX_LINES_INVERT) ? PFAC_STATUS_INVALID_PARAMETER : st;
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
    st = hostHitBits(handle, h_input, size, h_lineStart, h_lineLen, hit, nullptr);
    if (st != PFAC_STATUS_SUCCESS) return st;
    listLines(h_input, size, hit, invert, h_lineStart, h_lineLen, h_lineIndex, h_numLines, h_numSelected);
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_matchLinesContextFromDevice(PFAC_handle_t handle, char *d_input, size_t size, unsigned int flags, unsigned int before,
                                                unsigned int after, int *d_lineStart, int *d_lineLen, int *d_lineIndex, int *d_lineTag, size_t capacity,
                                                size_t *h_numLines, size_t *h_numSelected, size_t *h_numMatching, size_t *h_numGroups)
{
    PFAC_status_t st = checkContextArgs(handle, d_input, flags, d_lineStart, d_lineLen, h_numLines, h_numSelected, h_numMatching, h_numGroups);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0) { *h_numLines = *h_numSelected = *h_numMatching = *h_numGroups = 0; return PFAC_STATUS_SUCCESS; }
    if (capacity < size) return PFAC_STATUS_INVALID_PARAMETER;
    if (size > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(handle->lock);
    DeviceScan scan;
    st = beginDeviceScan(handle, d_input, size, &scan);
    if (st != PFAC_STATUS_SUCCESS) return st;
    return handle->lines_select_context_ptr(handle, d_input, scan.d_scan, size, (flags & PFACX_LINES_INVERT) ? 1 : 0, scan.hashed, before, after,
                                            d_lineStart, d_lineLen, d_lineIndex, d_lineTag, h_numLines, h_numSelected, h_numMatching, h_numGroups);
}

PFAC_status_t PFACX_matchLinesContextFromHost(PFAC_handle_t handle, char *h_input, size_t size, unsigned int flags, unsigned int before,
                                              unsigned int after, int *h_lineStart, int *h_lineLen, int *h_lineIndex, int *h_lineTag, size_t capacity,
                                              size_t *h_numLines, size_t *h_numSelected, size_t *h_numMatching, size_t *h_numGroups)
{
    PFAC_status_t st = checkContextArgs(handle, h_input, flags, h_lineStart, h_lineLen, h_numLines, h_numSelected, h_numMatching, h_numGroups);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0) { *h_numLines = *h_numSelected = *h_numMatching = *h_numGroups = 0; return PFAC_STATUS_SUCCESS; }
    if (capacity < size) return PFAC_STATUS_INVALID_PARAMETER;
    if (size > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    std::vector<uint64_t> member, selected;                               /* two bits per possible line */
    try {
        member.assign(size / 64 + 1, 0);
        selected.assign(size / 64 + 1, 0);
    } catch (const std::bad_alloc &) {
        return PFAC_STATUS_ALLOC_FAILED;
    }
    size_t numLines = 0;
    st = hostHitBits(handle, h_input, size, h_lineStart, h_lineLen, member, &numLines);
    if (st != PFAC_STATUS_SUCCESS) return st;
    const auto bit = [](const std::vector<uint64_t> &v, size_t k) { return ((v[k >> 6] >> (k & 63)) & 1u) != 0; };
    size_t matching = 0;
    if (flags & PFACX_LINES_INVERT)                                       /* H: the lines that do not match, and no bit behind the last line */
        for (size_t k = 0; k < numLines; k++) member[k >> 6] ^= uint64_t(1) << (k & 63);
    /* forward: the lines at most `after` behind the last member seen; backward: those at most `before` in front of the next */
    bool seen = false;
    for (size_t k = 0, last = 0; k < numLines; k++) {
        if (bit(member, k)) { seen = true; last = k; matching++; }
        if (seen && k - last <= after) selected[k >> 6] |= uint64_t(1) << (k & 63);
    }
    seen = false;
    for (size_t k = numLines, next = 0; k-- > 0;) {
        if (bit(member, k)) { seen = true; next = k; }
        if (seen && next - k <= before) selected[k >> 6] |= uint64_t(1) << (k & 63);
    }
    /* the list, in place over the arrays the pairs were in (the bits are complete) */
    size_t o = 0, groups = 0;
    bool behind = false;                                                  /* the line in front is selected */
    forEachLine(h_input, size, [&](size_t k, size_t s, size_t e) {
        const bool sel = bit(selected, k);
        if (sel) {
            if (!behind) groups++;
            h_lineStart[o] = (int)s;
            h_lineLen[o] = (int)(e - s);
            if (h_lineIndex) h_lineIndex[o] = (int)k;
            if (h_lineTag) h_lineTag[o] = (int)(((groups - 1) << 1) | (bit(member, k) ? 1u : 0u));
            o++;
        }
        behind = sel;
    });
    *h_numLines = numLines;
    *h_numSelected = o;
    *h_numMatching = matching;
    *h_numGroups = groups;
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
