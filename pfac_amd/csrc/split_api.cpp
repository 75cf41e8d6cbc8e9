/*
 * split_api.cpp -- PFACX_splitFromDevice / ...FromHost (include/pfac_ext.h): the offsets that cut a buffer into records at the bytes of a class --
 * what the batch, rules, count-batch and groups calls take as d_offsets, made where the text lies.
 *
 * Position c of [1, n - 1] is a cut by its own byte and the byte in front of it (the four flag combinations: pfac_host.h isCut).  The device form is the
 * passes of scan_split.hip (PFACX_splitRun) over the handle's split scratch (pfac::DeviceScratch::split: counted by PFACX_getInfo, freed by
 * PFACX_trim with every other scratch buffer).  The host form is the loop below on every platform; a class of one byte finds its delimiters with
 * memchr.  Neither needs a pattern set, neither folds: the class is tested on the caller's bytes.
 */
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstring>
#include <mutex>

#include "pfac_host.h"

namespace pfac_internal {

/* what both calls check first */
static PFAC_status_t checkSplitArgs(PFAC_handle_t handle, const void *input, unsigned int flags, const size_t *offsets, size_t capacity,
                                    const size_t *h_numSegments)
{
    if (!handle || !input || !h_numSegments || (flags & ~(PFACX_SPLIT_BEFORE | PFACX_SPLIT_RUNS)) || (capacity && !offsets) ||
        (reinterpret_cast<uintptr_t>(offsets) & 7u) || capacity > SIZE_MAX / sizeof(size_t))
        return PFAC_STATUS_INVALID_PARAMETER;
    return PFAC_STATUS_SUCCESS;
}

/* The offsets of in[0, n), n > 0, into offsets[0, capacity): 0, the cuts, n -- nothing at or behind capacity; returns the number of segments,
 * *longest = the longest of them */
static size_t splitOnHost(const unsigned char *in, size_t n, const ByteClass &d, unsigned int flags, size_t *offsets, size_t capacity,
                          size_t *longest)
{
    const bool before = (flags & PFACX_SPLIT_BEFORE) != 0, runs = (flags & PFACX_SPLIT_RUNS) != 0;
    size_t cuts = 0, last = 0, most = 0;
    const auto cut = [&](size_t c) {                                       /* ascending, inside (0, n) */
        if (cuts + 1 < capacity) offsets[cuts + 1] = c;
        if (c - last > most) most = c - last;
        last = c;
        cuts++;
    };
    const unsigned int *const cls = d.words, only = d.only;
    if (d.members == 1) {
        /* the delimiters by memchr; a run [p, e) of them cuts once under RUNS: in front of it, or behind it */
        for (size_t p = 0; p < n;) {
            const void *hit = std::memchr(in + p, (int)only, n - p);
            if (!hit) break;
            p = (size_t)(static_cast<const unsigned char *>(hit) - in);
            size_t e = p + 1;
            if (runs)
                while (e < n && in[e] == only) e++;
            const size_t c = before ? p : e;
            if (c > 0 && c < n) cut(c);
            p = e;
        }
    } else if (d.members != 0) {
        bool a = inClass(cls, in[0]);                                      /* the byte in front of c is a delimiter */
        for (size_t c = 1; c < n; c++) {
            const bool b = inClass(cls, in[c]);
            if (isCut(flags, a, b)) cut(c);
            a = b;
        }
    }
    if (n - last > most) most = n - last;
    if (capacity > 0) offsets[0] = 0;
    if (cuts + 1 < capacity) offsets[cuts + 1] = n;
    *longest = most;
    return cuts + 1;
}

} // namespace pfac_internal
using namespace pfac_internal;

extern "C" {

PFAC_status_t PFACX_splitFromDevice(PFAC_handle_t handle, const char *d_input, size_t size, const unsigned int *h_class, unsigned int flags,
                                    size_t *d_offsets, size_t capacity, size_t *h_numSegments, size_t *h_longest)
{
    const PFAC_status_t st = checkSplitArgs(handle, d_input, flags, d_offsets, capacity, h_numSegments);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0) {
        *h_numSegments = 0;
        if (h_longest) *h_longest = 0;
        return PFAC_STATUS_SUCCESS;
    }
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(handle->lock);
    PFACX_splitRun_t run{d_input, size, {}, flags, d_offsets, capacity};
    ByteClass(h_class).copyTo(run.cls);
    size_t segments = 0, longest = 0;
    const PFAC_status_t ran = handle->split_run_ptr(handle, &run, &segments, &longest);
    if (ran != PFAC_STATUS_SUCCESS) return ran;
    *h_numSegments = segments;
    if (h_longest) *h_longest = longest;
    return truncatedIf((unsigned long long)segments + 1, capacity);
}

PFAC_status_t PFACX_splitFromHost(PFAC_handle_t handle, const char *h_input, size_t size, const unsigned int *h_class, unsigned int flags,
                                  size_t *h_offsets, size_t capacity, size_t *h_numSegments, size_t *h_longest)
{
    const PFAC_status_t st = checkSplitArgs(handle, h_input, flags, h_offsets, capacity, h_numSegments);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0) {
        *h_numSegments = 0;
        if (h_longest) *h_longest = 0;
        return PFAC_STATUS_SUCCESS;
    }
    const ByteClass cls(h_class);
    std::lock_guard<std::mutex> guard(handle->lock);
    size_t longest = 0;
    const size_t segments = splitOnHost(reinterpret_cast<const unsigned char *>(h_input), size, cls, flags, h_offsets, capacity, &longest);
    *h_numSegments = segments;
    if (h_longest) *h_longest = longest;
    return truncatedIf((unsigned long long)segments + 1, capacity);
}

} /* extern "C" */
