/*
 * disjoint_api.cpp -- PFACX_matchDisjointFromDevice / ...FromHost, PFACX_replaceFromDevice / ...FromHost (include/pfac_ext.h): the input tokenised
 * into matches that do not overlap (leftmost, then longest), and the text with every token substituted by the string of its pattern.
 *
 * The device forms are the compacted scan with its ordering launches and passes over the pairs behind it, and passes over the tokens and one over the
 * output (scan_disjoint.hip: PFACX_disjointSelect, PFACX_replaceRun).  The host form of the selection takes the longest pairs from hostLongestPairs
 * and runs the loop of the definition over them, the list written in place over the arrays the pairs are in (token k comes from pair >= k); the host
 * form of the replacement is one sequential loop of memcpy, whatever the platform.
 */
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <mutex>

#include "pfac_host.h"

namespace pfac_internal {

static bool replOffFits(const pfac::Automaton &fa, size_t numOff) { return numOff >= (size_t)fa.numPatterns + 2; }   /* two offsets for every id of the set, which the caller holds still */

/* what both forms of the replacement refuse; *done: the call has its answer (size == 0) */
static PFAC_status_t checkReplaceArgs(PFAC_handle_t handle, const char *input, size_t size, const int *ids, const int *pos, size_t numTokens,
                                      const int *replOff, size_t numOff, const char *replBytesAt, size_t replBytes, const char *out, size_t outCapacity,
                                      size_t *h_outBytes, bool *done)
{
    *done = false;
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    const SetPin pin(handle);
    if (pin.status() != PFAC_STATUS_SUCCESS) return pin.status();
    if (!h_outBytes) return PFAC_STATUS_INVALID_PARAMETER;
    if (size == 0) { *h_outBytes = 0; *done = true; return PFAC_STATUS_SUCCESS; }
    if (!input || (!out && outCapacity)) return PFAC_STATUS_INVALID_PARAMETER;
    if (size > kMaxInt || numTokens > kMaxInt || replBytes > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    if (numTokens) {
        if (!ids || !pos || !replOff || (!replBytesAt && replBytes)) return PFAC_STATUS_INVALID_PARAMETER;
        if (!replOffFits(handle->fa, numOff)) return PFAC_STATUS_INVALID_PARAMETER;
    }
    const uintptr_t I = reinterpret_cast<uintptr_t>(input), O = reinterpret_cast<uintptr_t>(out);
    if (outCapacity && I < O + outCapacity && O < I + size) return PFAC_STATUS_INVALID_PARAMETER;      /* a text whose length changes has no in-place form */
    return PFAC_STATUS_SUCCESS;
}

} // namespace pfac_internal
using namespace pfac_internal;

extern "C" {

PFAC_status_t PFACX_matchDisjointFromDevice(PFAC_handle_t handle, char *d_input, size_t size, int *d_ids, int *d_pos, size_t capacity,
                                            size_t *h_numTokens, size_t *h_coveredBytes)
{
    PFAC_status_t st = checkSetAndPointers(handle, {d_input, d_ids, d_pos, h_numTokens, h_coveredBytes});
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0) { *h_numTokens = 0; *h_coveredBytes = 0; return PFAC_STATUS_SUCCESS; }
    if (capacity < size) return PFAC_STATUS_INVALID_PARAMETER;
    if (size > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(handle->lock);
    st = ensurePatternLen(handle);
    if (st != PFAC_STATUS_SUCCESS) return st;
    DeviceScan scan;                                                       /* a caseless set: the scan reads the folded copy */
    st = beginDeviceScan(handle, d_input, size, &scan);
    if (st != PFAC_STATUS_SUCCESS) return st;
    return handle->disjoint_select_ptr(handle, scan.d_scan, size, scan.hashed, handle->scratch.patternLen.get(), handle->scratch.patternLen.count(),
                                       d_ids, d_pos, h_numTokens, h_coveredBytes);
}

PFAC_status_t PFACX_matchDisjointFromHost(PFAC_handle_t handle, char *h_input, size_t size, int *h_ids, int *h_pos, size_t capacity,
                                          size_t *h_numTokens, size_t *h_coveredBytes)
{
    PFAC_status_t st = checkSetAndPointers(handle, {h_input, h_ids, h_pos, h_numTokens, h_coveredBytes});
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0) { *h_numTokens = 0; *h_coveredBytes = 0; return PFAC_STATUS_SUCCESS; }
    if (capacity < size) return PFAC_STATUS_INVALID_PARAMETER;
    if (size > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    const PinnedPairs scan(handle, h_input, size, h_ids, h_pos);                       /* in position order */
    if (scan.status != PFAC_STATUS_SUCCESS) return scan.status;
    size_t o = 0, covered = 0, end = 0;                                               /* end: where the last taken match ended */
    for (size_t j = 0; j < (size_t)scan.count; j++) {
        const size_t p = (size_t)h_pos[j];
        if (p < end) continue;                                                         /* starts inside a taken match */
        const int id = h_ids[j];
        const size_t len = patternLenOf(handle->fa, id);
        h_ids[o] = id;
        h_pos[o] = (int)p;
        o++;
        end = p + len;
        covered += len;
    }
    *h_numTokens = o;
    *h_coveredBytes = covered;
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_replaceFromDevice(PFAC_handle_t handle, const char *d_input, size_t size, const int *d_ids, const int *d_pos, size_t numTokens,
                                      const int *d_replOff, size_t numOff, const char *d_replBytes, size_t replBytes, char *d_out, size_t outCapacity,
                                      size_t *h_outBytes)
{
    bool done = false;
    PFAC_status_t st = checkReplaceArgs(handle, d_input, size, d_ids, d_pos, numTokens, d_replOff, numOff, d_replBytes, replBytes, d_out, outCapacity,
                                        h_outBytes, &done);
    if (st != PFAC_STATUS_SUCCESS || done) return st;
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(handle->lock);
    if (numTokens == 0) {                                                              /* a plain copy */
        const size_t bytes = size < outCapacity ? size : outCapacity;
        if (bytes && hipMemcpy(d_out, d_input, bytes, hipMemcpyDeviceToDevice) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
        if (hipStreamSynchronize(0) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
        *h_outBytes = size;
        return truncatedIf(size, outCapacity);
    }
    st = ensurePatternLen(handle);
    if (st != PFAC_STATUS_SUCCESS) return st;
    return handle->replace_run_ptr(handle, d_input, size, d_ids, d_pos, numTokens, handle->scratch.patternLen.get(), handle->scratch.patternLen.count(),
                                   d_replOff, numOff, d_replBytes, replBytes, d_out, outCapacity, h_outBytes);
}

PFAC_status_t PFACX_replaceFromHost(PFAC_handle_t handle, const char *h_input, size_t size, const int *h_ids, const int *h_pos, size_t numTokens,
                                    const int *h_replOff, size_t numOff, const char *h_replBytes, size_t replBytes, char *h_out, size_t outCapacity,
                                    size_t *h_outBytes)
{
    bool done = false;
    const PFAC_status_t st = checkReplaceArgs(handle, h_input, size, h_ids, h_pos, numTokens, h_replOff, numOff, h_replBytes, replBytes, h_out,
                                              outCapacity, h_outBytes, &done);
    if (st != PFAC_STATUS_SUCCESS || done) return st;
    const SetPin pin(handle);                                                          /* no scan: the lengths of whichever set is loaded, held still under the loop */
    if (pin.status() != PFAC_STATUS_SUCCESS) return pin.status();
    if (numTokens && !replOffFits(handle->fa, numOff)) return PFAC_STATUS_INVALID_PARAMETER;   /* ... which need not be the one checkReplaceArgs saw */
    const std::vector<int> &patternLen = handle->fa.patternLen;
    const size_t numIds = patternLen.size();                                           /* F + 1 <= numOff - 1: every id with a length has two offsets */
    unsigned long long w = 0;                                                          /* bytes of the text so far */
    auto put = [&](const char *src, size_t len) {                                      /* ... of which only those below outCapacity are written */
        if (w < outCapacity && len) std::memcpy(h_out + w, src, len < outCapacity - w ? len : (size_t)(outCapacity - w));
        w += len;
    };
    auto clampTo = [](int v, size_t top) -> size_t { return v < 0 ? 0 : ((size_t)v > top ? top : (size_t)v); };
    size_t cur = 0;                                                                    /* input bytes in front of this are done with */
    for (size_t k = 0; k < numTokens; k++) {
        const int id = h_ids[k];
        const size_t s = clampTo(h_pos[k], size);
        if (s > cur) { put(h_input + cur, s - cur); cur = s; }                         /* the gap */
        if (id < 1 || (size_t)id >= numIds) continue;                                  /* does nothing */
        const size_t len = clampTo(patternLen[id], size - s);
        const size_t o0 = clampTo(h_replOff[id], replBytes), o1 = clampTo(h_replOff[id + 1], replBytes);
        if (o1 > o0) put(h_replBytes + o0, o1 - o0);
        if (s + len > cur) cur = s + len;
    }
    if (size > cur) put(h_input + cur, size - cur);
    *h_outBytes = (size_t)w;
    return truncatedIf(w, outCapacity);
}

} /* extern "C" */
