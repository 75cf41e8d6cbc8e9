/*
 * capture_api.cpp -- PFACX_capturePairsFromDevice / ...FromHost, PFACX_matchCapturedFromDevice / ...FromHost (include/pfac_ext.h): the value behind
 * every match -- from the end of the match over the bytes of a skip class to the first byte of a stop class, inside a window.
 *
 * The six rules of the header are captureOnHost below, word for word.  The device forms are the passes of scan_capture.hip (PFACX_captureRun) over
 * the handle's capture scratch (pfac::DeviceScratch::capture: counted by PFACX_getInfo, freed by PFACX_trim with every other scratch buffer) and,
 * without PFACX_CAPTURE_AT_POS, the device copy of the pattern lengths (ensurePatternLen: shared with the batch and spans calls).  The host forms are
 * the loop below on every platform: one forward walk per pair, memchr for a stop class of one byte.  The scan forms are the compacted-output call
 * (PFAC_matchFromDeviceReduce; on the host hostLongestPairs) with the captured pairs behind it.  Nothing folds the classes: they are tested on the
 * caller's bytes.  S \ D is computed here, once, for both forms.
 */
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstring>
#include <mutex>

#include "pfac_host.h"

namespace pfac_internal {

/* the classes of a call as both forms use them: stop = D (null: {'\n'}), skip = S \ D (null S: empty) */
struct CaptureClasses {
    const ByteClass stop;
    unsigned int skip[8];
    CaptureClasses(const unsigned int *h_skip, const unsigned int *h_stop) : stop(h_stop)
    {
        for (int k = 0; k < 8; k++) skip[k] = h_skip ? h_skip[k] & ~stop.words[k] : 0u;
    }
};

/* what both pairs forms check first */
static PFAC_status_t checkCaptureArgs(PFAC_handle_t handle, const void *input, size_t size, unsigned int flags, const int *ids, const int *pos,
                                      size_t numPairs, const int *valStart, const int *valLen)
{
    if (!handle || !input || (flags & ~PFACX_CAPTURE_AT_POS) || size > kMaxInt || numPairs > kMaxInt ||
        (numPairs && (!pos || !valStart || !valLen || (!ids && !(flags & PFACX_CAPTURE_AT_POS)))))
        return PFAC_STATUS_INVALID_PARAMETER;
    return PFAC_STATUS_SUCCESS;
}

/* The host loop over in[0, n), 0 < n < 2^31: the rules 1 to 6 of the header for the pairs [0, numPairs).  lens: the F + 1 pattern lengths by id
 * (not read with PFACX_CAPTURE_AT_POS, ids neither).  A pair is only ever read, a position only used as an index once it lies inside [0, n) */
static void captureOnHost(const unsigned char *in, size_t n, const CaptureClasses &cls, size_t window, unsigned int flags, const int *lens, size_t F,
                          const int *ids, const int *pos, size_t numPairs, int *valStart, int *valLen)
{
    const bool atPos = (flags & PFACX_CAPTURE_AT_POS) != 0;
    for (size_t k = 0; k < numPairs; k++) {
        const int p = pos[k];
        size_t len = 0;
        bool inside = p >= 0 && (size_t)p < n;
        if (inside && !atPos) {
            const int id = ids[k];
            inside = id >= 1 && (size_t)id <= F;
            if (inside && lens[id] > 0) len = (size_t)lens[id];
        }
        if (!inside) {
            valStart[k] = -1;
            valLen[k] = 0;
            continue;
        }
        const size_t b = (size_t)p + len < n ? (size_t)p + len : n;
        const size_t w = window == 0 || window >= n - b ? n : b + window;
        size_t s = b;
        while (s < w && inClass(cls.skip, in[s])) s++;
        size_t e = s;
        if (cls.stop.members == 1) {
            const void *hit = s < w ? std::memchr(in + s, (int)cls.stop.only, w - s) : nullptr;
            e = hit ? (size_t)(static_cast<const unsigned char *>(hit) - in) : w;
        } else {
            while (e < w && !inClass(cls.stop.words, in[e])) e++;
        }
        valStart[k] = (int)s;
        valLen[k] = (int)(e - s);
    }
}

/* the device passes over a list (the caller holds the lock and has checked the module): the pattern lengths where the call reads them */
static PFAC_status_t captureOnDevice(PFAC_context *c, const char *d_input, size_t size, const CaptureClasses &cls, size_t window, unsigned int flags,
                                     const int *d_ids, const int *d_pos, size_t numPairs, int *d_valStart, int *d_valLen)
{
    PFACX_captureRun_t run{};
    run.d_input = d_input;
    run.size = size;
    for (int k = 0; k < 8; k++) run.skip[k] = cls.skip[k];
    cls.stop.copyTo(run.stop);
    run.window = window;
    run.flags = flags;
    run.d_pos = d_pos;
    run.numPairs = numPairs;
    run.d_valStart = d_valStart;
    run.d_valLen = d_valLen;
    if (!(flags & PFACX_CAPTURE_AT_POS)) {
        if (!c->isPatternsReady) return PFAC_STATUS_PATTERNS_NOT_READY;
        const PFAC_status_t st = ensurePatternLen(c);
        if (st != PFAC_STATUS_SUCCESS) return st;
        run.d_ids = d_ids;
        run.d_patternLen = c->scratch.patternLen.get();
        run.numLens = c->scratch.patternLen.count();
    }
    size_t slowPairs = 0;
    return c->capture_run_ptr(c, &run, &slowPairs);
}

/* what both scan forms check of their own arguments (pfac_host.h: scanForm) */
static bool matchCapturedArgsOk(const int *valStart, const int *valLen, size_t capCapacity, unsigned int flags)
{
    return !(capCapacity && (!valStart || !valLen)) && !(flags & ~PFACX_CAPTURE_AT_POS);
}

} // namespace pfac_internal
using namespace pfac_internal;

extern "C" {

PFAC_status_t PFACX_capturePairsFromDevice(PFAC_handle_t handle, const char *d_input, size_t size, const unsigned int *h_skip, const unsigned int *h_stop,
                                           size_t window, unsigned int flags, const int *d_ids, const int *d_pos, size_t numPairs, int *d_valStart,
                                           int *d_valLen)
{
    const PFAC_status_t st = checkCaptureArgs(handle, d_input, size, flags, d_ids, d_pos, numPairs, d_valStart, d_valLen);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0 || numPairs == 0) return PFAC_STATUS_SUCCESS;
    if (!(flags & PFACX_CAPTURE_AT_POS) && SetPin(handle).status() != PFAC_STATUS_SUCCESS) return PFAC_STATUS_PATTERNS_NOT_READY;
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    const CaptureClasses cls(h_skip, h_stop);
    std::lock_guard<std::mutex> guard(handle->lock);
    return captureOnDevice(handle, d_input, size, cls, window, flags, d_ids, d_pos, numPairs, d_valStart, d_valLen);
}

PFAC_status_t PFACX_capturePairsFromHost(PFAC_handle_t handle, const char *h_input, size_t size, const unsigned int *h_skip, const unsigned int *h_stop,
                                         size_t window, unsigned int flags, const int *h_ids, const int *h_pos, size_t numPairs, int *h_valStart,
                                         int *h_valLen)
{
    const PFAC_status_t st = checkCaptureArgs(handle, h_input, size, flags, h_ids, h_pos, numPairs, h_valStart, h_valLen);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0 || numPairs == 0) return PFAC_STATUS_SUCCESS;
    const CaptureClasses cls(h_skip, h_stop);
    std::lock_guard<std::mutex> guard(handle->lock);
    const bool atPos = (flags & PFACX_CAPTURE_AT_POS) != 0;
    if (!atPos && !handle->isPatternsReady) return PFAC_STATUS_PATTERNS_NOT_READY;
    const size_t F = atPos ? 0 : (handle->fa.patternLen.empty() ? 0 : handle->fa.patternLen.size() - 1);
    captureOnHost(reinterpret_cast<const unsigned char *>(h_input), size, cls, window, flags, atPos ? nullptr : handle->fa.patternLen.data(), F, h_ids,
                  h_pos, numPairs, h_valStart, h_valLen);
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_matchCapturedFromDevice(PFAC_handle_t handle, char *d_input, size_t size, const unsigned int *h_skip, const unsigned int *h_stop,
                                            size_t window, unsigned int flags, int *d_ids, int *d_pos, int *d_valStart, int *d_valLen, size_t capCapacity,
                                            int *h_num_matched)
{
    return scanForm<DevicePairs>(handle, d_input, size, d_ids, d_pos, matchCapturedArgsOk(d_valStart, d_valLen, capCapacity, flags), capCapacity, h_num_matched,
                          [&](size_t captured) {
                              return captureOnDevice(handle, d_input, size, CaptureClasses(h_skip, h_stop), window, flags, d_ids, d_pos, captured,
                                                     d_valStart, d_valLen);
                          });
}

PFAC_status_t PFACX_matchCapturedFromHost(PFAC_handle_t handle, char *h_input, size_t size, const unsigned int *h_skip, const unsigned int *h_stop,
                                          size_t window, unsigned int flags, int *h_ids, int *h_pos, int *h_valStart, int *h_valLen, size_t capCapacity,
                                          int *h_num_matched)
{
    return scanForm<PinnedPairs>(handle, h_input, size, h_ids, h_pos, matchCapturedArgsOk(h_valStart, h_valLen, capCapacity, flags), capCapacity, h_num_matched,
                        [&](size_t captured) {                             /* under the pin: the lengths are read from the set the pairs came from */
                            const pfac::Automaton &fa = handle->fa;
                            captureOnHost(reinterpret_cast<const unsigned char *>(h_input), size, CaptureClasses(h_skip, h_stop), window, flags,
                                          fa.patternLen.data(), fa.patternLen.empty() ? 0 : fa.patternLen.size() - 1, h_ids, h_pos, captured,
                                          h_valStart, h_valLen);
                            return PFAC_STATUS_SUCCESS;
                        });
}

} /* extern "C" */
