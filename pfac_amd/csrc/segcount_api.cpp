/*
 * segcount_api.cpp -- PFACX_countBatchFromDevice / ...FromHost / PFACX_countBatchPairsFromDevice (include/pfac_ext.h): how often each pattern
 * occurred in each segment of a batch, as (id, count) entries in CSR form.
 *
 * Every pattern that occurs at a position is a prefix of the longest one there, so all three forms work on longest pairs.  The device form takes
 * the ordered pairs of the batch in the handle's pair scratch from scratchBatchPairs (batch_api.cpp) and runs PFACX_segCountRun (scan_segcount.hip)
 * over them; the pairs form is that run call alone over the caller's list.  The host form takes the longest pairs of every segment from
 * HostBatchPairs (batch_api.cpp), pins the set the call started on, and keeps one counter per touched pattern (countsOnHost) inside
 * sortedSegmentLists, the host frame of such lists in pfac_host.h.
 */
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "pfac_host.h"

using namespace pfac_internal;

namespace {

/* what the three calls check first, in the order of the contract (the pattern set: under the lock); items: the input, or the pair list */
PFAC_status_t checkArgs(PFAC_handle_t handle, const void *items, size_t numItems, bool itemsRequired, const void *offsets, size_t numSegments,
                        unsigned int flags, const int *ids, const unsigned int *counts, size_t capacity, const size_t *segFirst,
                        const size_t *h_numEntries, const unsigned long long *h_total)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if ((itemsRequired && !items) || !h_numEntries || !h_total || (capacity && (!ids || !counts)) || (!offsets && numSegments != 1) ||
        (numSegments && !segFirst) || (flags & ~PFACX_COUNT_LONGEST))
        return PFAC_STATUS_INVALID_PARAMETER;
    if (numItems >= kTwoGiB || numSegments >= kTwoGiB || (numSegments == 0 && numItems > 0)) return PFAC_STATUS_INVALID_PARAMETER;
    return PFAC_STATUS_SUCCESS;
}

/* does the call follow the prefix chains?  Not for the longest counts, nor in a set in which no pattern is a prefix of another */
bool followsChains(const pfac::Automaton &fa, unsigned int flags) { return !(flags & PFACX_COUNT_LONGEST) && fa.maxChain > 1; }

/* the run call of both device forms behind their checks (the caller holds c->lock; numSegments > 0) */
PFAC_status_t runOnDevice(PFAC_context *c, const int *d_pairIds, size_t count, const int *d_segFirstPairs, size_t numSegments, unsigned int flags,
                          int *d_ids, unsigned int *d_counts, size_t capacity, size_t *d_segFirst, size_t *h_numEntries, unsigned long long *h_total)
{
    PFACX_segCountRun_t run{};
    run.d_pairIds = d_pairIds;
    run.count = count;
    run.d_segFirstPairs = d_segFirstPairs;
    run.numSegments = numSegments;
    run.d_table = followsChains(c->fa, flags) ? c->scratch.allTable.get() : nullptr;
    run.numIds = (size_t)c->fa.numPatterns;
    run.d_ids = d_ids;
    run.d_counts = d_counts;
    run.capacity = capacity;
    run.d_segFirst = d_segFirst;
    size_t entries = 0;
    unsigned long long total = 0;
    const PFAC_status_t st = c->segcount_run_ptr(c, &run, &entries, &total);
    if (st != PFAC_STATUS_SUCCESS) return st;
    *h_numEntries = entries;
    *h_total = total;
    return truncatedIf(entries, capacity);
}

/* nothing to count on the device: zeros, segFirst zeroed */
PFAC_status_t nothingOnDevice(size_t *d_segFirst, size_t numSegments, size_t *h_numEntries, unsigned long long *h_total)
{
    const PFAC_status_t st = zeroSegmentArrays(d_segFirst, nullptr, numSegments);
    if (st != PFAC_STATUS_SUCCESS) return st;
    *h_numEntries = 0;
    *h_total = 0;
    return PFAC_STATUS_SUCCESS;
}

/* The count list of a batch whose longest pairs are known: the ids of segment k at ids[first[k], first[k] + numPairs[k]).  Returns the full length */
size_t countsOnHost(const pfac::Automaton &fa, unsigned int flags, const int *ids, const size_t *first, const int *numPairs, size_t numSegments,
                    int *outIds, unsigned int *outCounts, size_t capacity, size_t *segFirst, unsigned long long *sum)
{
    const bool chains = followsChains(fa, flags);
    std::vector<unsigned int> counter((size_t)fa.numPatterns + 1, 0u);
    unsigned long long all = 0;
    auto fill = [&](size_t k, std::vector<int> &touched) {
        auto add = [&](int q) {
            if (counter[(size_t)q]++ == 0) touched.push_back(q);
            return true;
        };
        for (int i = 0; i < numPairs[k]; i++) {
            const int id = ids[first[k] + (size_t)i];
            if (chains) forEachChainMember(fa, id, add);
            else if (id >= 1 && id <= fa.numPatterns) add(id);
        }
    };
    const size_t total = sortedSegmentLists<int>(numSegments, capacity, segFirst, fill, [&](size_t, int q, size_t at, bool fits) {
        if (fits) { outIds[at] = q; outCounts[at] = counter[(size_t)q]; }
        all += counter[(size_t)q];
        counter[(size_t)q] = 0;
    });
    *sum = all;
    return total;
}

} // namespace

extern "C" {

PFAC_status_t PFACX_countBatchFromDevice(PFAC_handle_t handle, char *d_input, size_t size, const size_t *d_offsets, size_t numSegments,
                                         unsigned int flags, int *d_ids, unsigned int *d_counts, size_t capacity, size_t *d_segFirst,
                                         size_t *h_numEntries, unsigned long long *h_total)
{
    PFAC_status_t st = checkArgs(handle, d_input, size, true, d_offsets, numSegments, flags, d_ids, d_counts, capacity, d_segFirst, h_numEntries, h_total);
    if (st != PFAC_STATUS_SUCCESS) return st;
    PFAC_context *c = handle;
    if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(c->lock);
    if (!c->isPatternsReady) return PFAC_STATUS_PATTERNS_NOT_READY;
    if (size == 0) return nothingOnDevice(d_segFirst, numSegments, h_numEntries, h_total);
    if (followsChains(c->fa, flags)) st = ensureAllTable(c);
    BatchPairs pairs{};
    if (st == PFAC_STATUS_SUCCESS) st = scratchBatchPairs(c, d_input, size, d_offsets, numSegments, &pairs);
    if (st != PFAC_STATUS_SUCCESS) return st;
    return runOnDevice(c, pairs.ids, pairs.count, pairs.segFirstPairs, numSegments, flags, d_ids, d_counts, capacity, d_segFirst, h_numEntries, h_total);
}

PFAC_status_t PFACX_countBatchPairsFromDevice(PFAC_handle_t handle, const int *d_pairIds, size_t numPairs, const int *d_segFirstPairs,
                                              size_t numSegments, unsigned int flags, int *d_ids, unsigned int *d_counts, size_t capacity,
                                              size_t *d_segFirst, size_t *h_numEntries, unsigned long long *h_total)
{
    PFAC_status_t st = checkArgs(handle, d_pairIds, numPairs, numPairs != 0, d_segFirstPairs, numSegments, flags, d_ids, d_counts, capacity, d_segFirst,
                                 h_numEntries, h_total);
    if (st != PFAC_STATUS_SUCCESS) return st;
    PFAC_context *c = handle;
    if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(c->lock);
    if (!c->isPatternsReady) return PFAC_STATUS_PATTERNS_NOT_READY;
    if (numPairs == 0) return nothingOnDevice(d_segFirst, numSegments, h_numEntries, h_total);
    if (followsChains(c->fa, flags)) st = ensureAllTable(c);
    if (st != PFAC_STATUS_SUCCESS) return st;
    return runOnDevice(c, d_pairIds, numPairs, d_segFirstPairs, numSegments, flags, d_ids, d_counts, capacity, d_segFirst, h_numEntries, h_total);
}

PFAC_status_t PFACX_countBatchFromHost(PFAC_handle_t handle, char *h_input, size_t size, const size_t *h_offsets, size_t numSegments,
                                       unsigned int flags, int *h_ids, unsigned int *h_counts, size_t capacity, size_t *h_segFirst,
                                       size_t *h_numEntries, unsigned long long *h_total)
{
    PFAC_status_t st = checkArgs(handle, h_input, size, true, h_offsets, numSegments, flags, h_ids, h_counts, capacity, h_segFirst, h_numEntries, h_total);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (h_offsets && numSegments && !batchOffsetsValid(h_offsets, numSegments, size)) return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = handle;
    std::unique_lock<std::mutex> guard(c->lock);
    if (!c->isPatternsReady) return PFAC_STATUS_PATTERNS_NOT_READY;
    const unsigned long long generation = c->setGeneration;                    /* the set every scan below has to see */
    if (size == 0) {
        if (numSegments) std::memset(h_segFirst, 0, (numSegments + 1) * sizeof(size_t));
        *h_numEntries = 0;
        *h_total = 0;
        return PFAC_STATUS_SUCCESS;
    }
    HostBatchPairs pairs(c, h_input, size, h_offsets, numSegments, false, guard);
    if (pairs.status != PFAC_STATUS_SUCCESS) return pairs.status;
    st = pairs.pin(generation);
    if (st != PFAC_STATUS_SUCCESS) return st;                                  /* another thread has replaced the set meanwhile: PATTERNS_NOT_READY, no count is written */
    try {
        unsigned long long sum = 0;
        const size_t total = countsOnHost(c->fa, flags, pairs.ids, pairs.offsets, pairs.numPairs.data(), numSegments, h_ids, h_counts, capacity, h_segFirst, &sum);
        *h_numEntries = total;
        *h_total = sum;
        return truncatedIf(total, capacity);
    } catch (const std::bad_alloc &) {
        return PFAC_STATUS_ALLOC_FAILED;
    }
}

} /* extern "C" */
