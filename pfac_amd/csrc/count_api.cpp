/*
 * count_api.cpp -- PFACX_countFromDevice / ...FromHost / PFACX_countPairsFromDevice / PFACX_countNonzeroFromDevice (include/pfac_ext.h): which
 * patterns occurred, and how often.
 *
 * Every pattern that occurs at a position is a prefix of the longest one there, so the number of occurrences of pattern id is the longest histogram
 * summed over the patterns that have id on their prefix chain (Automaton::prefixPattern).  The device form is the compacted scan without its
 * ordering launches, into the pair scratch of the all-match calls, and a histogram, a store and a chain pass behind it (scan_count.hip:
 * PFACX_countPairs); the host form takes the longest pairs from hostLongestPairs into a temporary of its own -- ids and positions, `size` ints
 * each on every platform (the positions are not read, and on a CPU platform not written beyond the pairs: the price of the one helper is address
 * space) -- and counts here.
 */
#include <hip/hip_runtime_api.h>

#include <memory>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <vector>

#include "pfac_host.h"

namespace pfac_internal {

constexpr unsigned int kCountFlags = PFACX_COUNT_LONGEST | PFACX_COUNT_ACCUMULATE;

/* what the count calls that need a pattern set check first */
static PFAC_status_t checkCountArgs(PFAC_handle_t handle, unsigned int flags, const unsigned long long *counts, size_t numCounts)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!handle->isPatternsReady) return PFAC_STATUS_PATTERNS_NOT_READY;
    if (!counts || (flags & ~kCountFlags)) return PFAC_STATUS_INVALID_PARAMETER;
    if (handle->fa.numPatterns < 0 || numCounts < (size_t)handle->fa.numPatterns + 1) return PFAC_STATUS_INVALID_PARAMETER;
    return PFAC_STATUS_SUCCESS;
}

/* the table the device passes follow, or null: the longest histogram, or a set in which no pattern is a prefix of another */
static PFAC_status_t chainTable(PFAC_context *c, unsigned int flags, const void **d_table)
{
    *d_table = nullptr;
    if ((flags & PFACX_COUNT_LONGEST) || c->fa.maxChain <= 1) return PFAC_STATUS_SUCCESS;
    const PFAC_status_t st = ensureAllTable(c);
    if (st == PFAC_STATUS_SUCCESS) *d_table = c->scratch.allTable.get();
    return st;
}

/* counts[] from the longest histogram L (F + 1 entries; on return the histogram the call stands for); returns what the call added */
static unsigned long long countsFromLongest(const pfac::Automaton &fa, std::vector<unsigned long long> &L, unsigned int flags, unsigned long long *counts)
{
    const size_t F = (size_t)fa.numPatterns;
    unsigned long long total = 0;
    if (!(flags & PFACX_COUNT_LONGEST) && fa.maxChain > 1) {
        const std::vector<unsigned long long> longest(L);
        for (size_t id = 1; id <= F; id++) {
            if (longest[id] == 0) continue;
            int q = fa.prefixPattern[id];
            for (int k = 1; k < fa.chainLen[id] && q >= 1 && (size_t)q <= F; k++) {
                L[(size_t)q] += longest[id];
                q = fa.prefixPattern[(size_t)q];
            }
        }
    }
    for (size_t id = 1; id <= F; id++) total += L[id];
    if (flags & PFACX_COUNT_ACCUMULATE) {
        for (size_t id = 1; id <= F; id++) counts[id] += L[id];
    } else {
        counts[0] = 0;
        for (size_t id = 1; id <= F; id++) counts[id] = L[id];
    }
    return total;
}

} // namespace pfac_internal
using namespace pfac_internal;

extern "C" {

PFAC_status_t PFACX_countFromDevice(PFAC_handle_t handle, char *d_input, size_t size, unsigned int flags, unsigned long long *d_counts,
                                    size_t numCounts, size_t *h_total)
{
    PFAC_status_t st = checkCountArgs(handle, flags, d_counts, numCounts);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (!d_input || !h_total) return PFAC_STATUS_INVALID_PARAMETER;
    if (size > (size_t)0x7fffffff) return PFAC_STATUS_INVALID_PARAMETER;   /* int positions */
    if (!handle->hasDevice || !handle->module) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(handle->lock);
    if (size == 0) {                                                       /* nothing matched: the counts zeroed, or left alone */
        st = handle->count_pairs_ptr(handle, nullptr, 0, 0, nullptr, 0, nullptr, flags, d_counts, nullptr);
        if (st == PFAC_STATUS_SUCCESS && hipStreamSynchronize(0) != hipSuccess) st = PFAC_STATUS_INTERNAL_ERROR;
        if (st == PFAC_STATUS_SUCCESS) *h_total = 0;
        return st;
    }
    const void *d_table = nullptr;
    st = chainTable(handle, flags, &d_table);
    if (st != PFAC_STATUS_SUCCESS) return st;
    DeviceScan scan;                                                       /* a caseless set: the scan reads the folded copy */
    st = beginDeviceScan(handle, d_input, size, &scan);
    if (st != PFAC_STATUS_SUCCESS) return st;
    return handle->count_pairs_ptr(handle, scan.d_scan, size, scan.hashed, nullptr, 0, d_table, flags, d_counts, h_total);
}

PFAC_status_t PFACX_countFromHost(PFAC_handle_t handle, char *h_input, size_t size, unsigned int flags, unsigned long long *h_counts, size_t numCounts,
                                  size_t *h_total)
{
    PFAC_status_t st = checkCountArgs(handle, flags, h_counts, numCounts);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (!h_input || !h_total) return PFAC_STATUS_INVALID_PARAMETER;
    if (size > (size_t)0x7fffffff) return PFAC_STATUS_INVALID_PARAMETER;
    if (handle->platform == PFAC_PLATFORM_GPU && (!handle->hasDevice || !handle->module)) return PFAC_STATUS_LIB_NOT_EXIST;
    const size_t F = (size_t)handle->fa.numPatterns;
    std::vector<unsigned long long> L;
    std::unique_ptr<int[]> pairs(new (std::nothrow) int[2 * size + 1]);   /* the ids, then the positions; not initialised: a page nothing writes costs nothing */
    try {
        L.assign(F + 1, 0);
    } catch (const std::bad_alloc &) {
        return PFAC_STATUS_ALLOC_FAILED;
    }
    if (!pairs) return PFAC_STATUS_ALLOC_FAILED;
    if (size > 0) {
        int n = 0;
        const int *ids = pairs.get();
        st = hostLongestPairs(handle, h_input, size, pairs.get(), pairs.get() + size, &n);
        if (st != PFAC_STATUS_SUCCESS) return st;
        for (int i = 0; i < n; i++)
            if (ids[i] > 0 && (size_t)ids[i] <= F) L[(size_t)ids[i]]++;
    }
    std::shared_lock<std::shared_mutex> tables(handle->tablesInUse);
    if ((size_t)handle->fa.numPatterns != F) return PFAC_STATUS_PATTERNS_NOT_READY;          /* another thread has replaced the set meanwhile */
    try {
        *h_total = (size_t)countsFromLongest(handle->fa, L, flags, h_counts);
    } catch (const std::bad_alloc &) {
        return PFAC_STATUS_ALLOC_FAILED;
    }
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_countPairsFromDevice(PFAC_handle_t handle, const int *d_ids, size_t numPairs, unsigned int flags, unsigned long long *d_counts,
                                         size_t numCounts)
{
    PFAC_status_t st = checkCountArgs(handle, flags, d_counts, numCounts);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (numPairs > (size_t)0x7fffffff || (numPairs && !d_ids)) return PFAC_STATUS_INVALID_PARAMETER;
    if (!handle->hasDevice || !handle->module) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(handle->lock);
    const void *d_table = nullptr;
    st = chainTable(handle, flags, &d_table);
    if (st != PFAC_STATUS_SUCCESS) return st;
    return handle->count_pairs_ptr(handle, nullptr, 0, 0, d_ids, numPairs, d_table, flags, d_counts, nullptr);
}

PFAC_status_t PFACX_countNonzeroFromDevice(PFAC_handle_t handle, const unsigned long long *d_counts, size_t numCounts, int *d_ids,
                                           unsigned long long *d_outCounts, size_t capacity, size_t *h_numDistinct, unsigned long long *h_total)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!h_numDistinct || !h_total) return PFAC_STATUS_INVALID_PARAMETER;
    if (numCounts == 0) { *h_numDistinct = 0; *h_total = 0; return PFAC_STATUS_SUCCESS; }
    if (!d_counts || (capacity && (!d_ids || !d_outCounts)) || numCounts > (size_t)0x7fffffff) return PFAC_STATUS_INVALID_PARAMETER;
    if (!handle->hasDevice || !handle->module) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(handle->lock);
    return handle->count_nonzero_ptr(handle, d_counts, numCounts, d_ids, d_outCounts, capacity, h_numDistinct, h_total);
}

} /* extern "C" */
