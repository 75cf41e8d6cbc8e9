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

#include <mutex>
#include <vector>

#include "pfac_host.h"

namespace pfac_internal {

constexpr unsigned int kCountFlags = PFACX_COUNT_LONGEST | PFACX_COUNT_ACCUMULATE;

static bool countsFit(const pfac::Automaton &fa, size_t numCounts) { return fa.numPatterns >= 0 && numCounts >= (size_t)fa.numPatterns + 1; }   /* an entry for every id of the set, which the caller holds still */
/* what the count calls that need a pattern set check first */
static PFAC_status_t checkCountArgs(PFAC_handle_t handle, unsigned int flags, const unsigned long long *counts, size_t numCounts)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    const SetPin pin(handle);
    if (pin.status() != PFAC_STATUS_SUCCESS) return pin.status();
    if (!counts || (flags & ~kCountFlags) || !countsFit(handle->fa, numCounts)) return PFAC_STATUS_INVALID_PARAMETER;
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
        for (size_t id = 1; id <= F; id++)
            if (longest[id] != 0)
                forEachChainMember(fa, (int)id, [&](int q) { if ((size_t)q != id) L[(size_t)q] += longest[id]; return true; });
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
    if (size > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
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
    if (size > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    if (hostLacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    const HostPairs pairs(size, size);
    if (!pairs) return PFAC_STATUS_ALLOC_FAILED;
    int n = 0;
    unsigned long long generation = 0;
    if (size > 0) st = hostLongestPairs(handle, h_input, size, pairs.ids, pairs.pos, &n, &generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    const SetPin pin = size > 0 ? SetPin(handle, generation) : SetPin(handle);   /* the set the pairs came from; nothing scanned: whichever is loaded */
    if (pin.status() != PFAC_STATUS_SUCCESS) return pin.status();
    if (!countsFit(handle->fa, numCounts)) return PFAC_STATUS_INVALID_PARAMETER;   /* ... which need not be the one checkCountArgs saw */
    const size_t F = (size_t)handle->fa.numPatterns;
    try {
        std::vector<unsigned long long> L(F + 1, 0);
        for (int i = 0; i < n; i++)
            if (pairs.ids[i] > 0 && (size_t)pairs.ids[i] <= F) L[(size_t)pairs.ids[i]]++;
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
    if (numPairs > kMaxInt || (numPairs && !d_ids)) return PFAC_STATUS_INVALID_PARAMETER;
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
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
    if (!d_counts || (capacity && (!d_ids || !d_outCounts)) || numCounts > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(handle->lock);
    return handle->count_nonzero_ptr(handle, d_counts, numCounts, d_ids, d_outCounts, capacity, h_numDistinct, h_total);
}

} /* extern "C" */
