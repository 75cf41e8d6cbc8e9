/*
 * all_api.cpp -- PFACX_matchAllFromDevice / ...FromHost / PFACX_matchAllBatchFromDevice (include/pfac_ext.h): every pattern that
 * occurs at a position, not only the longest.
 *
 * Every pattern that starts at p is a prefix of the longest one that starts there, so the list is the longest-match list with each
 * pair followed by its chain of prefix patterns (Automaton::prefixPattern).  The GPU forms run the unchanged compacted-output path
 * with its ordered pairs in handle scratch (PFACX_allReduce), the batch fix-up of PFACX_matchBatchFromDeviceReduce where there are
 * segments, and the expansion (scan_all.hip) into the caller's arrays.  The host form takes the longest pairs from hostLongestPairs and
 * expands them in place on the host.  A set in
 * which no pattern is a prefix of another (maxChain == 1) needs no expansion: each call is its compacted counterpart.
 */
#include <hip/hip_runtime_api.h>

#include <mutex>
#include <vector>

#include "pfac_host.h"

namespace pfac_internal {

/* the device copy of {prefixPattern, chainLen} by id that the expansion and the count calls read (uploaded on the first call that needs it) */
PFAC_status_t ensureAllTable(PFAC_context *c)
{
    if (c->scratch.allTable) return PFAC_STATUS_SUCCESS;
    std::vector<pfac::Int2> t(c->fa.prefixPattern.size());
    for (size_t id = 0; id < t.size(); id++) t[id] = pfac::Int2{c->fa.prefixPattern[id], c->fa.chainLen[id]};
    return c->scratch.allTable.upload(t.data(), t.size());
}

/* the GPU forms behind their argument checks (0 < size < 2^31, capacity >= size; d_offsets null: one segment, no d_segFirst); the caller holds c->lock */
static PFAC_status_t matchAllDeviceLocked(PFAC_context *c, char *d_input, size_t size, const size_t *d_offsets, size_t numSegments,
                                          int *d_ids, int *d_pos, size_t capacity, size_t *d_segFirst, size_t *h_num_matched)
{
    DeviceScan scan;
    PFAC_status_t st = beginDeviceScan(c, d_input, size, &scan);
    if (st != PFAC_STATUS_SUCCESS) return st;
    d_input = scan.d_scan;
    const bool expand = c->fa.maxChain > 1;
    if (d_offsets) st = ensurePatternLen(c);
    if (st == PFAC_STATUS_SUCCESS && d_offsets) st = c->scratch.allSegFirst.reserve(numSegments + 1);      /* the first longest pair of each segment */
    if (st == PFAC_STATUS_SUCCESS && expand) st = ensureAllTable(c);
    if (st != PFAC_STATUS_SUCCESS) return st;
    int count = 0;
    int *ids = d_ids, *pos = d_pos;
    if (expand) {                                                   /* the pairs into handle scratch (PFACX_allReduce reserves it), the fix-up behind them */
        st = c->all_reduce_ptr(c, reinterpret_cast<int *>(d_input), (int)size, d_ids, d_pos, &count, scan.hashed);
        ids = c->scratch.allPairs.get();
        pos = ids + c->scratch.allPairs.count() / 2;              /* one allocation: the ids, then as many positions */
        if (st == PFAC_STATUS_SUCCESS && d_offsets)
            st = c->batch_reduce_fixup_ptr(c, d_input, size, d_offsets, numSegments, ids, pos, &count, c->scratch.allSegFirst.get(), c->scratch.patternLen.get());
    } else {                                                        /* ... straight into the caller's arrays */
        st = batchReduceLocked(c, d_input, size, d_offsets, numSegments, d_ids, d_pos, d_offsets ? c->scratch.allSegFirst.get() : nullptr, &count);
    }
    if (st != PFAC_STATUS_SUCCESS) return st;
    size_t total = (size_t)count;
    if (expand || d_offsets)
        st = c->all_expand_ptr(c, ids, pos, (size_t)count, expand ? c->scratch.allTable.get() : nullptr, d_ids, d_pos, capacity,
                               d_offsets ? c->scratch.allSegFirst.get() : nullptr, numSegments, d_segFirst, &total);
    if (st != PFAC_STATUS_SUCCESS) return st;
    *h_num_matched = total;
    return truncatedIf(total, capacity);
}

/* The `count` ordered longest pairs in ids / pos (room for `capacity` >= count) become the all-match list, in place: walked from
 * the last pair to the first, pair i lands at offsets >= i, so no pair is overwritten before it has been read.  Returns the full
 * length; slots >= capacity are not written. */
static size_t expandOnHost(const pfac::Automaton &fa, int *ids, int *pos, size_t count, size_t capacity)
{
    /* the members forEachChainMember visits (the ids come from a scan of this set: all of them are in [1, numPatterns]) */
    auto chainOf = [&](int id) -> size_t { return id < 1 || id > fa.numPatterns ? 0 : (fa.chainLen[(size_t)id] > 1 ? (size_t)fa.chainLen[(size_t)id] : 1); };
    size_t total = 0;
    for (size_t i = 0; i < count; i++) total += chainOf(ids[i]);
    if (fa.maxChain <= 1) return total;
    size_t o = total;
    for (size_t i = count; i-- > 0;) {
        const int id = ids[i], p = pos[i];
        size_t k = o -= chainOf(id);
        forEachChainMember(fa, id, [&](int q) {
            if (k < capacity) { ids[k] = q; pos[k] = p; }
            k++;
            return true;
        });
    }
    return total;
}

} // namespace pfac_internal
using namespace pfac_internal;

extern "C" {

PFAC_status_t PFACX_matchAllFromDevice(PFAC_handle_t handle, char *d_input, size_t size, int *d_ids, int *d_pos, size_t capacity,
                                       size_t *h_num_matched)
{
    if (const PFAC_status_t st = checkSetAndPointers(handle, {d_input, d_ids, d_pos, h_num_matched})) return st;
    if (size == 0) { *h_num_matched = 0; return PFAC_STATUS_SUCCESS; }
    if (capacity < size) return PFAC_STATUS_INVALID_PARAMETER;
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    if (size > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    std::lock_guard<std::mutex> guard(handle->lock);
    return matchAllDeviceLocked(handle, d_input, size, nullptr, 0, d_ids, d_pos, capacity, nullptr, h_num_matched);
}

PFAC_status_t PFACX_matchAllFromHost(PFAC_handle_t handle, char *h_input, size_t size, int *h_ids, int *h_pos, size_t capacity,
                                     size_t *h_num_matched)
{
    if (const PFAC_status_t st = checkSetAndPointers(handle, {h_input, h_ids, h_pos, h_num_matched})) return st;
    if (size == 0) { *h_num_matched = 0; return PFAC_STATUS_SUCCESS; }
    if (capacity < size) return PFAC_STATUS_INVALID_PARAMETER;
    if (size > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    const PinnedPairs scan(handle, h_input, size, h_ids, h_pos);
    if (scan.status != PFAC_STATUS_SUCCESS) return scan.status;
    const size_t total = expandOnHost(handle->fa, h_ids, h_pos, (size_t)scan.count, capacity);
    *h_num_matched = total;
    return truncatedIf(total, capacity);
}

PFAC_status_t PFACX_matchAllBatchFromDevice(PFAC_handle_t handle, char *d_input, size_t size, const size_t *d_offsets, size_t numSegments,
                                            int *d_ids, int *d_pos, size_t capacity, size_t *d_segFirst, size_t *h_num_matched)
{
    if (const PFAC_status_t st = checkSetAndPointers(handle, {d_input, d_offsets, d_ids, d_pos, d_segFirst, h_num_matched})) return st;
    if (size == 0) { *h_num_matched = 0; return PFAC_STATUS_SUCCESS; }
    if (numSegments == 0 || numSegments >= SIZE_MAX / sizeof(size_t)) return PFAC_STATUS_INVALID_PARAMETER;
    if (capacity < size) return PFAC_STATUS_INVALID_PARAMETER;
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    if (size > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    std::lock_guard<std::mutex> guard(handle->lock);
    return matchAllDeviceLocked(handle, d_input, size, d_offsets, numSegments, d_ids, d_pos, capacity, d_segFirst, h_num_matched);
}

} /* extern "C" */
