/*
 * words_api.cpp -- PFACX_matchWordsFromDevice / ...FromHost / PFACX_wordsPairsFromDevice (include/pfac_ext.h): the occurrences whose neighbours in
 * the input are not in a byte class -- whole words, whole lines, whole fields.
 *
 * Every pattern that starts at p is a prefix of the longest one that starts there, so the occurrences at p are the longest pair's prefix chain
 * (Automaton::prefixPattern); they share the byte in front of them, each has its own byte behind it.  The device form runs the unchanged
 * compacted-output path with its ordered pairs in handle scratch (PFACX_allReduce) and the boundary passes behind it (scan_words.hip:
 * PFACX_wordsRun), which read the CALLER's bytes; the pairs form runs those passes over a list of the caller's.  The host form takes the longest
 * pairs from hostLongestPairs into a temporary of its own and walks the chains here.
 */
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <mutex>

#include "pfac_host.h"

namespace pfac_internal {

/* [0-9A-Za-z_]: the class of a null h_class */
static const unsigned int kWordClass[8] = {0u, 0x03FF0000u, 0x87FFFFFEu, 0x07FFFFFEu, 0u, 0u, 0u, 0u};

/* what all three calls check first */
static PFAC_status_t checkWordsArgs(PFAC_handle_t handle, const void *input, size_t size, unsigned int flags, const size_t *h_num_matched)
{
    const PFAC_status_t st = checkSetAndPointers(handle, {input, h_num_matched});
    return st == PFAC_STATUS_SUCCESS && ((flags & ~PFACX_WORDS_ALL) || size > kMaxInt) ? PFAC_STATUS_INVALID_PARAMETER : st;
}

/* the boundary passes over `count` ordered longest pairs, behind the argument checks; the caller holds c->lock */
static PFAC_status_t wordsRunLocked(PFAC_context *c, const char *d_input, size_t size, const unsigned int *h_class, unsigned int flags,
                                    const int *d_pairIds, const int *d_pairPos, size_t count, int *d_ids, int *d_pos, size_t capacity,
                                    size_t *h_num_matched)
{
    PFAC_status_t st = ensurePatternLen(c);
    if (st == PFAC_STATUS_SUCCESS && c->fa.maxChain > 1) st = ensureAllTable(c);
    if (st != PFAC_STATUS_SUCCESS) return st;
    PFACX_wordsRun_t run{};
    run.d_input = d_input;
    run.size = size;
    run.d_pairIds = d_pairIds;
    run.d_pairPos = d_pairPos;
    run.count = count;
    run.d_table = c->fa.maxChain > 1 ? c->scratch.allTable.get() : nullptr;
    run.d_patternLen = c->scratch.patternLen.get();
    run.numIds = (size_t)(c->fa.numPatterns > 0 ? c->fa.numPatterns : 0);
    for (int k = 0; k < 8; k++) run.cls[k] = (h_class ? h_class : kWordClass)[k];
    run.all = (flags & PFACX_WORDS_ALL) ? 1u : 0u;
    run.d_ids = d_ids;
    run.d_pos = d_pos;
    run.capacity = capacity;
    size_t total = 0;
    st = c->words_run_ptr(c, &run, &total);
    if (st != PFAC_STATUS_SUCCESS) return st;
    *h_num_matched = total;
    return truncatedIf(total, capacity);
}

/* The host loop: the bounded members of the chains of `count` ordered longest pairs into ids / pos (slots >= capacity are not written); returns the
 * full length of the list */
static size_t wordsOnHost(const pfac::Automaton &fa, const unsigned char *in, size_t n, const unsigned int *cls, bool all, const int *pairIds,
                          const int *pairPos, size_t count, int *ids, int *pos, size_t capacity)
{
    size_t total = 0;
    for (size_t i = 0; i < count; i++) {
        const int id = pairIds[i], p = pairPos[i];
        if (p < 0 || (size_t)p >= n || (p > 0 && inClass(cls, in[p - 1]))) continue;
        forEachChainMember(fa, id, [&](int q) {
            const int len = fa.patternLen[(size_t)q];
            const size_t e = (size_t)p + (size_t)(len > 0 ? len : 0);
            if (len <= 0 || e > n || (e < n && inClass(cls, in[e]))) return true;
            if (total < capacity) { ids[total] = q; pos[total] = p; }
            total++;
            return all;                                                   /* list mode: the longest bounded member alone */
        });
    }
    return total;
}

} // namespace pfac_internal
using namespace pfac_internal;

extern "C" {

PFAC_status_t PFACX_matchWordsFromDevice(PFAC_handle_t handle, char *d_input, size_t size, const unsigned int *h_class, unsigned int flags, int *d_ids,
                                         int *d_pos, size_t capacity, size_t *h_num_matched)
{
    PFAC_status_t st = checkWordsArgs(handle, d_input, size, flags, h_num_matched);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (!d_ids || !d_pos) return PFAC_STATUS_INVALID_PARAMETER;
    if (size == 0) { *h_num_matched = 0; return PFAC_STATUS_SUCCESS; }
    if (capacity < size) return PFAC_STATUS_INVALID_PARAMETER;
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(handle->lock);
    DeviceScan scan;                                                       /* a caseless set: the scan reads the folded copy, the boundary passes the caller's bytes */
    st = beginDeviceScan(handle, d_input, size, &scan);
    if (st != PFAC_STATUS_SUCCESS) return st;
    /* the caller's arrays take the scan's unordered list, the ordered pairs go to the handle's pair scratch: the passes never filter in place */
    int count = 0;
    st = handle->all_reduce_ptr(handle, reinterpret_cast<int *>(scan.d_scan), (int)size, d_ids, d_pos, &count, scan.hashed);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (count < 0 || (size_t)count > size) return PFAC_STATUS_INTERNAL_ERROR;
    const int *pairIds = handle->scratch.allPairs.get();
    const int *pairPos = pairIds + handle->scratch.allPairs.count() / 2;   /* one allocation: the ids, then as many positions */
    if (count == 0) { *h_num_matched = 0; return PFAC_STATUS_SUCCESS; }
    return wordsRunLocked(handle, d_input, size, h_class, flags, pairIds, pairPos, (size_t)count, d_ids, d_pos, capacity, h_num_matched);
}

PFAC_status_t PFACX_matchWordsFromHost(PFAC_handle_t handle, char *h_input, size_t size, const unsigned int *h_class, unsigned int flags, int *h_ids,
                                       int *h_pos, size_t capacity, size_t *h_num_matched)
{
    PFAC_status_t st = checkWordsArgs(handle, h_input, size, flags, h_num_matched);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (!h_ids || !h_pos) return PFAC_STATUS_INVALID_PARAMETER;
    if (size == 0) { *h_num_matched = 0; return PFAC_STATUS_SUCCESS; }
    if (capacity < size) return PFAC_STATUS_INVALID_PARAMETER;
    if (hostLacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    const HostPairs pairs(size, size);
    if (!pairs) return PFAC_STATUS_ALLOC_FAILED;
    const PinnedPairs scan(handle, h_input, size, pairs.ids, pairs.pos);
    if (scan.status != PFAC_STATUS_SUCCESS) return scan.status;
    const size_t total = wordsOnHost(handle->fa, reinterpret_cast<const unsigned char *>(h_input), size, h_class ? h_class : kWordClass,
                                     (flags & PFACX_WORDS_ALL) != 0, pairs.ids, pairs.pos, (size_t)(scan.count > 0 ? scan.count : 0), h_ids, h_pos, capacity);
    *h_num_matched = total;
    return truncatedIf(total, capacity);
}

PFAC_status_t PFACX_wordsPairsFromDevice(PFAC_handle_t handle, const char *d_input, size_t size, const unsigned int *h_class, unsigned int flags,
                                         const int *d_pairIds, const int *d_pairPos, size_t numPairs, int *d_ids, int *d_pos, size_t capacity,
                                         size_t *h_num_matched)
{
    PFAC_status_t st = checkWordsArgs(handle, d_input, size, flags, h_num_matched);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (numPairs > kMaxInt || capacity > SIZE_MAX / sizeof(int) || (numPairs && (!d_pairIds || !d_pairPos)) || (capacity && (!d_ids || !d_pos)))
        return PFAC_STATUS_INVALID_PARAMETER;
    if (size == 0) { *h_num_matched = 0; return PFAC_STATUS_SUCCESS; }
    if (capacity && numPairs) {
        const size_t in = numPairs * sizeof(int), out = capacity * sizeof(int);
        if (overlap(d_ids, out, d_pairIds, in) || overlap(d_ids, out, d_pairPos, in) || overlap(d_pos, out, d_pairIds, in) || overlap(d_pos, out, d_pairPos, in))
            return PFAC_STATUS_INVALID_PARAMETER;
    }
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    if (numPairs == 0) { *h_num_matched = 0; return PFAC_STATUS_SUCCESS; }
    std::lock_guard<std::mutex> guard(handle->lock);
    return wordsRunLocked(handle, d_input, size, h_class, flags, d_pairIds, d_pairPos, numPairs, d_ids, d_pos, capacity, h_num_matched);
}

} /* extern "C" */
