/*
 * order_api.cpp -- PFACX_orderHitsFromDevice / ...FromHost (include/pfac_ext.h): a hit list of up to four int columns put in start order, stably,
 * with ascending ids among equal starts where PFACX_ORDER_TIES_BY_ID asks for it.
 *
 * No matcher runs and no pattern set is read: the device form is the argument checks and one call into the module (scan_order_hits.hip:
 * PFACX_orderRun, a radix sort over (key, index) pairs in handle scratch); the host form is a stable sort of an index array with the same
 * comparator and one gather per column -- memory proportional to numHits.
 */
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "pfac_host.h"

namespace pfac_internal {

/* what both forms refuse, in the order of the header */
static PFAC_status_t checkOrderArgs(PFAC_context *c, const int *start, const int *ids, const int *end, const int *aux, size_t numHits,
                                    unsigned int flags, const int *perm)
{
    if (!c) return PFAC_STATUS_INVALID_PARAMETER;
    if (numHits && !start) return PFAC_STATUS_INVALID_PARAMETER;
    if (numHits > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    if (flags & ~PFACX_ORDER_TIES_BY_ID) return PFAC_STATUS_INVALID_PARAMETER;
    if ((flags & PFACX_ORDER_TIES_BY_ID) && !ids) return PFAC_STATUS_INVALID_PARAMETER;
    const int *given[5] = {start, ids, end, aux, perm};
    const size_t bytes = numHits * sizeof(int);
    for (int i = 0; i < 5; i++)
        for (int j = i + 1; j < 5; j++)
            if (given[i] && given[j] && overlap(given[i], bytes, given[j], bytes)) return PFAC_STATUS_INVALID_PARAMETER;
    return PFAC_STATUS_SUCCESS;
}

} // namespace pfac_internal
using namespace pfac_internal;

extern "C" {

PFAC_status_t PFACX_orderHitsFromDevice(PFAC_handle_t handle, int *d_start, int *d_ids, int *d_end, int *d_aux, size_t numHits, unsigned int flags,
                                        int *d_perm, int *h_wasOrdered)
{
    const PFAC_status_t st = checkOrderArgs(handle, d_start, d_ids, d_end, d_aux, numHits, flags, d_perm);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    if (numHits == 0) {
        if (h_wasOrdered) *h_wasOrdered = 1;
        return PFAC_STATUS_SUCCESS;
    }
    std::lock_guard<std::mutex> guard(handle->lock);
    PFACX_orderRun_t run{};
    run.d_start = d_start;
    run.d_ids = d_ids;
    run.d_end = d_end;
    run.d_aux = d_aux;
    run.numHits = numHits;
    run.flags = flags;
    run.d_perm = d_perm;
    int wasOrdered = 0;
    const PFAC_status_t ran = handle->order_run_ptr(handle, &run, &wasOrdered);
    if (ran != PFAC_STATUS_SUCCESS) return ran;
    if (h_wasOrdered) *h_wasOrdered = wasOrdered;
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_orderHitsFromHost(PFAC_handle_t handle, int *h_start, int *h_ids, int *h_end, int *h_aux, size_t numHits, unsigned int flags,
                                      int *h_perm, int *h_wasOrdered)
{
    const PFAC_status_t st = checkOrderArgs(handle, h_start, h_ids, h_end, h_aux, numHits, flags, h_perm);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (numHits == 0) {
        if (h_wasOrdered) *h_wasOrdered = 1;
        return PFAC_STATUS_SUCCESS;
    }
    std::lock_guard<std::mutex> guard(handle->lock);
    const bool ties = (flags & PFACX_ORDER_TIES_BY_ID) != 0;
    /* entry a goes in front of entry b; equal entries keep their incoming order (the sort is stable) */
    const auto before = [&](int a, int b) {
        if (h_start[a] != h_start[b]) return h_start[a] < h_start[b];
        return ties && h_ids[a] < h_ids[b];
    };
    bool ordered = true;
    for (size_t k = 1; k < numHits && ordered; k++) ordered = !before((int)k, (int)(k - 1));
    if (ordered) {
        if (h_perm)
            for (size_t k = 0; k < numHits; k++) h_perm[k] = (int)k;
        if (h_wasOrdered) *h_wasOrdered = 1;
        return PFAC_STATUS_SUCCESS;
    }
    try {
        std::vector<int> index(numHits), temp(numHits);                        /* nothing of the caller's is written before both exist */
        for (size_t k = 0; k < numHits; k++) index[k] = (int)k;
        std::stable_sort(index.begin(), index.end(), before);
        for (int *col : {h_start, h_ids, h_end, h_aux}) {
            if (!col) continue;
            for (size_t k = 0; k < numHits; k++) temp[k] = col[index[k]];
            std::copy(temp.begin(), temp.end(), col);
        }
        if (h_perm) std::copy(index.begin(), index.end(), h_perm);
    } catch (const std::bad_alloc &) { return PFAC_STATUS_ALLOC_FAILED; }
    if (h_wasOrdered) *h_wasOrdered = 0;
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
