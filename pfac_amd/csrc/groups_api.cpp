/*
 * groups_api.cpp -- PFACX_groupsOpen / PFACX_groupsClose / PFACX_groupsMatchFromDevice / ...FromHost / PFACX_groupsPairsFromDevice
 * (include/pfac_ext.h): each segment of a batch sees only the patterns whose 64-bit group mask meets the segment's.
 *
 * The mask table is resolved once, at open: the mask of every id that names a pattern is ORed into the id that pattern is reported under
 * (duplicate lines: ReportedIds, pfac_host.h), every other id ends with 0.  Every pattern that occurs at a position is a prefix of the longest one there, so all three forms
 * work on longest pairs and walk each pair's prefix chain (Automaton::prefixPattern) once; what decides a member is one 64-bit AND.  The device
 * form takes the ordered pairs of the batch in the handle's pair scratch from scratchBatchPairs (batch_api.cpp) and runs PFACX_groupsRun
 * (scan_groups.hip) over them; the pairs form is that run call alone over the caller's list.  The host form takes the longest pairs of every
 * segment, with their positions, from HostBatchPairs (batch_api.cpp), pins the set the table was opened on, and walks the chains in a loop of
 * its own (groupsOnHost).
 */
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "pfac_host.h"

struct PFACX_groups_s : pfac_internal::HandleObject {
    size_t numIds = 0;                        /* F of the pattern set it was opened on */
    std::vector<unsigned long long> masks;    /* [F + 1] by REPORTED id: the OR over the duplicate lines; 0 for entry 0 and for ids never reported */
    /* the same on the device, uploaded by the first device call: state of the table (deviceTableBytes), freed by PFACX_groupsClose */
    pfac::DeviceBuffer<unsigned long long> d_masks;

    ~PFACX_groups_s() override { d_masks.release(); }
    size_t deviceBytes() const override { return d_masks.bytes(); }
};

using namespace pfac_internal;

namespace {

/* the caller's masks by id resolved into g->masks (the caller holds the handle's lock) */
void resolveMasks(const pfac::Automaton &fa, const unsigned long long *given, PFACX_groups_s *g)
{
    const size_t F = (size_t)fa.numPatterns;
    g->masks.assign(F + 1, 0ull);
    ReportedIds reported(fa);                               /* (a lower id of duplicate lines may have a mask) */
    for (size_t id = 1; id <= F; id++) {
        if (given[id] == 0ull) continue;
        const int to = reported.of((int)id);
        if (to) g->masks[(size_t)to] |= given[id];          /* (0: a pattern the set does not report at all) */
    }
    g->numIds = F;
}

/* what the three match calls check first, in the order of the contract (the generation and the pattern set: under the lock); items: the input's
 * bytes, or the pairs */
PFAC_status_t checkMatchArgs(PFACX_groups_t groups, size_t numItems, bool itemsMissing, const void *offsets, size_t numSegments, unsigned int flags,
                             const int *ids, const int *pos, size_t capacity, const size_t *h_num_matched)
{
    if (!groups || !groups->handle) return PFAC_STATUS_INVALID_HANDLE;
    if (numItems >= kTwoGiB || numSegments >= kTwoGiB || (flags & ~PFACX_GROUPS_ALL)) return PFAC_STATUS_INVALID_PARAMETER;
    if (itemsMissing || !h_num_matched || (capacity && (!ids || !pos)) || (!offsets && numSegments != 1) || (numSegments == 0 && numItems > 0))
        return PFAC_STATUS_INVALID_PARAMETER;
    return PFAC_STATUS_SUCCESS;
}

/* the first device call of a group handle: its mask table (the caller holds the handle's lock) */
PFAC_status_t ensureDeviceMasks(PFACX_groups_s *g) { return g->d_masks ? PFAC_STATUS_SUCCESS : g->d_masks.upload(g->masks.data(), g->masks.size()); }

/* nothing to match on the device: 0 pairs, segFirst and segGroups zeroed where given */
PFAC_status_t nothingOnDevice(size_t *d_segFirst, unsigned long long *d_segGroups, size_t numSegments, size_t *h_num_matched)
{
    const PFAC_status_t st = zeroSegmentArrays(d_segFirst, d_segGroups, numSegments);
    if (st != PFAC_STATUS_SUCCESS) return st;
    *h_num_matched = 0;
    return PFAC_STATUS_SUCCESS;
}

/* the run call of both device forms behind their checks (the caller holds c->lock; numSegments > 0) */
PFAC_status_t runOnDevice(PFACX_groups_s *g, const int *d_pairIds, const int *d_pairPos, size_t count, const int *d_segFirstPairs, size_t numSegments,
                          const unsigned long long *d_segMasks, unsigned int flags, int *d_ids, int *d_pos, size_t capacity, size_t *d_segFirst,
                          unsigned long long *d_segGroups, size_t *h_num_matched)
{
    PFAC_context *c = g->handle;
    PFACX_groupsRun_t run{};
    run.d_pairIds = d_pairIds;
    run.d_pairPos = d_pairPos;
    run.count = count;
    run.d_segFirstPairs = d_segFirstPairs;
    run.numSegments = numSegments;
    run.d_segMasks = d_segMasks;
    run.d_patternMasks = g->d_masks.get();
    run.d_table = c->fa.maxChain > 1 ? c->scratch.allTable.get() : nullptr;
    run.numIds = g->numIds;
    run.all = (flags & PFACX_GROUPS_ALL) ? 1u : 0u;
    run.d_ids = d_ids;
    run.d_pos = d_pos;
    run.capacity = capacity;
    run.d_segFirst = d_segFirst;
    run.d_segGroups = d_segGroups;
    size_t total = 0;
    const PFAC_status_t st = c->groups_run_ptr(c, &run, &total);
    if (st != PFAC_STATUS_SUCCESS) return st;
    *h_num_matched = total;
    return truncatedIf(total, capacity);
}

/* The group list of a batch whose longest pairs are known: the ids of segment k at ids[first[k], first[k] + numPairs[k]), their positions in the
 * segment at pos[] likewise; positions are reported relative to the buffer.  Returns the full length */
size_t groupsOnHost(const pfac::Automaton &fa, const PFACX_groups_s &g, const int *ids, const int *pos, const size_t *first, const int *numPairs,
                    size_t numSegments, const unsigned long long *segMasks, bool all, int *outIds, int *outPos, size_t capacity, size_t *segFirst,
                    unsigned long long *segGroups)
{
    size_t total = 0;
    for (size_t k = 0; k < numSegments; k++) {
        if (segFirst) segFirst[k] = total;
        const unsigned long long segMask = segMasks ? segMasks[k] : ~0ull;
        unsigned long long hits = 0;
        for (int i = 0; segMask != 0ull && i < numPairs[k]; i++) {
            const int p = (int)(first[k] + (size_t)pos[first[k] + (size_t)i]);
            bool found = false;
            forEachChainMember(fa, ids[first[k] + (size_t)i], [&](int q) {       /* (the caller's pin: fa.numPatterns == g.numIds) */
                const unsigned long long m = g.masks[(size_t)q] & segMask;
                if (m == 0ull) return true;
                hits |= m;                                                      /* over the whole chain, whatever is reported */
                if (all || !found) {
                    if (total < capacity) { outIds[total] = q; outPos[total] = p; }
                    total++;
                    found = true;
                }
                return true;
            });
        }
        if (segGroups) segGroups[k] = hits;
    }
    if (segFirst) segFirst[numSegments] = total;
    return total;
}

} // namespace

extern "C" {

PFAC_status_t PFACX_groupsOpen(PFAC_handle_t handle, const unsigned long long *h_patternMasks, size_t numMasks, PFACX_groups_t *groups)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!groups) return PFAC_STATUS_INVALID_PARAMETER;
    *groups = nullptr;
    if (!h_patternMasks) return PFAC_STATUS_INVALID_PARAMETER;
    return adoptNew(handle, groups, [=](PFACX_groups_s &g) -> PFAC_status_t {
        if (numMasks < (size_t)handle->fa.numPatterns + 1) return PFAC_STATUS_INVALID_PARAMETER;
        resolveMasks(handle->fa, h_patternMasks, &g);
        return PFAC_STATUS_SUCCESS;
    });
}

PFAC_status_t PFACX_groupsClose(PFACX_groups_t groups) { return closeObject(groups); }

PFAC_status_t PFACX_groupsMatchFromDevice(PFACX_groups_t groups, char *d_input, size_t size, const size_t *d_offsets, size_t numSegments,
                                          const unsigned long long *d_segMasks, unsigned int flags, int *d_ids, int *d_pos, size_t capacity,
                                          size_t *d_segFirst, unsigned long long *d_segGroups, size_t *h_num_matched)
{
    PFAC_status_t st = checkMatchArgs(groups, size, !d_input, d_offsets, numSegments, flags, d_ids, d_pos, capacity, h_num_matched);
    if (st != PFAC_STATUS_SUCCESS) return st;
    PFAC_context *c = groups->handle;
    if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(c->lock);
    st = checkSetGeneration(c, groups->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0) return nothingOnDevice(d_segFirst, d_segGroups, numSegments, h_num_matched);
    st = ensureDeviceMasks(groups);
    if (st == PFAC_STATUS_SUCCESS && c->fa.maxChain > 1) st = ensureAllTable(c);
    BatchPairs pairs{};
    if (st == PFAC_STATUS_SUCCESS) st = scratchBatchPairs(c, d_input, size, d_offsets, numSegments, &pairs);
    if (st != PFAC_STATUS_SUCCESS) return st;
    return runOnDevice(groups, pairs.ids, pairs.pos, pairs.count, pairs.segFirstPairs, numSegments, d_segMasks, flags, d_ids, d_pos, capacity, d_segFirst,
                       d_segGroups, h_num_matched);
}

PFAC_status_t PFACX_groupsPairsFromDevice(PFACX_groups_t groups, const int *d_pairIds, const int *d_pairPos, size_t numPairs,
                                          const int *d_segFirstPairs, size_t numSegments, const unsigned long long *d_segMasks, unsigned int flags,
                                          int *d_ids, int *d_pos, size_t capacity, size_t *d_segFirst, unsigned long long *d_segGroups,
                                          size_t *h_num_matched)
{
    PFAC_status_t st = checkMatchArgs(groups, numPairs, numPairs && (!d_pairIds || !d_pairPos), d_segFirstPairs, numSegments, flags, d_ids, d_pos,
                                      capacity, h_num_matched);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (capacity > SIZE_MAX / sizeof(int)) return PFAC_STATUS_INVALID_PARAMETER;
    if (capacity && numPairs) {
        const size_t in = numPairs * sizeof(int), out = capacity * sizeof(int);
        if (overlap(d_ids, out, d_pairIds, in) || overlap(d_ids, out, d_pairPos, in) || overlap(d_pos, out, d_pairIds, in) || overlap(d_pos, out, d_pairPos, in))
            return PFAC_STATUS_INVALID_PARAMETER;
    }
    PFAC_context *c = groups->handle;
    if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(c->lock);
    st = checkSetGeneration(c, groups->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (numPairs == 0) return nothingOnDevice(d_segFirst, d_segGroups, numSegments, h_num_matched);
    st = ensureDeviceMasks(groups);
    if (st == PFAC_STATUS_SUCCESS && c->fa.maxChain > 1) st = ensureAllTable(c);
    if (st != PFAC_STATUS_SUCCESS) return st;
    return runOnDevice(groups, d_pairIds, d_pairPos, numPairs, d_segFirstPairs, numSegments, d_segMasks, flags, d_ids, d_pos, capacity, d_segFirst,
                       d_segGroups, h_num_matched);
}

PFAC_status_t PFACX_groupsMatchFromHost(PFACX_groups_t groups, char *h_input, size_t size, const size_t *h_offsets, size_t numSegments,
                                        const unsigned long long *h_segMasks, unsigned int flags, int *h_ids, int *h_pos, size_t capacity,
                                        size_t *h_segFirst, unsigned long long *h_segGroups, size_t *h_num_matched)
{
    PFAC_status_t st = checkMatchArgs(groups, size, !h_input, h_offsets, numSegments, flags, h_ids, h_pos, capacity, h_num_matched);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (h_offsets && numSegments && !batchOffsetsValid(h_offsets, numSegments, size)) return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = groups->handle;
    std::unique_lock<std::mutex> guard(c->lock);
    st = checkSetGeneration(c, groups->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0) {
        if (h_segFirst && numSegments) std::memset(h_segFirst, 0, (numSegments + 1) * sizeof(size_t));
        if (h_segGroups && numSegments) std::memset(h_segGroups, 0, numSegments * sizeof(unsigned long long));
        *h_num_matched = 0;
        return PFAC_STATUS_SUCCESS;
    }
    HostBatchPairs pairs(c, h_input, size, h_offsets, numSegments, true, guard);
    if (pairs.status != PFAC_STATUS_SUCCESS) return pairs.status;
    if (pairs.pin(groups->generation) != PFAC_STATUS_SUCCESS) return PFAC_STATUS_INVALID_PARAMETER;      /* another thread has replaced the set meanwhile: the contract's answer for a group table */
    const size_t total = groupsOnHost(c->fa, *groups, pairs.ids, pairs.pos, pairs.offsets, pairs.numPairs.data(), numSegments, h_segMasks,
                                      (flags & PFACX_GROUPS_ALL) != 0, h_ids, h_pos, capacity, h_segFirst, h_segGroups);
    *h_num_matched = total;
    return truncatedIf(total, capacity);
}

} /* extern "C" */
