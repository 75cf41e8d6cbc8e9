/*
 * locate_api.cpp -- PFACX_locatePairsFromDevice / ...FromHost, PFACX_matchLocatedFromDevice / ...FromHost (include/pfac_ext.h): the record and the
 * column of every position of a list -- what `grep -n -b -o` prints -- by the cuts that PFACX_split* defines for the same class and flags.
 *
 * record(p) = the number of cuts <= p, column(p) = p - the largest such cut (0: none); -1 both for a position outside [0, size).  The device
 * forms are the passes of scan_locate.hip (PFACX_locateRun) over the handle's locate scratch (pfac::DeviceScratch::locate: counted by
 * PFACX_getInfo, freed by PFACX_trim with every other scratch buffer).  The host forms are the loop below on every platform: one forward walk over
 * the input and the positions together, no offsets array.  The pairs forms need no pattern set; the scan forms are the compacted-output call
 * (PFAC_matchFromDeviceReduce; on the host hostLongestPairs) with the located pairs behind it.  Nothing folds the class: it is tested on the
 * caller's bytes.
 */
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <mutex>

#include "pfac_host.h"

namespace pfac_internal {

/* what both pairs forms check first */
static PFAC_status_t checkLocateArgs(PFAC_handle_t handle, const void *input, size_t size, unsigned int flags, const int *pos, size_t numPairs,
                                     const int *record)
{
    if (!handle || !input || (flags & ~(PFACX_SPLIT_BEFORE | PFACX_SPLIT_RUNS)) || size > kMaxInt || numPairs > kMaxInt ||
        (numPairs && (!pos || !record)))
        return PFAC_STATUS_INVALID_PARAMETER;
    return PFAC_STATUS_SUCCESS;
}

/* The host loop over in[0, n), 0 < n < 2^31: record[k] and column[k] (column may be null) for pos[0, numPairs), -1 for a position outside [0, n);
 * returns the number of records.  The walk goes cut by cut through the input and hands every position in front of the next cut the cuts so far and
 * the last of them; it ends with the list unless the caller wants the count.  A list that is not non-decreasing gets unspecified values: a position
 * is only ever compared, never used as an index */
static size_t locateOnHost(const unsigned char *in, size_t n, const unsigned int *cls, unsigned int flags, const int *pos, size_t numPairs, int *record,
                           int *column, bool wantCount)
{
    size_t cuts = 0, j = 0;
    int last = 0;                                                          /* the largest cut so far; 0: none */
    const auto emit = [&](size_t k) {
        const int p = pos[k];
        const bool inside = p >= 0 && (size_t)p < n;
        record[k] = inside ? (int)cuts : -1;
        if (column) column[k] = inside ? p - last : -1;
    };
    bool a = inClass(cls, in[0]);                                          /* the byte in front of c is a delimiter */
    for (size_t c = 1; c < n && (j < numPairs || wantCount); c++) {
        while (j < numPairs && (pos[j] < 0 || (size_t)pos[j] < c)) emit(j++);
        const bool b = inClass(cls, in[c]);
        if (isCut(flags, a, b)) {
            cuts++;
            last = (int)c;
        }
        a = b;
    }
    while (j < numPairs) emit(j++);
    return cuts + 1;
}

/* what both scan forms check of their own arguments (pfac_host.h: scanForm) */
static bool matchLocatedArgsOk(const int *record, size_t locCapacity, unsigned int flags)
{
    return !(locCapacity && !record) && !(flags & ~(PFACX_SPLIT_BEFORE | PFACX_SPLIT_RUNS));
}

/* the device passes over a list (the caller holds the lock and has checked the module) */
static PFAC_status_t locateOnDevice(PFAC_context *c, const char *d_input, size_t size, const unsigned int *h_class, unsigned int flags, const int *d_pos,
                                    size_t numPairs, int *d_record, int *d_column, size_t *records)
{
    PFACX_locateRun_t run{d_input, size, {}, flags, d_pos, numPairs, d_record, d_column};
    ByteClass(h_class).copyTo(run.cls);
    return c->locate_run_ptr(c, &run, records);
}

} // namespace pfac_internal
using namespace pfac_internal;

extern "C" {

PFAC_status_t PFACX_locatePairsFromDevice(PFAC_handle_t handle, const char *d_input, size_t size, const unsigned int *h_class, unsigned int flags,
                                          const int *d_pos, size_t numPairs, int *d_record, int *d_column, size_t *h_numRecords)
{
    const PFAC_status_t st = checkLocateArgs(handle, d_input, size, flags, d_pos, numPairs, d_record);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0) {
        if (h_numRecords) *h_numRecords = 0;
        return PFAC_STATUS_SUCCESS;
    }
    if (lacksModule(handle)) return PFAC_STATUS_LIB_NOT_EXIST;
    if (numPairs == 0 && !h_numRecords) return PFAC_STATUS_SUCCESS;
    std::lock_guard<std::mutex> guard(handle->lock);
    size_t records = 0;
    const PFAC_status_t ran = locateOnDevice(handle, d_input, size, h_class, flags, d_pos, numPairs, d_record, d_column, &records);
    if (ran == PFAC_STATUS_SUCCESS && h_numRecords) *h_numRecords = records;
    return ran;
}

PFAC_status_t PFACX_locatePairsFromHost(PFAC_handle_t handle, const char *h_input, size_t size, const unsigned int *h_class, unsigned int flags,
                                        const int *h_pos, size_t numPairs, int *h_record, int *h_column, size_t *h_numRecords)
{
    const PFAC_status_t st = checkLocateArgs(handle, h_input, size, flags, h_pos, numPairs, h_record);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0) {
        if (h_numRecords) *h_numRecords = 0;
        return PFAC_STATUS_SUCCESS;
    }
    if (numPairs == 0 && !h_numRecords) return PFAC_STATUS_SUCCESS;
    const ByteClass cls(h_class);
    std::lock_guard<std::mutex> guard(handle->lock);
    const size_t records = locateOnHost(reinterpret_cast<const unsigned char *>(h_input), size, cls.words, flags, h_pos, numPairs, h_record, h_column,
                                        h_numRecords != nullptr);
    if (h_numRecords) *h_numRecords = records;
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_matchLocatedFromDevice(PFAC_handle_t handle, char *d_input, size_t size, const unsigned int *h_class, unsigned int flags, int *d_ids,
                                           int *d_pos, int *d_record, int *d_column, size_t locCapacity, int *h_num_matched)
{
    return scanForm<DevicePairs>(handle, d_input, size, d_ids, d_pos, matchLocatedArgsOk(d_record, locCapacity, flags), locCapacity, h_num_matched,
                          [&](size_t located) {
                              size_t records = 0;
                              return locateOnDevice(handle, d_input, size, h_class, flags, d_pos, located, d_record, d_column, &records);
                          });
}

PFAC_status_t PFACX_matchLocatedFromHost(PFAC_handle_t handle, char *h_input, size_t size, const unsigned int *h_class, unsigned int flags, int *h_ids,
                                         int *h_pos, int *h_record, int *h_column, size_t locCapacity, int *h_num_matched)
{
    return scanForm<PinnedPairs>(handle, h_input, size, h_ids, h_pos, matchLocatedArgsOk(h_record, locCapacity, flags), locCapacity, h_num_matched,
                        [&](size_t located) {
                            (void)locateOnHost(reinterpret_cast<const unsigned char *>(h_input), size, ByteClass(h_class).words, flags, h_pos, located,
                                               h_record, h_column, false);
                            return PFAC_STATUS_SUCCESS;
                        });
}

} /* extern "C" */
