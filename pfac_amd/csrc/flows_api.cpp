/*
 * flows_api.cpp -- PFACX_flowsOpen / Close / Reset / MatchFromDevice / MatchFromHost / Flush (include/pfac_ext.h): many streams
 * (stream_api.cpp) advanced by one call, occurrences that straddle two batches included.
 *
 * A flow set keeps, per flow, what a stream keeps: T (bytes seen), the number of carried bytes (min(M - 1, T): exactly the pending
 * positions) and where the carry is.  All of that lives on the HOST -- the call needs the piece sizes there anyway to cut the work --
 * and the carried bytes themselves live where the set is fed from:
 *   device-fed: ONE allocation of 2 x numFlows carry buffers; a call's seam launch (scan_flows.hip) reads a flow's current buffer and
 *               writes its next carry into the other one, and the host flips the flows of the call after the call has succeeded -- a
 *               failed call leaves every flow as it was.  The pieces are scanned in place by ONE compacted scan of the whole buffer
 *               (reduceOnDevice: whatever kernel variant, walker, perf mode and fold the handle selects), not launched at all when no
 *               piece is longer than M - 1 bytes; the seams and the merge of both lists run behind it (PFACX_flowsRun).  The piece
 *               descriptors are built in pinned host memory and uploaded asynchronously in front of the scan.  The host waits
 *               twice: for the scan's count (which sizes the staging list) and for the end of the merge.  The scan uses the
 *               caller's arrays below `size` as its pair list, like every compacted call; the merge writes nothing at or beyond
 *               the total.
 *   host-fed:   a vector per flow; the pieces go one by one through what a host-fed stream's call goes through (hostPiece, stream_api.cpp:
 *               hostLongestPairsLocked, whatever the platform), into the caller's arrays at the running count, and the next carries are
 *               kept aside until the last piece has succeeded.
 * Every piece and flush call holds the set's own lock and the handle's lock from the check of the pattern set to its end.
 */
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "pfac_host.h"

namespace {
struct Flow {
    unsigned long long total = 0;             /* T: bytes seen */
    uint32_t carried = 0;                     /* min(M - 1, T) */
    uint32_t cur = 0;                         /* device-fed: which of the flow's two carry buffers is current */
    std::vector<unsigned char> h_carry;       /* host-fed */
};
}

struct PFACX_flows_s : pfac_internal::HandleObject {
    int kind = 0;                            /* 0: not fed yet, 1: host calls, 2: device calls */
    std::vector<Flow> flows;
    std::vector<unsigned int> named;          /* per flow: the number of the last call that named it (a flow named twice) */
    unsigned int callNo = 0;
    pfac::DeviceBuffer<char> d_carries;       /* device-fed: buffer b of flow f at (2 f + b) * carryStride */
    size_t carryStride = 0;
    int deviceM = 0;                          /* the maxPatternLen the carries were sized for */
    std::mutex lock;                          /* one call at a time per set */

    void freeDevice()
    {
        d_carries.release();
        deviceM = 0;
    }
    ~PFACX_flows_s() override { freeDevice(); }
    size_t deviceBytes() const override { return d_carries.bytes(); }
};

using namespace pfac_internal;

namespace {

void forget(Flow &f)
{
    f.total = 0;
    f.carried = 0;
    f.cur = 0;
    std::vector<unsigned char>().swap(f.h_carry);
}

/* every id below numFlows, no flow twice */
bool idsValid(PFACX_flows_s *s, const unsigned int *ids, size_t n)
{
    s->callNo = s->callNo + 1u ? s->callNo + 1u : 1u;
    if (s->callNo == 1u) std::fill(s->named.begin(), s->named.end(), 0u);
    for (size_t k = 0; k < n; k++) {
        if (ids[k] >= s->flows.size() || s->named[ids[k]] == s->callNo) return false;
        s->named[ids[k]] = s->callNo;
    }
    return true;
}

/* the carries of a device-fed set, sized for the handle's pattern set (only ever resized while nothing is carried: a set of another M
 * is refused until every flow has been reset) */
PFAC_status_t ensureCarries(PFACX_flows_s *s, size_t M)
{
    if (M <= 1 || (s->d_carries && s->deviceM == (int)M)) return PFAC_STATUS_SUCCESS;
    s->freeDevice();
    const size_t stride = ((M - 1) + 15) & ~size_t(15);
    if (s->flows.size() > (SIZE_MAX - 256) / (2 * stride)) return PFAC_STATUS_ALLOC_FAILED;
    if (s->d_carries.reserve(2 * stride * s->flows.size() + 256) != PFAC_STATUS_SUCCESS) return PFAC_STATUS_ALLOC_FAILED;
    s->carryStride = stride;
    s->deviceM = (int)M;
    return PFAC_STATUS_SUCCESS;
}

/* room for P piece descriptors in the handle's pinned host memory (the caller fills them) and on the device */
PFAC_status_t stagePieces(PFAC_context *c, size_t P, PFACX_flowPiece_t **h_pieces)
{
    const size_t bytes = P * sizeof(PFACX_flowPiece_t);
    if (c->h_flowPiecesBytes < bytes) {
        if (c->h_flowPieces) (void)hipHostFree(c->h_flowPieces);
        c->h_flowPieces = nullptr;
        c->h_flowPiecesBytes = 0;
        if (hipHostMalloc(&c->h_flowPieces, bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            c->h_flowPieces = nullptr;
            return PFAC_STATUS_ALLOC_FAILED;
        }
        c->h_flowPiecesBytes = bytes;
    }
    const PFAC_status_t st = c->scratch.flowPieces.reserve(bytes);
    if (st != PFAC_STATUS_SUCCESS) return st;
    *h_pieces = static_cast<PFACX_flowPiece_t *>(c->h_flowPieces);
    return PFAC_STATUS_SUCCESS;
}

/* ... on their way to the device, on the default stream: in front of the scan, read by the launches behind it */
PFAC_status_t uploadPieces(PFAC_context *c, size_t P)
{
    return hipMemcpyAsync(c->scratch.flowPieces.get(), c->h_flowPieces, P * sizeof(PFACX_flowPiece_t), hipMemcpyHostToDevice, nullptr) == hipSuccess
               ? PFAC_STATUS_SUCCESS : PFAC_STATUS_INTERNAL_ERROR;
}

/* the seams and the merge of a device call or flush behind uploadPieces: the handle's flows scratch cut into what PFACX_flowsRun reads
 * and writes, the scan's scanCount ordered pairs (at d_ids / d_pos) copied aside; *total = the number of pairs */
PFAC_status_t runOnDevice(PFACX_flows_s *s, const char *d_input, size_t P, size_t sumFinal, size_t scanCount,
                          int *d_ids, int *d_pos, size_t capacity, int *d_first, int *total)
{
    PFAC_context *c = s->handle;
    const size_t M = (size_t)c->fa.maxPatternLen;
    const size_t blocks = (P + 255) / 256;
    const size_t stageStride = 2 * (M - 1) > pfac::kStreamSeamLdsBytes ? up256(2 * (M - 1)) : 0;
    const size_t oSeamCount = 0;
    const size_t oPairLo = oSeamCount + up256(P * 4);
    const size_t oCounts = oPairLo + up256(P * 4);
    const size_t oSums = oCounts + up256(P * 4);
    const size_t oSeamIds = oSums + up256((blocks + 2) * 4);
    const size_t oSeamPos = oSeamIds + up256(sumFinal * 4);
    const size_t oScanIds = oSeamPos + up256(sumFinal * 4);
    const size_t oScanPos = oScanIds + up256(scanCount * 4);
    const size_t oStage = oScanPos + up256(scanCount * 4);
    if (stageStride && P > (SIZE_MAX / 2 - oStage) / stageStride) return PFAC_STATUS_ALLOC_FAILED;
    const size_t bytes = oStage + P * stageStride;
    PFAC_status_t st = c->scratch.flows.reserve(bytes ? bytes : 256);
    if (st != PFAC_STATUS_SUCCESS) return st;
    char *base = c->scratch.flows.get();
    if (scanCount &&
        (hipMemcpyAsync(base + oScanIds, d_ids, scanCount * 4, hipMemcpyDeviceToDevice, nullptr) != hipSuccess ||
         hipMemcpyAsync(base + oScanPos, d_pos, scanCount * 4, hipMemcpyDeviceToDevice, nullptr) != hipSuccess))
        return PFAC_STATUS_INTERNAL_ERROR;
    PFACX_flowsRun_t run;
    run.d_input = d_input;
    run.d_pieces = reinterpret_cast<const PFACX_flowPiece_t *>(c->scratch.flowPieces.get());
    run.numPieces = P;
    run.d_carries = s->d_carries.get();
    run.carryStride = s->carryStride;
    run.d_stage = stageStride ? base + oStage : nullptr;
    run.stageStride = stageStride;
    run.d_seamIds = reinterpret_cast<int *>(base + oSeamIds);
    run.d_seamPos = reinterpret_cast<int *>(base + oSeamPos);
    run.d_seamCount = reinterpret_cast<unsigned int *>(base + oSeamCount);
    run.d_pairLo = reinterpret_cast<unsigned int *>(base + oPairLo);
    run.d_counts = reinterpret_cast<unsigned int *>(base + oCounts);
    run.d_blockSums = reinterpret_cast<unsigned int *>(base + oSums);
    run.d_scanIds = reinterpret_cast<const int *>(base + oScanIds);
    run.d_scanPos = reinterpret_cast<const int *>(base + oScanPos);
    run.scanCount = scanCount;
    run.d_ids = d_ids;
    run.d_pos = d_pos;
    run.capacity = capacity;
    run.d_pieceFirst = d_first;
    return c->flows_run_ptr(c, &run, total);
}

/* the argument checks both piece calls share (the caller holds both locks) */
PFAC_status_t checkPieces(PFACX_flows_s *s, const void *input, size_t size, const size_t *h_offsets, const unsigned int *h_flowIds, size_t numPieces,
                          const int *ids, const int *pos, size_t capacity, const int *pieceFirst, const unsigned long long *h_pieceOffsets,
                          const int *h_num_matched)
{
    const PFAC_status_t st = checkSetGeneration(s->handle, s->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (!input || !h_offsets || !ids || !pos || !pieceFirst || !h_num_matched || (numPieces && (!h_flowIds || !h_pieceOffsets))) return PFAC_STATUS_INVALID_PARAMETER;
    if (numPieces == 0) return size == 0 ? PFAC_STATUS_SUCCESS : PFAC_STATUS_INVALID_PARAMETER;
    const size_t M = (size_t)s->handle->fa.maxPatternLen;
    if (size >= (size_t)0x80000000u || numPieces >= (size_t)0x80000000u || !batchOffsetsValid(h_offsets, numPieces, size)) return PFAC_STATUS_INVALID_PARAMETER;
    const unsigned long long need = (unsigned long long)size + (unsigned long long)numPieces * (M - 1);
    if (need >= 0x80000000ull || capacity < need) return PFAC_STATUS_INVALID_PARAMETER;
    if (!idsValid(s, h_flowIds, numPieces)) return PFAC_STATUS_INVALID_PARAMETER;
    return PFAC_STATUS_SUCCESS;
}

} // namespace

extern "C" {

PFAC_status_t PFACX_flowsOpen(PFAC_handle_t handle, size_t numFlows, PFACX_flows_t *flows)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!flows) return PFAC_STATUS_INVALID_PARAMETER;
    *flows = nullptr;
    if (numFlows == 0 || numFlows >= (size_t)0x80000000u) return PFAC_STATUS_INVALID_PARAMETER;
    return adoptNew(handle, flows, [numFlows](PFACX_flows_s &s) {
        s.flows.resize(numFlows);
        s.named.assign(numFlows, 0u);
        return PFAC_STATUS_SUCCESS;
    });
}

PFAC_status_t PFACX_flowsClose(PFACX_flows_t flows) { return closeObject(flows); }

PFAC_status_t PFACX_flowsReset(PFACX_flows_t flows, const unsigned int *h_flowIds, size_t n)
{
    if (!flows || !flows->handle) return PFAC_STATUS_INVALID_HANDLE;
    std::lock_guard<std::mutex> own(flows->lock);
    std::lock_guard<std::mutex> guard(flows->handle->lock);
    if (!h_flowIds && n == 0) {
        for (Flow &f : flows->flows) forget(f);
        flows->kind = 0;
        flows->generation = flows->handle->setGeneration;
        return PFAC_STATUS_SUCCESS;
    }
    if (!h_flowIds) return PFAC_STATUS_INVALID_PARAMETER;
    for (size_t k = 0; k < n; k++) if (h_flowIds[k] >= flows->flows.size()) return PFAC_STATUS_INVALID_PARAMETER;
    for (size_t k = 0; k < n; k++) forget(flows->flows[h_flowIds[k]]);
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_flowsMatchFromDevice(PFACX_flows_t flows, char *d_input, size_t size, const size_t *h_offsets, const unsigned int *h_flowIds,
                                         size_t numPieces, int *d_ids, int *d_pos, size_t capacity, int *d_pieceFirst,
                                         unsigned long long *h_pieceOffsets, int *h_num_matched)
{
    if (!flows || !flows->handle) return PFAC_STATUS_INVALID_HANDLE;
    std::lock_guard<std::mutex> own(flows->lock);
    std::lock_guard<std::mutex> guard(flows->handle->lock);
    PFAC_context *c = flows->handle;
    PFAC_status_t st = checkPieces(flows, d_input, size, h_offsets, h_flowIds, numPieces, d_ids, d_pos, capacity, d_pieceFirst, h_pieceOffsets, h_num_matched);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (numPieces == 0) { *h_num_matched = 0; return PFAC_STATUS_SUCCESS; }
    if (size && flows->kind == 1) return PFAC_STATUS_INVALID_PARAMETER;          /* a host-fed set */
    if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    correctTextureMode(c);                                                       /* (a call whose pieces have only seams resolves it too) */
    const size_t M = (size_t)c->fa.maxPatternLen;
    st = ensureCarries(flows, M);
    if (st != PFAC_STATUS_SUCCESS) return st;
    int total = 0;
    try {
        PFACX_flowPiece_t *pieces = nullptr;
        st = stagePieces(c, numPieces, &pieces);
        if (st != PFAC_STATUS_SUCCESS) return st;
        size_t sumFinal = 0;
        bool anyOwned = false;
        for (size_t k = 0; k < numPieces; k++) {
            const Flow &f = flows->flows[h_flowIds[k]];
            const size_t len = h_offsets[k + 1] - h_offsets[k];
            PFACX_flowPiece_t &d = pieces[k];
            d = PFACX_flowPiece_t{};
            d.start = (unsigned int)h_offsets[k];
            d.flow = h_flowIds[k];
            d.seamOff = (unsigned int)sumFinal;
            if (len) {                                                          /* an empty piece touches nothing: no seam, no carry */
                const StreamSplit sp = streamSplitOf(f.carried, len, M);
                d.len = (unsigned int)len;
                d.carried = f.carried;
                d.numFinal = (unsigned int)sp.seam;
                d.cur = f.cur;
                sumFinal += sp.seam;
                anyOwned = anyOwned || sp.owned != 0;
            }
        }
        /* the pieces in place: one compacted scan of the whole buffer (a caseless set: of its fold), its ordered pairs at d_ids / d_pos */
        st = uploadPieces(c, numPieces);
        if (st != PFAC_STATUS_SUCCESS) return st;
        int scanCount = 0;
        if (anyOwned) {
            DeviceScan scan;
            st = beginDeviceScan(c, d_input, size, &scan);
            if (st == PFAC_STATUS_SUCCESS) st = reduceOnDevice(c, scan.d_scan, size, d_ids, d_pos, true, &scanCount);
            if (st != PFAC_STATUS_SUCCESS) return st;
        }
        st = runOnDevice(flows, d_input, numPieces, sumFinal, (size_t)scanCount, d_ids, d_pos, capacity, d_pieceFirst, &total);
        if (st != PFAC_STATUS_SUCCESS) return st;
    } catch (const std::bad_alloc &) { return PFAC_STATUS_ALLOC_FAILED; }
    /* success: the flows move on */
    for (size_t k = 0; k < numPieces; k++) {
        Flow &f = flows->flows[h_flowIds[k]];
        const size_t len = h_offsets[k + 1] - h_offsets[k];
        h_pieceOffsets[k] = f.total;
        if (!len) continue;
        f.total += len;
        f.carried = (uint32_t)std::min(M - 1, (size_t)f.carried + len);
        if (M > 1) f.cur ^= 1u;
    }
    if (size) flows->kind = 2;
    *h_num_matched = total;
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_flowsMatchFromHost(PFACX_flows_t flows, char *h_input, size_t size, const size_t *h_offsets, const unsigned int *h_flowIds,
                                       size_t numPieces, int *h_ids, int *h_pos, size_t capacity, int *h_pieceFirst,
                                       unsigned long long *h_pieceOffsets, int *h_num_matched)
{
    if (!flows || !flows->handle) return PFAC_STATUS_INVALID_HANDLE;
    std::lock_guard<std::mutex> own(flows->lock);
    std::lock_guard<std::mutex> guard(flows->handle->lock);
    PFAC_context *c = flows->handle;
    PFAC_status_t st = checkPieces(flows, h_input, size, h_offsets, h_flowIds, numPieces, h_ids, h_pos, capacity, h_pieceFirst, h_pieceOffsets, h_num_matched);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (numPieces == 0) { *h_num_matched = 0; return PFAC_STATUS_SUCCESS; }
    if (size && flows->kind == 2) return PFAC_STATUS_INVALID_PARAMETER;          /* a device-fed set */
    if (hostLacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    int at = 0;
    try {
        std::vector<std::vector<unsigned char>> next(numPieces);                /* the flows change when the whole call has succeeded */
        for (size_t k = 0; k < numPieces; k++) {
            const size_t len = h_offsets[k + 1] - h_offsets[k];
            h_pieceFirst[k] = at;
            if (!len) continue;
            int n = 0;
            const Flow &f = flows->flows[h_flowIds[k]];
            st = hostPiece(c, f.h_carry.data(), f.carried, h_input + h_offsets[k], len, false, h_ids + at, h_pos + at, next[k], &n);
            if (st != PFAC_STATUS_SUCCESS) return st;
            at += n;
        }
        h_pieceFirst[numPieces] = at;
        for (size_t k = 0; k < numPieces; k++) {
            Flow &f = flows->flows[h_flowIds[k]];
            const size_t len = h_offsets[k + 1] - h_offsets[k];
            h_pieceOffsets[k] = f.total;
            if (!len) continue;
            f.total += len;
            f.carried = (uint32_t)next[k].size();
            f.h_carry.swap(next[k]);
        }
    } catch (const std::bad_alloc &) { return PFAC_STATUS_ALLOC_FAILED; }
    if (size) flows->kind = 1;
    *h_num_matched = at;
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_flowsFlush(PFACX_flows_t flows, const unsigned int *h_flowIds, size_t n, int *ids, int *pos, size_t capacity, int *first,
                               int *h_num_matched)
{
    if (!flows || !flows->handle) return PFAC_STATUS_INVALID_HANDLE;
    std::lock_guard<std::mutex> own(flows->lock);
    std::lock_guard<std::mutex> guard(flows->handle->lock);
    PFAC_context *c = flows->handle;
    PFAC_status_t st = checkSetGeneration(c, flows->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (!ids || !pos || !first || !h_num_matched || (n && !h_flowIds)) return PFAC_STATUS_INVALID_PARAMETER;
    const size_t M = (size_t)c->fa.maxPatternLen;
    if (n >= (size_t)0x80000000u) return PFAC_STATUS_INVALID_PARAMETER;
    const unsigned long long need = std::max<unsigned long long>(1, (unsigned long long)n * (M - 1));
    if (need >= 0x80000000ull || capacity < need) return PFAC_STATUS_INVALID_PARAMETER;
    if (!idsValid(flows, h_flowIds, n)) return PFAC_STATUS_INVALID_PARAMETER;
    int total = 0;
    try {
        if (flows->kind == 2 && n) {
            if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
            st = ensureCarries(flows, M);
            if (st != PFAC_STATUS_SUCCESS) return st;
            PFACX_flowPiece_t *pieces = nullptr;
            st = stagePieces(c, n, &pieces);
            if (st != PFAC_STATUS_SUCCESS) return st;
            size_t sumFinal = 0;
            for (size_t k = 0; k < n; k++) {
                const Flow &f = flows->flows[h_flowIds[k]];
                PFACX_flowPiece_t &d = pieces[k];
                d = PFACX_flowPiece_t{};
                d.flow = h_flowIds[k];
                d.carried = d.numFinal = f.carried;                                /* every carried position, the carry's end the end of the data */
                d.seamOff = (unsigned int)sumFinal;
                d.cur = f.cur;
                sumFinal += f.carried;
            }
            st = uploadPieces(c, n);
            if (st == PFAC_STATUS_SUCCESS) st = runOnDevice(flows, nullptr, n, sumFinal, 0, ids, pos, capacity, first, &total);
            if (st != PFAC_STATUS_SUCCESS) return st;
        } else if (flows->kind == 1) {
            if (hostLacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
            std::vector<unsigned char> none;
            for (size_t k = 0; k < n; k++) {
                first[k] = total;
                const Flow &f = flows->flows[h_flowIds[k]];
                if (!f.carried) continue;
                int got = 0;
                st = hostPiece(c, f.h_carry.data(), f.carried, nullptr, 0, true, ids + total, pos + total, none, &got);
                if (st != PFAC_STATUS_SUCCESS) return st;
                total += got;
            }
            first[n] = total;
        } else {
            /* nothing has been fed since the set was opened or reset: no pairs; `first` may be host or device memory */
            const std::vector<int> zeros(n + 1, 0);
            if (!c->hasDevice) std::memcpy(first, zeros.data(), zeros.size() * sizeof(int));
            else if (hipMemcpy(first, zeros.data(), zeros.size() * sizeof(int), hipMemcpyDefault) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
        }
    } catch (const std::bad_alloc &) { return PFAC_STATUS_ALLOC_FAILED; }
    for (size_t k = 0; k < n; k++) forget(flows->flows[h_flowIds[k]]);
    *h_num_matched = total;
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
