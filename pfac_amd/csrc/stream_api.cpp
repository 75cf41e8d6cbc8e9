/*
 * stream_api.cpp -- PFACX_streamOpen / Reset / Close / MatchFromDevice / MatchFromHost / Flush (include/pfac_ext.h): input that
 * arrives in pieces, occurrences that straddle two pieces included.
 *
 * With M = maxPatternLen, a start position is final once M - 1 bytes behind it have been seen.  A stream keeps the last
 * min(M - 1, T) bytes it has seen (the carry); exactly the positions in the carry are pending, so R = T - carried and no other state
 * is needed.  A piece call reports the carried positions that the piece makes final (the seam: [carry | first M - 1 bytes of the
 * piece], a few KiB at most) and the piece's own positions below size - (M - 1) (the piece in place, its last M - 1 bytes read-ahead
 * only), then carries the last M - 1 bytes on.  The flush reports every carried position with the carry's end as the end of data.
 *   device-fed: the carry lives in two device buffers (the seam launch writes the next one, so a failed call leaves the stream as it
 *               was); seam = scan_stream.hip, piece = the compacted-output path for positions [0, owned) (PFACX_streamReduce).
 *   host-fed:   the carry is host memory, kept as the caller sent it (every match path folds a caseless set's input itself); seam and
 *               piece go through hostLongestPairsLocked, whatever the platform.
 * Every piece and flush call holds the handle's lock from the check of the pattern set to its end (and the stream's own lock: one call
 * at a time per stream), so a set read on another thread cannot slip between a call's halves.
 */
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "pfac_host.h"

struct PFACX_stream_s : pfac_internal::HandleObject {
    int kind = 0;                            /* 0: not fed yet, 1: host calls, 2: device calls */
    unsigned long long total = 0;             /* T: bytes seen */
    size_t carried = 0;                       /* min(M - 1, T): the pending positions are the carried ones */
    std::vector<unsigned char> h_carry;       /* host-fed */
    pfac::DeviceBuffer<char> d_block;         /* device-fed: one allocation = two carry buffers (+ the seam's stage where it does not fit the LDS) */
    char *d_carry[2] = {nullptr, nullptr};
    char *d_stage = nullptr;
    int deviceM = 0;                          /* the maxPatternLen the block was sized for */
    int cur = 0;
    std::mutex lock;                          /* one call at a time per stream */

    void freeDevice()
    {
        d_block.release();
        d_carry[0] = d_carry[1] = d_stage = nullptr;
        deviceM = 0;
    }
    ~PFACX_stream_s() override { freeDevice(); }
    size_t deviceBytes() const override { return d_block.bytes(); }
};

namespace pfac_internal {

static void forget(PFACX_stream_s *s)
{
    s->kind = 0;
    s->total = 0;
    s->carried = 0;
    s->h_carry.clear();
    s->cur = 0;
}

/* the carry buffers of a device-fed stream, sized for the handle's pattern set (only ever resized while nothing is carried) */
static PFAC_status_t ensureStreamDevice(PFACX_stream_s *s, int M)
{
    if (s->d_block && s->deviceM == M) return PFAC_STATUS_SUCCESS;
    s->freeDevice();
    const size_t one = up256((size_t)M - 1);
    const size_t seam = 2 * ((size_t)M - 1);
    const size_t stage = seam > pfac::kStreamSeamLdsBytes ? up256(seam) : 0;
    const PFAC_status_t st = s->d_block.reserve(2 * one + stage + 256);
    if (st != PFAC_STATUS_SUCCESS) return st;
    s->d_carry[0] = s->d_block.get();
    s->d_carry[1] = s->d_block.get() + one + 128;
    s->d_stage = stage ? s->d_block.get() + 2 * one + 256 : nullptr;
    s->deviceM = M;
    return PFAC_STATUS_SUCCESS;
}

/* how a piece of `size` bytes splits the work: of the positions [R, T + size) the first `finalAll` are final; `seam` of them are carried */
StreamSplit streamSplitOf(size_t carried, size_t size, size_t M)
{
    const size_t all = carried + size;
    const size_t finalAll = all >= M - 1 ? all - (M - 1) : 0;
    StreamSplit sp;
    sp.seam = finalAll < carried ? finalAll : carried;
    sp.owned = finalAll - sp.seam;
    return sp;
}

PFAC_status_t hostPiece(PFAC_context *c, const unsigned char *carry, size_t carried, char *piece, size_t size, bool flush, int *ids, int *pos,
                        std::vector<unsigned char> &next, int *count)
{
    const size_t M = (size_t)c->fa.maxPatternLen;
    StreamSplit sp = streamSplitOf(carried, size, M);
    if (flush) { sp.seam = carried; sp.owned = 0; }
    const size_t head = std::min(size, M - 1);
    int seamPairs = 0, piecePairs = 0;
    if (sp.seam) {
        /* [carry | head of the piece], at most 2 (M - 1) bytes, with a result entry per byte: more than the caller's arrays need hold */
        std::vector<unsigned char> seam(carried + head);
        std::vector<int> seamIds(seam.size()), seamPos(seam.size());
        std::memcpy(seam.data(), carry, carried);
        if (head) std::memcpy(seam.data() + carried, piece, head);
        const PFAC_status_t st = hostLongestPairsLocked(c, reinterpret_cast<char *>(seam.data()), sp.seam, seam.size(), -(int)carried, seamIds.data(),
                                                        seamPos.data(), &seamPairs);
        if (st != PFAC_STATUS_SUCCESS) return st;
        std::copy_n(seamIds.data(), seamPairs, ids);
        std::copy_n(seamPos.data(), seamPairs, pos);
    }
    if (sp.owned) {
        const PFAC_status_t st = hostLongestPairsLocked(c, piece, sp.owned, size, 0, ids + seamPairs, pos + seamPairs, &piecePairs);
        if (st != PFAC_STATUS_SUCCESS) return st;
    }
    const size_t nextCarried = flush ? 0 : std::min(M - 1, carried + size);
    next.resize(nextCarried);
    const size_t fromPiece = std::min(nextCarried, size);
    if (nextCarried > fromPiece) std::memcpy(next.data(), carry + (carried - (nextCarried - fromPiece)), nextCarried - fromPiece);
    if (fromPiece) std::memcpy(next.data() + (nextCarried - fromPiece), piece + (size - fromPiece), fromPiece);
    *count = seamPairs + piecePairs;
    return PFAC_STATUS_SUCCESS;
}

} // namespace pfac_internal
using namespace pfac_internal;

extern "C" {

PFAC_status_t PFACX_streamOpen(PFAC_handle_t handle, PFACX_stream_t *stream)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!stream) return PFAC_STATUS_INVALID_PARAMETER;
    *stream = nullptr;
    return adoptNew(handle, stream, [](PFACX_stream_s &) { return PFAC_STATUS_SUCCESS; });
}

PFAC_status_t PFACX_streamReset(PFACX_stream_t stream)
{
    if (!stream || !stream->handle) return PFAC_STATUS_INVALID_HANDLE;
    std::lock_guard<std::mutex> own(stream->lock);
    std::lock_guard<std::mutex> guard(stream->handle->lock);
    forget(stream);
    stream->generation = stream->handle->setGeneration;
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_streamClose(PFACX_stream_t stream) { return closeObject(stream); }

PFAC_status_t PFACX_streamMatchFromDevice(PFACX_stream_t stream, char *d_piece, size_t size, int *d_ids, int *d_pos, size_t capacity,
                                          int *h_num_matched, unsigned long long *h_pieceOffset)
{
    if (!stream || !stream->handle) return PFAC_STATUS_INVALID_HANDLE;
    std::lock_guard<std::mutex> own(stream->lock);
    std::lock_guard<std::mutex> guard(stream->handle->lock);      /* one lock around the set's check, M, seam and piece */
    PFAC_status_t st = checkSetGeneration(stream->handle, stream->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    PFAC_context *c = stream->handle;
    if (!d_piece || !d_ids || !d_pos || !h_num_matched || !h_pieceOffset) return PFAC_STATUS_INVALID_PARAMETER;
    if (size == 0) { *h_num_matched = 0; *h_pieceOffset = stream->total; return PFAC_STATUS_SUCCESS; }
    const size_t M = (size_t)c->fa.maxPatternLen;
    if (capacity < size || capacity - size < M) return PFAC_STATUS_INVALID_PARAMETER;
    if (stream->kind == 1) return PFAC_STATUS_INVALID_PARAMETER;           /* a host-fed stream */
    if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    if (size > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    correctTextureMode(c);                                                 /* (a piece that has only a seam resolves it too) */
    const StreamSplit sp = streamSplitOf(stream->carried, size, M);
    int seamPairs = 0, piecePairs = 0;
    size_t nextCarried = 0;
    if (M > 1) {
        st = ensureStreamDevice(stream, (int)M);
        if (st != PFAC_STATUS_SUCCESS) return st;
        /* the seam: the carried positions this piece makes final, and the next carry into the other buffer */
        st = c->stream_seam_ptr(c, stream->d_carry[stream->cur], stream->carried, d_piece, size, sp.seam, stream->d_carry[stream->cur ^ 1],
                                stream->d_stage, d_ids, d_pos, &seamPairs);
        if (st != PFAC_STATUS_SUCCESS) return st;
        nextCarried = std::min(M - 1, stream->carried + size);
    }
    if (sp.owned) {
        /* the piece in place (a caseless set: its fold, as in every device call), output behind the seam's pairs; a piece shorter than
         * M - 1 has nothing final and never gets here */
        DeviceScan scan;
        st = beginDeviceScan(c, d_piece, size, &scan);
        if (st != PFAC_STATUS_SUCCESS) return st;
        st = c->stream_reduce_ptr(c, reinterpret_cast<int *>(scan.d_scan), (int)sp.owned, (int)size, d_ids + seamPairs, d_pos + seamPairs, &piecePairs,
                                  scan.hashed);
        if (st != PFAC_STATUS_SUCCESS) return st;
    }
    *h_num_matched = seamPairs + piecePairs;
    *h_pieceOffset = stream->total;
    stream->kind = 2;
    stream->total += size;
    stream->carried = nextCarried;
    if (M > 1) stream->cur ^= 1;
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_streamMatchFromHost(PFACX_stream_t stream, char *h_piece, size_t size, int *h_ids, int *h_pos, size_t capacity,
                                        int *h_num_matched, unsigned long long *h_pieceOffset)
{
    if (!stream || !stream->handle) return PFAC_STATUS_INVALID_HANDLE;
    std::lock_guard<std::mutex> own(stream->lock);
    std::lock_guard<std::mutex> guard(stream->handle->lock);      /* one lock around the set's check, M, seam and piece */
    PFAC_status_t st = checkSetGeneration(stream->handle, stream->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    PFAC_context *c = stream->handle;
    if (!h_piece || !h_ids || !h_pos || !h_num_matched || !h_pieceOffset) return PFAC_STATUS_INVALID_PARAMETER;
    if (size == 0) { *h_num_matched = 0; *h_pieceOffset = stream->total; return PFAC_STATUS_SUCCESS; }
    const size_t M = (size_t)c->fa.maxPatternLen;
    if (capacity < size || capacity - size < M) return PFAC_STATUS_INVALID_PARAMETER;
    if (size > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    if (stream->kind == 2) return PFAC_STATUS_INVALID_PARAMETER;           /* a device-fed stream */
    const bool gpu = c->platform == PFAC_PLATFORM_GPU;
    if (gpu && lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    int pairs = 0;
    try {
        std::vector<unsigned char> next;                       /* the stream changes when the whole call has succeeded */
        st = hostPiece(c, stream->h_carry.data(), stream->carried, h_piece, size, false, h_ids, h_pos, next, &pairs);
        if (st != PFAC_STATUS_SUCCESS) return st;
        stream->h_carry.swap(next);
        stream->carried = stream->h_carry.size();
    } catch (const std::bad_alloc &) { return PFAC_STATUS_ALLOC_FAILED; }
    *h_num_matched = pairs;
    *h_pieceOffset = stream->total;
    stream->kind = 1;
    stream->total += size;
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_streamFlush(PFACX_stream_t stream, int *ids, int *pos, size_t capacity, int *h_num_matched)
{
    if (!stream || !stream->handle) return PFAC_STATUS_INVALID_HANDLE;
    std::lock_guard<std::mutex> own(stream->lock);
    std::lock_guard<std::mutex> guard(stream->handle->lock);      /* one lock around the set's check, M, seam and piece */
    PFAC_status_t st = checkSetGeneration(stream->handle, stream->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    PFAC_context *c = stream->handle;
    if (!ids || !pos || !h_num_matched) return PFAC_STATUS_INVALID_PARAMETER;
    const size_t M = (size_t)c->fa.maxPatternLen;
    if (capacity < M) return PFAC_STATUS_INVALID_PARAMETER;
    const size_t carried = stream->carried;
    int pairs = 0;
    if (carried && stream->kind == 2) {
        if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
        st = c->stream_seam_ptr(c, stream->d_carry[stream->cur], carried, nullptr, 0, carried, stream->d_carry[stream->cur ^ 1], stream->d_stage, ids, pos,
                                &pairs);
        if (st != PFAC_STATUS_SUCCESS) return st;
    } else if (carried && stream->kind == 1) {
        if (hostLacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
        try {
            std::vector<unsigned char> none;
            st = hostPiece(c, stream->h_carry.data(), carried, nullptr, 0, true, ids, pos, none, &pairs);
        } catch (const std::bad_alloc &) { return PFAC_STATUS_ALLOC_FAILED; }
        if (st != PFAC_STATUS_SUCCESS) return st;
    }
    *h_num_matched = pairs;
    forget(stream);
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
