/*
 * host_pipeline.cpp -- host buffers through the GPU: PFAC_matchFromHost and PFAC_matchFromHostReduce on the GPU platform
 * (ref PFAC/src/PFAC.cpp:879-961, 1010-1128: allocate, upload, scan, download, free, in sequence).  The stream goes through two
 * staging pieces owned by the handle: piece i + 1 uploads while piece i is scanned by the compacted-output kernel, only the
 * (position, id) pairs come back, the zeros of the result vector are written on the host.
 * How the threads of such a call work together -- the cut into pieces, the uploader beside the scans, the zero-fill team and their waits -- is
 * piece_pipeline.h (no HIP in it: tools/tsan_pipeline.cpp runs it under ThreadSanitizer); the HIP calls of a piece are stagedPairs() below, once for
 * both calls, which differ in what they do with a piece's pairs.
 */
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <vector>

#include "pfac_host.h"
#include "piece_pipeline.h"

using pfac::Int2;
using namespace pfac_internal;

namespace pfac_internal {

/* PFAC_matchFromDevice behind the argument checks; the caller holds handle->lock */
PFAC_status_t matchDeviceLocked(PFAC_context *c, char *d_inputString, size_t size, int *d_matched_result)
{
    if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;      /* never a CPU fallback */
    correctTextureMode(c);
    if (c->perfMode == PFAC_TIME_DRIVEN) return c->kernel_time_driven_ptr(c, d_inputString, size, d_matched_result);
    if (c->perfMode == PFAC_SPACE_DRIVEN) return c->kernel_space_driven_ptr(c, d_inputString, size, d_matched_result);
    return PFAC_STATUS_INTERNAL_ERROR;
}

/*
 * Host buffers through the GPU: results for positions [0, owned) of a stream of which `readable` >= owned bytes
 * may be read (walks that start before `owned` may run into the rest: the slices of a sharded stream,
 * omp_PFAC.cpp:324,377).  The caller holds c->lock.
 *
 * The reference allocates, uploads, scans, downloads and frees in sequence (PFAC.cpp:916-960), which leaves the
 * scan idle for the 5 bytes per position that cross the host link.  Here the stream is cut into pieces of
 * kHostPiece positions: piece i+1 is uploaded and piece i-1 downloaded while piece i is scanned (SURVEY 8f
 * rank 2).  Each piece is scanned together with the maxPatternLen bytes behind it -- a walk may read that far --
 * and only its own results go back.  The staging buffers, two copy streams and their events belong to the
 * handle and are created on first use; the scan itself stays on the default stream.
 */
static PFAC_status_t ensureHostStage(PFAC_context *c, size_t need)
{
    pfac::DeviceScratch &s = c->scratch;
    if (s.stagePos[1].count() >= need) return PFAC_STATUS_SUCCESS;      /* the last of the six: a stage is whole or not there */
    freeHostStage(c);
    bool ok = true;
    for (int b = 0; b < 2 && ok; b++) {
        ok = s.stageIn[b].reserve((need + 3) & ~size_t(3)) == PFAC_STATUS_SUCCESS && s.stageOut[b].reserve(need) == PFAC_STATUS_SUCCESS &&
             s.stagePos[b].reserve(need) == PFAC_STATUS_SUCCESS;
        hipEvent_t e[3] = {nullptr, nullptr, nullptr};
        for (int k = 0; k < 3 && ok; k++) ok = hipEventCreateWithFlags(&e[k], hipEventDisableTiming) == hipSuccess;
        c->evUp[b] = e[0]; c->evScan[b] = e[1]; c->evDown[b] = e[2];
    }
    hipStream_t up = nullptr, down = nullptr;
    ok = ok && hipStreamCreateWithFlags(&up, hipStreamNonBlocking) == hipSuccess &&
         hipStreamCreateWithFlags(&down, hipStreamNonBlocking) == hipSuccess;
    c->stageUp = up; c->stageDown = down;
    if (!ok) { (void)hipGetLastError(); freeHostStage(c); return PFAC_STATUS_CUDA_ALLOC_FAILED; }
    return PFAC_STATUS_SUCCESS;
}

/* PFACX_prepare: everything a handle's first PFAC_matchFromHost / PFAC_matchFromHostReduce would otherwise allocate, create or load inside the
 * call (round 5's driver line: first call 103 ms, steady 7 ms): the two staging pieces with their streams and events, the ordering scratch of a
 * piece, the code objects of the compacted-output scan and its ordering launches (one throwaway scan of a piece filled with a byte no pattern
 * starts with), and the runtime's own staging of pageable host memory (one throwaway upload of a pageable piece).  The caller holds c->lock. */
PFAC_status_t prepareHostPath(PFAC_context *c, size_t maxBytes)
{
    if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    const size_t n = PieceCut(maxBytes ? maxBytes : kHostPiece, ~size_t(0), kHostPiece, (size_t)c->fa.maxPatternLen).stageNeed();   /* the longest piece of such a call */
    PFAC_status_t st = ensureHostStage(c, n);
    if (st != PFAC_STATUS_SUCCESS) return st;
    correctTextureMode(c);
    int filler = 0;                                            /* a byte the initial state has no transition on, if there is one: the scan then finds nothing */
    for (int b = 0; b < pfac::kCharSet && (size_t)b < c->h_initialRow.size(); b++)
        if (c->h_initialRow[(size_t)b] == pfac::kTrapState) { filler = b; break; }
    hipStream_t up = static_cast<hipStream_t>(c->stageUp);
    bool ok = true;
    try {
        const std::vector<char> pageable(n, (char)filler);
        ok = hipMemcpyAsync(c->scratch.stageIn[0].get(), pageable.data(), n, hipMemcpyHostToDevice, up) == hipSuccess && hipStreamSynchronize(up) == hipSuccess &&
             hipMemsetAsync(c->scratch.stageIn[1].get(), filler, n, nullptr) == hipSuccess;
    } catch (const std::bad_alloc &) { return PFAC_STATUS_ALLOC_FAILED; }
    if (!ok) { (void)hipGetLastError(); return PFAC_STATUS_INTERNAL_ERROR; }
    for (int b = 0; b < 2 && st == PFAC_STATUS_SUCCESS; b++) {              /* both buffers, the way both host calls use them: pairs in any order / in position order */
        int count = 0;
        st = reduceOnDevice(c, c->scratch.stageIn[b].get(), n, c->scratch.stageOut[b].get(), c->scratch.stagePos[b].get(), /* ordered */ b == 1, &count);
    }
    if (st == PFAC_STATUS_SUCCESS && hipStreamSynchronize(nullptr) != hipSuccess) st = PFAC_STATUS_INTERNAL_ERROR;
    return st;
}

/* every result crosses the link: pieces with many matches */
static PFAC_status_t matchHostFullVector(PFAC_context *c, char *h_inputString, size_t owned, size_t readable, int *h_matched_result)
{
    const PieceCut cut(owned, readable, kHostPiece, (size_t)c->fa.maxPatternLen);
    PFAC_status_t st = ensureHostStage(c, cut.stageNeed());
    if (st != PFAC_STATUS_SUCCESS) return st;
    hipStream_t up = static_cast<hipStream_t>(c->stageUp), down = static_cast<hipStream_t>(c->stageDown);
    bool used[2] = {false, false};
    for (size_t i = 0; i < cut.numPieces() && st == PFAC_STATUS_SUCCESS; i++) {
        const Piece p = cut.at(i);
        const int b = p.buffer;
        char *const d_in = c->scratch.stageIn[b].get();
        int *const d_ids = c->scratch.stageOut[b].get();
        hipEvent_t evUp = static_cast<hipEvent_t>(c->evUp[b]), evScan = static_cast<hipEvent_t>(c->evScan[b]),
                   evDown = static_cast<hipEvent_t>(c->evDown[b]);
        bool ok = true;
        if (used[b]) ok = hipStreamWaitEvent(up, evScan, 0) == hipSuccess;          /* the scan of piece i-2 has read this buffer */
        ok = ok && hipMemcpyAsync(d_in, h_inputString + p.off, p.scanned, hipMemcpyHostToDevice, up) == hipSuccess &&
             hipEventRecord(evUp, up) == hipSuccess && hipStreamWaitEvent(nullptr, evUp, 0) == hipSuccess;
        if (ok && used[b]) ok = hipStreamWaitEvent(nullptr, evDown, 0) == hipSuccess;   /* its results have left this buffer */
        if (!ok) { st = PFAC_STATUS_INTERNAL_ERROR; break; }
        st = foldStaged(c, d_in, p.scanned);                  /* a caseless set: in place, behind the upload */
        if (st != PFAC_STATUS_SUCCESS) break;
        st = matchDeviceLocked(c, d_in, p.scanned, d_ids);
        if (st != PFAC_STATUS_SUCCESS) break;
        ok = hipEventRecord(evScan, nullptr) == hipSuccess && hipStreamWaitEvent(down, evScan, 0) == hipSuccess &&
             hipMemcpyAsync(h_matched_result + p.off, d_ids, p.mine * sizeof(int), hipMemcpyDeviceToHost, down) == hipSuccess &&
             hipEventRecord(evDown, down) == hipSuccess;
        if (!ok) st = PFAC_STATUS_INTERNAL_ERROR;
        used[b] = true;
    }
    const bool drained = hipStreamSynchronize(up) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess &&
                         hipStreamSynchronize(down) == hipSuccess;
    if (!drained && st == PFAC_STATUS_SUCCESS) st = PFAC_STATUS_INTERNAL_ERROR;
    return st;
}

/*
 * The staged compacted scan of a host buffer, what both calls below are built on: the pieces of `cut` go up into stageIn[i & 1] on the upload
 * stream (evUp[i & 1] behind each; by a thread of their own: piece_pipeline.h runPieces), the default stream waits for a piece's event, folds the
 * piece in place (a caseless set) and scans it with the compacted-output kernel, and take(piece, count, d_ids, d_pos) -> status gets its pairs --
 * in position order if `ordered` -- while the next piece is on its way.  A pair whose position is not below piece.mine lies in the read-ahead: it
 * is the next piece's, which finds it again.  Both streams are drained before this returns.  at(Staged) tells a caller with a clock or threads of
 * its own where the call is; nothing is told if the staging buffers cannot be had.
 */
enum class Staged { ready, uploadsBegun, piecesDone, drained };
template <class At, class Take>
static PFAC_status_t stagedPairs(PFAC_context *c, char *h_inputString, const PieceCut &cut, bool ordered, At at, Take take)
{
    PFAC_status_t st = ensureHostStage(c, cut.stageNeed());
    if (st != PFAC_STATUS_SUCCESS) return st;
    correctTextureMode(c);
    hipStream_t up = static_cast<hipStream_t>(c->stageUp);
    at(Staged::ready);
    int device = 0;
    (void)hipGetDevice(&device);
    int count = 0;                                             /* of the piece scanned last */
    st = runPieces(
        cut.numPieces(), [&]() { return hipSetDevice(device) == hipSuccess; },
        [&](size_t i) {
            const Piece p = cut.at(i);
            return hipMemcpyAsync(c->scratch.stageIn[p.buffer].get(), h_inputString + p.off, p.scanned, hipMemcpyHostToDevice, up) == hipSuccess &&
                   hipEventRecord(static_cast<hipEvent_t>(c->evUp[p.buffer]), up) == hipSuccess;
        },
        [&]() { at(Staged::uploadsBegun); },
        [&](size_t i) {
            const Piece p = cut.at(i);
            char *const d_in = c->scratch.stageIn[p.buffer].get();
            if (hipStreamWaitEvent(nullptr, static_cast<hipEvent_t>(c->evUp[p.buffer]), 0) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
            const PFAC_status_t folded = foldStaged(c, d_in, p.scanned);          /* a caseless set: in place, behind the upload */
            if (folded != PFAC_STATUS_SUCCESS) return folded;
            return reduceOnDevice(c, d_in, p.scanned, c->scratch.stageOut[p.buffer].get(), c->scratch.stagePos[p.buffer].get(), ordered, &count);
        },
        [&](size_t i) {
            const Piece p = cut.at(i);
            return take(p, (size_t)count, c->scratch.stageOut[p.buffer].get(), c->scratch.stagePos[p.buffer].get());
        });
    at(Staged::piecesDone);
    const bool drained = hipStreamSynchronize(up) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess;
    if (!drained && st == PFAC_STATUS_SUCCESS) st = PFAC_STATUS_INTERNAL_ERROR;
    at(Staged::drained);
    return st;
}

/*
 * PFAC_matchFromHost on the GPU.  Four of the five bytes per position that the reference moves over the host link
 * (PFAC.cpp:916-960) are results, and nearly all of them are zero.  So the pieces are scanned with the compacted-
 * output kernel and only the (position, id) pairs come back; the zeros are written where they are needed -- by a few
 * helper threads of this call straight into the caller's result vector, while the pieces are uploaded and scanned
 * (piece_pipeline.h: ZeroFill) -- and the pairs of a piece are scattered on top as soon as they are back.  A piece in which
 * more than one position in eight matches takes the full-vector route above instead (after the zero fill, so the two
 * never write the same words at the same time).
 */
PFAC_status_t matchHostOnGpu(PFAC_context *c, char *h_inputString, size_t owned, size_t readable, int *h_matched_result)
{
    if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    const PieceCut cut(owned, readable, kHostPiece, (size_t)c->fa.maxPatternLen);
    unsigned helpers = 0;                                      /* of the zero fill: sized from the cores this thread may run on, up to 8 */
    if (owned >= (size_t(4) << 20)) {
        const unsigned hw = ZeroFill::cpusAllowed();
        helpers = ZeroFill::fromEnv(hw >= 64 ? 8 : hw >= 16 ? 4 : hw >= 4 ? 2 : 1);
    }
    ZeroFill fill(h_matched_result, cut, helpers);
    const bool trace = std::getenv("PFAC_HOST_TRACE") != nullptr;
    std::chrono::steady_clock::time_point tStart;
    auto since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tStart).count(); };
    double tUp0 = 0, tThreads = 0, tLoop = 0;
    auto at = [&](Staged where) {
        if (where == Staged::ready) tStart = std::chrono::steady_clock::now();
        else if (where == Staged::uploadsBegun) {              /* the link first: the fill is not worth a microsecond of an idle copy engine */
            tUp0 = since();
            fill.start();
            tThreads = since();
        } else if (where == Staged::piecesDone) tLoop = since();
        else {
            const double tDrained = since();
            fill.finish();                                     /* every element of the caller's vector is written, whatever happened */
            if (trace) std::fprintf(stderr, "PFAC_HOST_TRACE %zu B %zu pieces %u helpers: first upload queued %.3f ms, threads started %.3f, piece loop done %.3f, drained %.3f, filled+joined %.3f\n",
                                    owned, cut.numPieces(), fill.started(), tUp0, tThreads, tLoop, tDrained, since());
        }
    };
    std::vector<int> pos, id;                                  /* the pairs of one piece */
    std::vector<Piece> densePieces;
    PFAC_status_t st = stagedPairs(c, h_inputString, cut, /* ordered */ false, at, [&](const Piece &p, size_t count, const int *d_ids, const int *d_pos) {
        if (count > p.mine / 8) { densePieces.push_back(p); return PFAC_STATUS_SUCCESS; }
        pos.resize(count);
        id.resize(count);
        if (count && (hipMemcpy(pos.data(), d_pos, count * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
                      hipMemcpy(id.data(), d_ids, count * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess))
            return PFAC_STATUS_INTERNAL_ERROR;
        fill.waitFilled(p.index);                              /* long done, as a rule: the fill runs ahead of the link */
        for (size_t k = 0; k < count; k++)
            if ((size_t)pos[k] < p.mine) h_matched_result[p.off + (size_t)pos[k]] = id[k];   /* beyond: the next piece's (or nobody's) */
        return PFAC_STATUS_SUCCESS;
    });
    for (size_t k = 0; k < densePieces.size() && st == PFAC_STATUS_SUCCESS; k++) {
        const Piece &p = densePieces[k];
        st = matchHostFullVector(c, h_inputString + p.off, p.mine, readable - p.off, h_matched_result + p.off);
    }
    return st;
}

/*
 * PFAC_matchFromHostReduce on the GPU (ref PFAC.cpp:1010-1128: one allocation of size + 8 * size device bytes, one blocking
 * copy, one scan, two copies back).  Same pipeline as PFAC_matchFromHost: the stream goes through the handle's staging
 * buffers in pieces of kHostReducePiece positions, and the pairs of a piece, in position order, are copied straight behind
 * those of the pieces before it: pieces are in stream order, so the whole list is.  Device memory: two pieces (9 bytes per
 * position) instead of 9 bytes for every position of the stream.
 * The stream may be a slice of a longer one (PFACX_matchFromHostReduceMultiGPU): positions [0, owned) get their pairs, `readable`
 * bytes may be read, posBase is added to every position; the caller's arrays hold `owned` entries.
 */
constexpr size_t kHostReducePiece = size_t(16) << 20;
PFAC_status_t matchHostReduceOnGpu(PFAC_context *c, char *h_inputString, size_t size, size_t readable, size_t posBase, int *h_matched_result, int *h_pos, int *h_num_matched)
{
    if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    const PieceCut cut(size, readable, kHostReducePiece, (size_t)c->fa.maxPatternLen);
    size_t total = 0;
    const PFAC_status_t st = stagedPairs(c, h_inputString, cut, /* ordered */ true, [](Staged) {}, [&](const Piece &p, size_t count, const int *d_ids, const int *d_pos) {
        if (count == 0) return PFAC_STATUS_SUCCESS;
        /* total <= p.off (a position has at most one pair); the pairs that stay (positions below p.mine) are at most p.mine, so they lie among the
         * first size - total of the list: the caller's arrays (size entries) hold what is copied */
        const size_t room = size - total, copied = count < room ? count : room;
        if (hipMemcpy(h_pos + total, d_pos, copied * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
        size_t keep = copied;                                  /* positions ascend: those in the overlap are a suffix */
        while (keep > 0 && (size_t)h_pos[total + keep - 1] >= p.mine) keep--;
        if (keep && hipMemcpy(h_matched_result + total, d_ids, keep * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
        if (p.off + posBase) for (size_t k = 0; k < keep; k++) h_pos[total + k] += (int)(p.off + posBase);
        total += keep;
        return PFAC_STATUS_SUCCESS;
    });
    if (st == PFAC_STATUS_SUCCESS) *h_num_matched = (int)total;
    return st;
}

/*
 * PFACX_matchBatchFromHost on the GPU: the stream in pieces of kHostPiece positions, as for PFAC_matchFromHost.  Piece [a, b) is
 * uploaded with its read-ahead up to w = min(size, b + maxPatternLen), the segment boundaries inside (a, w) are rebased to a and the
 * window's ends added, the device batch runs on the window and the results of [a, b) come back.  Clipping the last segment at w is
 * exact: no walk from a position before b reaches w.  A segment may straddle pieces or span several.  Piece by piece, in sequence
 * (one staging buffer): the batch call is for many small buffers that are on the device already, and this form keeps its contract.
 */
PFAC_status_t matchBatchHostOnGpu(PFAC_context *c, char *h_input, size_t size, const size_t *h_offsets, size_t numSegments, int *h_matched_result)
{
    if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    const size_t overlap = (size_t)c->fa.maxPatternLen;
    const size_t piece = size < kHostPiece ? size : kHostPiece;
    PFAC_status_t st = ensureHostStage(c, piece + overlap);
    if (st != PFAC_STATUS_SUCCESS) return st;
    char *const d_in = c->scratch.stageIn[0].get();
    int *const d_out = c->scratch.stageOut[0].get();
    std::vector<size_t> local;
    try {
        for (size_t a = 0; a < size && st == PFAC_STATUS_SUCCESS; a += piece) {
            const size_t b = size - a < piece ? size : a + piece;
            const size_t w = size - b < overlap ? size : b + overlap;
            /* the segment that holds a: the last k < numSegments with offsets[k] <= a; its successors' starts inside (a, w) */
            size_t k = (size_t)(std::upper_bound(h_offsets, h_offsets + numSegments, a) - h_offsets) - 1;
            local.clear();
            local.push_back(0);
            for (k++; k < numSegments && h_offsets[k] < w; k++) local.push_back(h_offsets[k] - a);
            local.push_back(w - a);
            st = c->scratch.batchOffsets.reserve(local.size() > 4096 ? local.size() : 4096);
            if (st != PFAC_STATUS_SUCCESS) return st;
            if (hipMemcpy(d_in, h_input + a, w - a, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(c->scratch.batchOffsets.get(), local.data(), local.size() * sizeof(size_t), hipMemcpyHostToDevice) != hipSuccess) {
                st = PFAC_STATUS_INTERNAL_ERROR;
                break;
            }
            st = foldStaged(c, d_in, w - a);                    /* a caseless set: the window in place */
            if (st != PFAC_STATUS_SUCCESS) break;
            st = matchBatchDeviceLocked(c, d_in, w - a, c->scratch.batchOffsets.get(), local.size() - 1, d_out);
            if (st == PFAC_STATUS_SUCCESS &&
                hipMemcpy(h_matched_result + a, d_out, (b - a) * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
                st = PFAC_STATUS_INTERNAL_ERROR;
        }
    } catch (const std::bad_alloc &) { st = PFAC_STATUS_ALLOC_FAILED; }
    if (hipStreamSynchronize(nullptr) != hipSuccess && st == PFAC_STATUS_SUCCESS) st = PFAC_STATUS_INTERNAL_ERROR;
    return st;
}

} // namespace pfac_internal
