/*
 * approx_api.cpp -- PFACX_approxOpen / PFACX_approxGetPieces / PFACX_approxClose / PFACX_approxMatchFromDevice / ...FromHost /
 * PFACX_approxPairsFromDevice (include/pfac_ext.h): patterns matched within k mismatches.
 *
 * A pattern of L bytes with budget k occurs at s where at most k bytes of in[s, s + L) differ from its own.  PFACX_approxOpen checks the caller's
 * CSR arrays and copies them, cuts pattern i into k_i + 1 disjoint parts (piece_cut.h, shared with edit_api.cpp: planPatterns: part j is [j L / (k + 1), (j + 1) L / (k + 1)), its PIECE
 * the first min(part length, maxPieceLen) bytes) -- at any occurrence at least one part, and so its piece, is exact --, loads the distinct pieces
 * into the handle through the reader every pattern set goes through -- one line per piece, in order of first appearance, so handle id q is the q-th
 * distinct piece -- and builds per handle id q the entries of its class (buildPieceTables): {pattern id, blobOff, start | L << 16, k | j << 8} by
 * pattern id descending, then piece index descending, in CSR form by q, with a dword-aligned blob of each pattern's bytes.  Every piece that
 * occurs at p is a prefix of the longest one there, so all three match forms work on the LONGEST pairs of the piece set and walk each pair's
 * prefix chain (Automaton::prefixPattern), member by member through its class: a pattern starts at p - start, must lie inside the input, holds
 * where its distance is within its budget, and is kept by its LOWEST exact piece alone -- an entry of piece j is dropped where a piece j' < j is
 * exact at the same start --, so an occurrence that several exact pieces find is listed once.  The device form runs the unchanged
 * compacted-output path with its ordered pairs in handle scratch (PFACX_allReduce) and the passes of scan_approx.hip (PFACX_approxRun) behind
 * it; the pairs form runs those passes over a list of the caller's.  The host form takes the longest pairs from hostLongestPairs into a
 * temporary of its own and walks the chains here (approxOnHost).
 * The open tail (the pieces loaded and the handle checked to hold them), the order of the checks, the scan, the pair temporaries and the
 * generation re-check of the three forms are the frame of verify_calls.h; this file's own is the run's arguments (approxRunLocked) and the host loop.
 */
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "pfac_host.h"
#include "piece_cut.h"
#include "verify_calls.h"

struct PFACX_approx_s : pfac_internal::HandleObject {
    size_t numIds = 0;                        /* F of the piece set it loaded */
    size_t numPatterns = 0;                   /* S */
    size_t maxPiece = 0;                      /* the cut of a piece, the default resolved */
    /* by pattern id in CSR form (pieceOff[0] = pieceOff[1] = 0: no pattern 0): per piece, in piece order, the handle's pattern id of its
     * string, its start in the pattern and its length */
    std::vector<unsigned int> pieceOff;       /* [S + 2] */
    std::vector<int> pieceId, pieceStart, pieceLen;
    /* by handle id q: the entries of its class at entries[entryOff[q], entryOff[q + 1]), by pattern id descending, then piece index descending */
    std::vector<unsigned int> entryOff;       /* [F + 2] */
    std::vector<pfac::ApproxEntry> entries;
    std::vector<unsigned int> blob;           /* per pattern (L + 3) / 4 dwords of its bytes, the bytes behind L zero */
    /* the same on the device, uploaded by the first device call: state of the object (deviceTableBytes), freed by PFACX_approxClose */
    pfac::DeviceBuffer<unsigned int> d_entryOff, d_blob;
    pfac::DeviceBuffer<pfac::ApproxEntry> d_entries;

    template <class Self, class F> static void forEachDeviceBuffer(Self &self, F f) { f(self.d_entryOff); f(self.d_entries); f(self.d_blob); }
    PFAC_status_t uploadTables() { return pfac_internal::uploadAll(d_entryOff, entryOff, d_entries, entries, d_blob, blob); }
    ~PFACX_approx_s() override { forEachDeviceBuffer(*this, [](auto &b) { b.release(); }); }
    size_t deviceBytes() const override { size_t n = 0; forEachDeviceBuffer(*this, [&n](const auto &b) { n += b.bytes(); }); return n; }
};

using namespace pfac_internal;

namespace {

/* the passes over `count` ordered longest pairs, behind the argument checks; the caller holds c->lock */
PFAC_status_t approxRunLocked(PFACX_approx_s *ap, const VerifyCall &call, int *d_mis, const int *d_pairIds, const int *d_pairPos, size_t count)
{
    PFACX_approxRun_t run{};
    const PFAC_status_t st = fillRunFrame(ap, call, d_pairIds, d_pairPos, count, &run.v);
    if (st != PFAC_STATUS_SUCCESS) return st;
    run.d_entryOff = ap->d_entryOff.get();
    run.d_entries = ap->d_entries.get();
    run.numEntries = ap->entries.size();
    run.maxPieceLen = ap->maxPiece;
    run.d_mis = d_mis;
    return finishRun(ap->handle, ap->handle->approx_run_ptr, run, call);
}

/* The host loop: the entries that hold along the chains of `count` ordered longest pairs into ids / pos / mis (slots >= capacity are not
 * written; mis may be null); returns the full length of the list */
size_t approxOnHost(const pfac::Automaton &fa, const PFACX_approx_s &ap, const unsigned char *in, size_t n, const int *pairIds, const int *pairPos,
                    size_t count, int *ids, int *pos, int *mis, size_t capacity)
{
    size_t total = 0;
    const unsigned char *blob = reinterpret_cast<const unsigned char *>(ap.blob.data());
    for (size_t i = 0; i < count; i++) {
        const int p = pairPos[i];
        if (p < 0 || (size_t)p >= n) continue;
        forEachChainMember(fa, pairIds[i], [&](int q) {                       /* (the caller's pin: fa.numPatterns == ap.numIds) */
            for (size_t v = ap.entryOff[(size_t)q]; v < ap.entryOff[(size_t)q + 1]; v++) {
                const pfac::ApproxEntry e = ap.entries[v];
                const size_t start = e.startLen & 0xFFFFu, len = e.startLen >> 16, k = e.budgetPiece & 0xFFu, j = (e.budgetPiece >> 8) & 0xFFu;
                if (start > (size_t)p) continue;                                /* it would start in front of the input */
                const size_t s = (size_t)p - start;
                if (len > n - s) continue;                                      /* ... or end behind it */
                const unsigned char *pat = blob + 4 * (size_t)e.blobOff;
                size_t d = 0;
                for (size_t t = 0; t < len && d <= k; t++) d += in[s + t] != pat[t];
                if (d > k) continue;
                bool earlier = false;                                           /* a lower exact piece reports this occurrence */
                for (size_t jj = 0; jj < j && !earlier; jj++) {
                    const size_t from = partStart(jj, len, k), plen = std::min(partStart(jj + 1, len, k) - from, ap.maxPiece);
                    earlier = std::memcmp(in + s + from, pat + from, plen) == 0;
                }
                if (earlier) continue;
                if (total < capacity) {
                    ids[total] = e.id;
                    pos[total] = (int)s;
                    if (mis) mis[total] = (int)d;
                }
                total++;
            }
            return true;
        });
    }
    return total;
}

} // namespace

extern "C" {

PFAC_status_t PFACX_approxOpen(PFAC_handle_t handle, const unsigned char *h_bytes, const size_t *h_patOff, const int *h_budget, size_t numPatterns,
                               size_t minPieceLen, size_t maxPieceLen, PFACX_approx_t *approx, int *badPattern)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!approx) return PFAC_STATUS_INVALID_PARAMETER;
    *approx = nullptr;
    int bad = 0;
    if (badPattern) *badPattern = 0;
    if (!h_bytes || !h_patOff || !h_budget || numPatterns == 0 || numPatterns >= kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    PiecePlan plan;   /* piece_cut.h: the cut PFACX_editOpen shares */
    try {
        const PFAC_status_t st = planPatterns(h_bytes, h_patOff, h_budget, numPatterns, minPieceLen, maxPieceLen, &plan, &bad);
        if (badPattern) *badPattern = bad;
        if (st != PFAC_STATUS_SUCCESS) return st;                             /* nothing of the handle has changed */
    } catch (const std::bad_alloc &) { return PFAC_STATUS_ALLOC_FAILED; }
    return adoptOverStrings(handle, plan.pieces, approx, [&](PFACX_approx_s &obj) -> PFAC_status_t {   /* (verify_calls.h: the tables hold only over the pieces) */
        buildPieceTables<pfac::ApproxEntry>(plan, &obj);
        return PFAC_STATUS_SUCCESS;
    });
}

PFAC_status_t PFACX_approxClose(PFACX_approx_t approx) { return closeObject(approx); }

PFAC_status_t PFACX_approxGetPieces(PFACX_approx_t approx, size_t *h_pieceOff, int *h_pieceId, int *h_pieceStart, int *h_pieceLen, size_t n)
{
    if (!approx || !approx->handle) return PFAC_STATUS_INVALID_HANDLE;
    PFAC_context *c = approx->handle;
    std::lock_guard<std::mutex> guard(c->lock);
    const PFAC_status_t st = checkSetGeneration(c, approx->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    return getPieces(*approx, h_pieceOff, h_pieceId, h_pieceStart, h_pieceLen, n);
}

PFAC_status_t PFACX_approxMatchFromDevice(PFACX_approx_t approx, char *d_input, size_t size, int *d_ids, int *d_pos, int *d_mis, size_t capacity,
                                          size_t *h_num_matched)
{
    const VerifyCall call{d_input, size, d_ids, d_pos, capacity, h_num_matched};
    return verifyFromDevice(approx, call, [&](const int *ids, const int *pos, size_t count) { return approxRunLocked(approx, call, d_mis, ids, pos, count); });
}

PFAC_status_t PFACX_approxMatchFromHost(PFACX_approx_t approx, char *h_input, size_t size, int *h_ids, int *h_pos, int *h_mis, size_t capacity,
                                        size_t *h_num_matched)
{
    const VerifyCall call{h_input, size, h_ids, h_pos, capacity, h_num_matched};
    return verifyFromHost(approx, call, [&](const int *ids, const int *pos, size_t count) {
        return approxOnHost(approx->handle->fa, *approx, reinterpret_cast<const unsigned char *>(h_input), size, ids, pos, count, h_ids, h_pos, h_mis,
                            capacity);
    });
}

PFAC_status_t PFACX_approxPairsFromDevice(PFACX_approx_t approx, const char *d_input, size_t size, const int *d_pairIds, const int *d_pairPos,
                                          size_t numPairs, int *d_ids, int *d_pos, int *d_mis, size_t capacity, size_t *h_num_matched)
{
    const VerifyCall call{d_input, size, d_ids, d_pos, capacity, h_num_matched};
    return verifyPairsFromDevice(approx, call, d_pairIds, d_pairPos, numPairs, {d_ids, d_pos, d_mis}, [&](const int *ids, const int *pos, size_t count) {
        return approxRunLocked(approx, call, d_mis, ids, pos, count);
    });
}

} /* extern "C" */
