/*
 * edit_api.cpp -- PFACX_editOpen / PFACX_editGetPieces / PFACX_editClose / PFACX_editMatchFromDevice / ...FromHost / PFACX_editPairsFromDevice
 * (include/pfac_ext.h): patterns matched within k edits, insertions and deletions included.
 *
 * Pattern i occurs at end e where D(e) = min over s of ed(pat_i, in[s, e)) <= k_i (Sellers' recurrence).  PFACX_editOpen runs the cut of
 * PFACX_approxOpen (piece_cut.h: planPatterns, buildPieceTables; the tables are those of approx_api.cpp with EditEntry for ApproxEntry) and loads
 * the distinct pieces into the handle: an alignment with at most k edits over k + 1 disjoint parts leaves one part untouched, so its piece is
 * exact somewhere in the input.  All three match forms work on the LONGEST pairs of the piece set and walk each pair's prefix chain, member by
 * member through its class.  An entry (pattern, piece j at offset o) at pair position p is a CANDIDATE with the diagonal d0 = p - o; it covers
 * the ends e with |e - L - d0| <= k inside [0, n], is verified by a dynamic program over the band of 2 k + 1 diagonals on either side of d0
 * (DESIGN.md 5y says why that is exact for the covered ends and their neighbours), and lists the covered ends that hold and that no candidate
 * with a smaller piece index, or the same piece at a smaller position, covers: every occurrence once.  The device form runs the unchanged
 * compacted-output path with its ordered pairs in handle scratch (PFACX_allReduce) and the passes of scan_edit.hip (PFACX_editRun) behind it;
 * the pairs form runs those passes over a list of the caller's.  The host form takes the longest pairs from hostLongestPairs into a temporary
 * of its own and verifies with byte loops here (editOnHost): the same band, the same ownership rule, no code shared with the kernel.
 * The open tail (the pieces loaded and the handle checked to hold them), the order of the checks, the scan, the pair temporaries and the
 * generation re-check of the three forms are the frame of verify_calls.h; this file's own is the run's arguments (editRunLocked) and the host loop.
 */
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "pfac_host.h"
#include "piece_cut.h"
#include "verify_calls.h"

struct PFACX_edit_s : pfac_internal::HandleObject {
    size_t numIds = 0;                        /* F of the piece set it loaded */
    size_t numPatterns = 0;                   /* S */
    size_t maxPiece = 0;                      /* the cut of a piece, the default resolved */
    unsigned int maxBudget = 0;               /* the largest k: the budget class of the device passes */
    bool bestEnds = false;                    /* PFACX_EDIT_BEST_ENDS */
    /* as in PFACX_approx_s: the pieces by pattern id in CSR form, the classes by handle id, the blob */
    std::vector<unsigned int> pieceOff;       /* [S + 2] */
    std::vector<int> pieceId, pieceStart, pieceLen;
    std::vector<unsigned int> entryOff;       /* [F + 2] */
    std::vector<pfac::EditEntry> entries;
    std::vector<unsigned int> blob;           /* per pattern (L + 3) / 4 dwords of its bytes, the bytes behind L zero */
    /* the same on the device, uploaded by the first device call: state of the object (deviceTableBytes), freed by PFACX_editClose */
    pfac::DeviceBuffer<unsigned int> d_entryOff, d_blob;
    pfac::DeviceBuffer<pfac::EditEntry> d_entries;

    template <class Self, class F> static void forEachDeviceBuffer(Self &self, F f) { f(self.d_entryOff); f(self.d_entries); f(self.d_blob); }
    PFAC_status_t uploadTables() { return pfac_internal::uploadAll(d_entryOff, entryOff, d_entries, entries, d_blob, blob); }
    ~PFACX_edit_s() override { forEachDeviceBuffer(*this, [](auto &b) { b.release(); }); }
    size_t deviceBytes() const override { size_t n = 0; forEachDeviceBuffer(*this, [&n](const auto &b) { n += b.bytes(); }); return n; }
};

using namespace pfac_internal;

namespace {

/* the passes over `count` ordered longest pairs, behind the argument checks; the caller holds c->lock */
PFAC_status_t editRunLocked(PFACX_edit_s *ed, const VerifyCall &call, int *d_end, int *d_dist, const int *d_pairIds, const int *d_pairPos, size_t count)
{
    PFACX_editRun_t run{};
    const PFAC_status_t st = fillRunFrame(ed, call, d_pairIds, d_pairPos, count, &run.v);
    if (st != PFAC_STATUS_SUCCESS) return st;
    run.d_entryOff = ed->d_entryOff.get();
    run.d_entries = ed->d_entries.get();
    run.numEntries = ed->entries.size();
    run.maxPieceLen = ed->maxPiece;
    run.maxBudget = ed->maxBudget;
    run.bestEnds = ed->bestEnds ? 1 : 0;
    run.d_end = d_end;
    run.d_dist = d_dist;
    return finishRun(ed->handle, ed->handle->edit_run_ptr, run, call);
}

/* one cell of the band on the host: the cost, saturated at k + 1, and the start of the shortest best match */
struct HostCell { unsigned int cost; long long start; };
inline bool better(const HostCell &a, const HostCell &b) { return a.cost != b.cost ? a.cost < b.cost : a.start > b.start; }

/* is piece [from, from + plen) of pat exact at some p' in [lo, hi] with the piece inside [0, n)? */
bool exactWithin(const unsigned char *in, size_t n, const unsigned char *pat, size_t from, size_t plen, long long lo, long long hi)
{
    lo = std::max(lo, 0ll);
    hi = std::min(hi, (long long)n - (long long)plen);
    for (long long q = lo; q <= hi; q++)
        if (std::memcmp(in + q, pat + from, plen) == 0) return true;
    return false;
}

/* The host loop: the ends that hold along the chains of `count` ordered longest pairs into ids / pos / end / dist (slots >= capacity are not
 * written; end and dist may be null); returns the full length of the list */
size_t editOnHost(const pfac::Automaton &fa, const PFACX_edit_s &ed, const unsigned char *in, size_t n, const int *pairIds, const int *pairPos,
                  size_t count, int *ids, int *pos, int *end, int *dist, size_t capacity)
{
    size_t total = 0;
    const unsigned char *blob = reinterpret_cast<const unsigned char *>(ed.blob.data());
    std::vector<HostCell> row, next;
    for (size_t i = 0; i < count; i++) {
        const int p = pairPos[i];
        if (p < 0 || (size_t)p >= n) continue;
        forEachChainMember(fa, pairIds[i], [&](int q) {                       /* (the caller's pin: fa.numPatterns == ed.numIds) */
            for (size_t v = ed.entryOff[(size_t)q]; v < ed.entryOff[(size_t)q + 1]; v++) {
                const pfac::EditEntry entry = ed.entries[v];
                const long long o = entry.startLen & 0xFFFFu, len = entry.startLen >> 16, k = entry.budgetPiece & 0xFFu, j = (entry.budgetPiece >> 8) & 0xFFu;
                const long long d0 = (long long)p - o, W = 2 * k + 1, cells = 2 * W + 1, N = (long long)n;
                if (d0 < -k || len + d0 - k > N) continue;                      /* no start, or no end, inside the input */
                const unsigned char *pat = blob + 4 * (size_t)entry.blobOff;
                const HostCell inf{(unsigned int)k + 1u, -1};
                /* cell t of row r is the column c = r + d0 - W + t */
                row.assign((size_t)cells, inf);
                for (long long t = 0; t < cells; t++) {
                    const long long c = d0 - W + t;
                    if (c >= 0 && c <= N) row[(size_t)t] = HostCell{0u, c};
                }
                bool alive = true;
                for (long long r = 1; r <= len && alive; r++) {
                    next.assign((size_t)cells, inf);
                    alive = false;
                    for (long long t = 0; t < cells; t++) {
                        const long long c = r + d0 - W + t;
                        if (c < 0 || c > N) continue;
                        HostCell best = inf;
                        const auto take = [&](const HostCell &from, unsigned int step) {
                            const HostCell cand{std::min(from.cost + step, (unsigned int)k + 1u), from.start};
                            if (cand.cost <= (unsigned int)k && better(cand, best)) best = cand;
                        };
                        if (c >= 1) take(row[(size_t)t], in[c - 1] != pat[r - 1] ? 1u : 0u);
                        if (t + 1 < cells) take(row[(size_t)t + 1], 1u);
                        if (t >= 1) take(next[(size_t)t - 1], 1u);
                        next[(size_t)t] = best;
                        alive = alive || best.cost <= (unsigned int)k;
                    }
                    row.swap(next);
                }
                if (!alive) continue;                                           /* a row with every cell above k: costs never fall along a path */
                for (long long t = W - k; t <= W + k; t++) {
                    const long long e = len + d0 - W + t;
                    const HostCell here = row[(size_t)t];
                    if (e < 0 || e > N || here.cost > (unsigned int)k) continue;
                    if (ed.bestEnds && (row[(size_t)t - 1].cost <= here.cost || (e != N && row[(size_t)t + 1].cost < here.cost))) continue;
                    bool earlier = false;                                       /* a candidate with a smaller (j, p) covers this end */
                    for (long long jj = 0; jj <= j && !earlier; jj++) {
                        const size_t from = partStart((size_t)jj, (size_t)len, (size_t)k);
                        const size_t plen = std::min(partStart((size_t)jj + 1, (size_t)len, (size_t)k) - from, ed.maxPiece);
                        const long long lo = e - len + (long long)from - k;
                        earlier = exactWithin(in, n, pat, from, plen, lo, jj < j ? lo + 2 * k : (long long)p - 1);
                    }
                    if (earlier) continue;
                    if (total < capacity) {
                        ids[total] = entry.id;
                        pos[total] = (int)here.start;
                        if (end) end[total] = (int)e;
                        if (dist) dist[total] = (int)here.cost;
                    }
                    total++;
                }
            }
            return true;
        });
    }
    return total;
}

} // namespace

extern "C" {

PFAC_status_t PFACX_editOpen(PFAC_handle_t handle, const unsigned char *h_bytes, const size_t *h_patOff, const int *h_budget, size_t numPatterns,
                             size_t minPieceLen, size_t maxPieceLen, unsigned int flags, PFACX_edit_t *edit, int *badPattern)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!edit) return PFAC_STATUS_INVALID_PARAMETER;
    *edit = nullptr;
    int bad = 0;
    if (badPattern) *badPattern = 0;
    if (!h_bytes || !h_patOff || !h_budget || numPatterns == 0 || numPatterns >= kMaxInt || (flags & ~PFACX_EDIT_BEST_ENDS) != 0u)
        return PFAC_STATUS_INVALID_PARAMETER;
    PiecePlan plan;
    try {
        const PFAC_status_t st = planPatterns(h_bytes, h_patOff, h_budget, numPatterns, minPieceLen, maxPieceLen, &plan, &bad);
        if (badPattern) *badPattern = bad;
        if (st != PFAC_STATUS_SUCCESS) return st;                             /* nothing of the handle has changed */
    } catch (const std::bad_alloc &) { return PFAC_STATUS_ALLOC_FAILED; }
    return adoptOverStrings(handle, plan.pieces, edit, [&](PFACX_edit_s &obj) -> PFAC_status_t {       /* (verify_calls.h: the tables hold only over the pieces) */
        obj.maxBudget = (unsigned int)*std::max_element(plan.budget.begin(), plan.budget.end());
        obj.bestEnds = (flags & PFACX_EDIT_BEST_ENDS) != 0u;
        buildPieceTables<pfac::EditEntry>(plan, &obj);
        return PFAC_STATUS_SUCCESS;
    });
}

PFAC_status_t PFACX_editClose(PFACX_edit_t edit) { return closeObject(edit); }

PFAC_status_t PFACX_editGetPieces(PFACX_edit_t edit, size_t *h_pieceOff, int *h_pieceId, int *h_pieceStart, int *h_pieceLen, size_t n)
{
    if (!edit || !edit->handle) return PFAC_STATUS_INVALID_HANDLE;
    PFAC_context *c = edit->handle;
    std::lock_guard<std::mutex> guard(c->lock);
    const PFAC_status_t st = checkSetGeneration(c, edit->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    return getPieces(*edit, h_pieceOff, h_pieceId, h_pieceStart, h_pieceLen, n);
}

PFAC_status_t PFACX_editMatchFromDevice(PFACX_edit_t edit, char *d_input, size_t size, int *d_ids, int *d_pos, int *d_end, int *d_dist, size_t capacity,
                                        size_t *h_num_matched)
{
    const VerifyCall call{d_input, size, d_ids, d_pos, capacity, h_num_matched};
    return verifyFromDevice(edit, call, [&](const int *ids, const int *pos, size_t count) { return editRunLocked(edit, call, d_end, d_dist, ids, pos, count); });
}

PFAC_status_t PFACX_editMatchFromHost(PFACX_edit_t edit, char *h_input, size_t size, int *h_ids, int *h_pos, int *h_end, int *h_dist, size_t capacity,
                                      size_t *h_num_matched)
{
    const VerifyCall call{h_input, size, h_ids, h_pos, capacity, h_num_matched};
    return verifyFromHost(edit, call, [&](const int *ids, const int *pos, size_t count) {
        return editOnHost(edit->handle->fa, *edit, reinterpret_cast<const unsigned char *>(h_input), size, ids, pos, count, h_ids, h_pos, h_end, h_dist,
                          capacity);
    });
}

PFAC_status_t PFACX_editPairsFromDevice(PFACX_edit_t edit, const char *d_input, size_t size, const int *d_pairIds, const int *d_pairPos,
                                        size_t numPairs, int *d_ids, int *d_pos, int *d_end, int *d_dist, size_t capacity, size_t *h_num_matched)
{
    const VerifyCall call{d_input, size, d_ids, d_pos, capacity, h_num_matched};
    return verifyPairsFromDevice(edit, call, d_pairIds, d_pairPos, numPairs, {d_ids, d_pos, d_end, d_dist}, [&](const int *ids, const int *pos, size_t count) {
        return editRunLocked(edit, call, d_end, d_dist, ids, pos, count);
    });
}

} /* extern "C" */
