/*
 * approx_api.cpp -- PFACX_approxOpen / PFACX_approxGetPieces / PFACX_approxClose / PFACX_approxMatchFromDevice / ...FromHost /
 * PFACX_approxPairsFromDevice (include/pfac_ext.h): patterns matched within k mismatches.
 *
 * A pattern of L bytes with budget k occurs at s where at most k bytes of in[s, s + L) differ from its own.  PFACX_approxOpen checks the caller's
 * CSR arrays and copies them, cuts pattern i into k_i + 1 disjoint parts (planPatterns: part j is [j L / (k + 1), (j + 1) L / (k + 1)), its PIECE
 * the first min(part length, maxPieceLen) bytes) -- at any occurrence at least one part, and so its piece, is exact --, loads the distinct pieces
 * into the handle through the reader every pattern set goes through -- one line per piece, in order of first appearance, so handle id q is the q-th
 * distinct piece -- and builds per handle id q the entries of its class (buildTables): {pattern id, blobOff, start | L << 16, k | j << 8} by
 * pattern id descending, then piece index descending, in CSR form by q, with a dword-aligned blob of each pattern's bytes.  Every piece that
 * occurs at p is a prefix of the longest one there, so all three match forms work on the LONGEST pairs of the piece set and walk each pair's
 * prefix chain (Automaton::prefixPattern), member by member through its class: a pattern starts at p - start, must lie inside the input, holds
 * where its distance is within its budget, and is kept by its LOWEST exact piece alone -- an entry of piece j is dropped where a piece j' < j is
 * exact at the same start --, so an occurrence that several exact pieces find is listed once.  The device form runs the unchanged
 * compacted-output path with its ordered pairs in handle scratch (PFACX_allReduce) and the passes of scan_approx.hip (PFACX_approxRun) behind
 * it; the pairs form runs those passes over a list of the caller's.  The host form takes the longest pairs from hostLongestPairs into a
 * temporary of its own and walks the chains here (approxOnHost).
 */
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "pfac_host.h"

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
    ~PFACX_approx_s() override { forEachDeviceBuffer(*this, [](auto &b) { b.release(); }); }
    size_t deviceBytes() const override { size_t n = 0; forEachDeviceBuffer(*this, [&n](const auto &b) { n += b.bytes(); }); return n; }
};

using namespace pfac_internal;

namespace {

constexpr size_t kMaxPatternLen = 65535, kDefaultMaxPiece = 32, kDefaultMinPiece = 4;
constexpr size_t kMaxPatternBytes = (size_t)1 << 32;

/* the caller's patterns, copied, with the pieces of each and the piece set as the reader's text */
struct ApproxPlan {
    std::vector<unsigned char> bytes;                 /* all patterns back to back */
    std::vector<size_t> off;                          /* [S + 1] into bytes */
    std::vector<int> budget;                          /* by pattern id */
    size_t maxPiece = 0;
    std::vector<unsigned int> pieceOff;               /* [S + 2] by pattern id */
    std::vector<int> pieceId, pieceStart, pieceLen;   /* per piece */
    std::vector<std::string> pieces;                  /* by handle id - 1: the distinct pieces in order of first appearance */
    std::string text;                                 /* one line per distinct piece */
};

/* part j of a pattern of len bytes with budget k starts here; part k ends at len */
inline size_t partStart(size_t j, size_t len, size_t k) { return j * len / (k + 1); }

/* The plan of S patterns in CSR form.  INVALID_PARAMETER with *badPattern = the id of the pattern: an offset that does not ascend (an empty
 * pattern), a pattern longer than 65 535 bytes, a budget outside [0, 7], a pattern shorter than (k + 1) minPieceLen, a piece that holds '\n' */
PFAC_status_t planPatterns(const unsigned char *h_bytes, const size_t *h_patOff, const int *h_budget, size_t numPatterns, size_t minPieceLen,
                           size_t maxPieceLen, ApproxPlan *plan, int *badPattern)
{
    const size_t S = numPatterns, cut = maxPieceLen ? maxPieceLen : kDefaultMaxPiece, least = minPieceLen ? minPieceLen : kDefaultMinPiece;
    size_t blobWords = 0, numPieces = 0;
    for (size_t i = 1; i <= S; i++) {                                       /* nothing is allocated before every pattern has passed */
        *badPattern = (int)i;
        if (h_patOff[i] <= h_patOff[i - 1] || h_patOff[i] - h_patOff[i - 1] > kMaxPatternLen) return PFAC_STATUS_INVALID_PARAMETER;
        const size_t len = h_patOff[i] - h_patOff[i - 1];
        if (h_budget[i - 1] < 0 || h_budget[i - 1] > PFACX_APPROX_MAX_MISMATCHES) return PFAC_STATUS_INVALID_PARAMETER;
        const size_t k = (size_t)h_budget[i - 1];
        if (least > kMaxPatternLen || len < (k + 1) * least) return PFAC_STATUS_INVALID_PARAMETER;
        const unsigned char *pat = h_bytes + h_patOff[i - 1];
        for (size_t j = 0; j <= k; j++) {
            const size_t from = partStart(j, len, k), plen = std::min(partStart(j + 1, len, k) - from, cut);
            if (std::memchr(pat + from, '\n', plen) != nullptr) return PFAC_STATUS_INVALID_PARAMETER;   /* the pattern reader splits lines there */
        }
        blobWords += (len + 3) / 4;
        numPieces += k + 1;
    }
    *badPattern = 0;
    if (h_patOff[S] - h_patOff[0] > kMaxPatternBytes || blobWords > kMaxInt || numPieces > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    plan->maxPiece = cut;
    plan->off.assign(S + 1, 0);
    plan->budget.assign(S + 1, 0);
    plan->pieceOff.assign(S + 2, 0u);
    plan->bytes.assign(h_bytes + h_patOff[0], h_bytes + h_patOff[S]);
    plan->pieceId.reserve(numPieces);
    plan->pieceStart.reserve(numPieces);
    plan->pieceLen.reserve(numPieces);
    std::map<std::string, int> seen;
    for (size_t i = 1; i <= S; i++) {
        const size_t len = h_patOff[i] - h_patOff[i - 1], k = (size_t)h_budget[i - 1];
        plan->off[i] = plan->off[i - 1] + len;
        plan->budget[i] = (int)k;
        const unsigned char *pat = plan->bytes.data() + plan->off[i - 1];
        for (size_t j = 0; j <= k; j++) {
            const size_t from = partStart(j, len, k), plen = std::min(partStart(j + 1, len, k) - from, cut);
            const std::string piece(reinterpret_cast<const char *>(pat) + from, plen);
            const auto placed = seen.emplace(piece, (int)plan->pieces.size() + 1);
            if (placed.second) {
                plan->pieces.push_back(piece);
                plan->text += piece;
                plan->text += '\n';
            }
            plan->pieceId.push_back(placed.first->second);
            plan->pieceStart.push_back((int)from);
            plan->pieceLen.push_back((int)plen);
        }
        plan->pieceOff[i + 1] = (unsigned int)plan->pieceId.size();
    }
    return PFAC_STATUS_SUCCESS;
}

/* the tables of `ap` from the plan: the classes by handle id, each by pattern id descending, then piece index descending, and the blob */
void buildTables(ApproxPlan &plan, PFACX_approx_s *ap)
{
    const size_t S = plan.off.size() - 1, F = plan.pieces.size(), E = plan.pieceId.size();
    ap->numIds = F;
    ap->numPatterns = S;
    ap->maxPiece = plan.maxPiece;
    ap->entryOff.assign(F + 2, 0u);
    for (size_t e = 0; e < E; e++) ap->entryOff[(size_t)plan.pieceId[e] + 1]++;
    for (size_t q = 1; q <= F + 1; q++) ap->entryOff[q] += ap->entryOff[q - 1];  /* entryOff[q + 1] = the end of class q; entryOff[q]: its start */
    /* (entryOff[0] = entryOff[1] = 0: class 0 is empty) */
    std::vector<unsigned int> next(ap->entryOff.begin(), ap->entryOff.end());
    ap->entries.assign(E, pfac::ApproxEntry{0, 0, 0u, 0u});
    ap->blob.clear();
    for (size_t i = S; i >= 1; i--) {                                              /* pattern id descending within every class */
        const size_t at = plan.off[i - 1], len = plan.off[i] - at, blobAt = ap->blob.size(), k = (size_t)plan.budget[i];
        ap->blob.resize(blobAt + (len + 3) / 4, 0u);
        std::memcpy(ap->blob.data() + blobAt, plan.bytes.data() + at, len);
        for (size_t j = k + 1; j-- > 0;) {                                         /* ... then piece index descending */
            const size_t e = plan.pieceOff[i] + j;
            ap->entries[next[(size_t)plan.pieceId[e]]++] =
                pfac::ApproxEntry{(int)i, (int)blobAt, (unsigned int)plan.pieceStart[e] | (unsigned int)len << 16, (unsigned int)k | (unsigned int)j << 8};
        }
    }
    ap->pieceOff = std::move(plan.pieceOff);
    ap->pieceId = std::move(plan.pieceId);
    ap->pieceStart = std::move(plan.pieceStart);
    ap->pieceLen = std::move(plan.pieceLen);
}

/* what the three match calls check first (the generation and the pattern set: under the lock) */
PFAC_status_t checkApproxArgs(PFACX_approx_t ap, const void *input, size_t size, const size_t *h_num_matched)
{
    if (!ap || !ap->handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!input || !h_num_matched || size > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    return PFAC_STATUS_SUCCESS;
}

/* the first device call of an approximate object: its tables (the caller holds the handle's lock) */
PFAC_status_t ensureDeviceTables(PFACX_approx_s *ap)
{
    if (ap->d_entryOff) return PFAC_STATUS_SUCCESS;
    const PFAC_status_t st = uploadAll(ap->d_entryOff, ap->entryOff, ap->d_entries, ap->entries, ap->d_blob, ap->blob);
    if (st != PFAC_STATUS_SUCCESS) PFACX_approx_s::forEachDeviceBuffer(*ap, [](auto &b) { b.release(); });
    return st;
}

/* the passes over `count` ordered longest pairs, behind the argument checks; the caller holds c->lock */
PFAC_status_t approxRunLocked(PFACX_approx_s *ap, const char *d_input, size_t size, const int *d_pairIds, const int *d_pairPos, size_t count,
                              int *d_ids, int *d_pos, int *d_mis, size_t capacity, size_t *h_num_matched)
{
    PFAC_context *c = ap->handle;
    PFAC_status_t st = c->fa.maxChain > 1 ? ensureAllTable(c) : PFAC_STATUS_SUCCESS;
    if (st == PFAC_STATUS_SUCCESS) st = ensureDeviceTables(ap);
    if (st != PFAC_STATUS_SUCCESS) return st;
    PFACX_approxRun_t run{};
    run.d_input = d_input;
    run.size = size;
    run.d_pairIds = d_pairIds;
    run.d_pairPos = d_pairPos;
    run.count = count;
    run.d_table = c->fa.maxChain > 1 ? c->scratch.allTable.get() : nullptr;
    run.numIds = ap->numIds;
    run.d_entryOff = ap->d_entryOff.get();
    run.d_entries = ap->d_entries.get();
    run.numEntries = ap->entries.size();
    run.d_blob = ap->d_blob.get();
    run.blobWords = ap->blob.size();
    run.maxPieceLen = ap->maxPiece;
    run.d_ids = d_ids;
    run.d_pos = d_pos;
    run.d_mis = d_mis;
    run.capacity = capacity;
    size_t total = 0;
    st = c->approx_run_ptr(c, &run, &total);
    if (st != PFAC_STATUS_SUCCESS) return st;
    *h_num_matched = total;
    return truncatedIf(total, capacity);
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
    ApproxPlan plan;
    try {
        const PFAC_status_t st = planPatterns(h_bytes, h_patOff, h_budget, numPatterns, minPieceLen, maxPieceLen, &plan, &bad);
        if (badPattern) *badPattern = bad;
        if (st != PFAC_STATUS_SUCCESS) return st;                             /* nothing of the handle has changed */
    } catch (const std::bad_alloc &) { return PFAC_STATUS_ALLOC_FAILED; }
    /* the pieces through the reader of every pattern set: the set is replaced, the handle case-sensitive */
    PFAC_status_t st = PFACX_readPatternFromMemory(handle, plan.text.data(), plan.text.size());
    if (st != PFAC_STATUS_SUCCESS) return st;
    return adoptNew(handle, approx, [&](PFACX_approx_s &obj) -> PFAC_status_t {
        /* another thread may have replaced the set since: the tables hold only over the pieces, id by id */
        const pfac::Automaton &fa = handle->fa;
        if (handle->caseInsensitive || (size_t)fa.numPatterns != plan.pieces.size()) return PFAC_STATUS_INVALID_PARAMETER;
        for (size_t q = 1; q <= plan.pieces.size(); q++) {
            const std::string &piece = plan.pieces[q - 1];
            if ((size_t)fa.patternLen[q] != piece.size() || fa.chainLen[q] < 1 ||
                std::memcmp(fa.file.data() + fa.patternOff[q], piece.data(), piece.size()) != 0)
                return PFAC_STATUS_INVALID_PARAMETER;
        }
        buildTables(plan, &obj);
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
    const size_t pieces = approx->pieceId.size();
    if ((h_pieceId || h_pieceStart || h_pieceLen) && n < pieces) return PFAC_STATUS_INVALID_PARAMETER;
    if (h_pieceOff)
        for (size_t i = 0; i < approx->pieceOff.size(); i++) h_pieceOff[i] = approx->pieceOff[i];
    const size_t bytes = pieces * sizeof(int);
    if (h_pieceId) std::memcpy(h_pieceId, approx->pieceId.data(), bytes);
    if (h_pieceStart) std::memcpy(h_pieceStart, approx->pieceStart.data(), bytes);
    if (h_pieceLen) std::memcpy(h_pieceLen, approx->pieceLen.data(), bytes);
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_approxMatchFromDevice(PFACX_approx_t approx, char *d_input, size_t size, int *d_ids, int *d_pos, int *d_mis, size_t capacity,
                                          size_t *h_num_matched)
{
    PFAC_status_t st = checkApproxArgs(approx, d_input, size, h_num_matched);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (!d_ids || !d_pos) return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = approx->handle;
    if (size && capacity < size) return PFAC_STATUS_INVALID_PARAMETER;
    if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(c->lock);
    st = checkSetGeneration(c, approx->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0) { *h_num_matched = 0; return PFAC_STATUS_SUCCESS; }
    DeviceScan scan;
    st = beginDeviceScan(c, d_input, size, &scan);
    if (st != PFAC_STATUS_SUCCESS) return st;
    /* the caller's arrays take the scan's unordered list, the ordered pairs go to the handle's pair scratch: the passes never filter in place */
    int count = 0;
    st = c->all_reduce_ptr(c, reinterpret_cast<int *>(scan.d_scan), (int)size, d_ids, d_pos, &count, scan.hashed);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (count < 0 || (size_t)count > size) return PFAC_STATUS_INTERNAL_ERROR;
    const int *pairIds = c->scratch.allPairs.get();
    const int *pairPos = pairIds + c->scratch.allPairs.count() / 2;        /* one allocation: the ids, then as many positions */
    if (count == 0) { *h_num_matched = 0; return PFAC_STATUS_SUCCESS; }
    return approxRunLocked(approx, d_input, size, pairIds, pairPos, (size_t)count, d_ids, d_pos, d_mis, capacity, h_num_matched);
}

PFAC_status_t PFACX_approxMatchFromHost(PFACX_approx_t approx, char *h_input, size_t size, int *h_ids, int *h_pos, int *h_mis, size_t capacity,
                                        size_t *h_num_matched)
{
    PFAC_status_t st = checkApproxArgs(approx, h_input, size, h_num_matched);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (capacity && (!h_ids || !h_pos)) return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = approx->handle;
    {
        std::lock_guard<std::mutex> guard(c->lock);
        st = checkSetGeneration(c, approx->generation);
        if (st != PFAC_STATUS_SUCCESS) return st;
    }
    if (size == 0) { *h_num_matched = 0; return PFAC_STATUS_SUCCESS; }
    if (hostLacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    const HostPairs pairs(size, size);
    if (!pairs) return PFAC_STATUS_ALLOC_FAILED;
    const PinnedPairs scan(c, h_input, size, pairs.ids, pairs.pos);
    if (scan.status != PFAC_STATUS_SUCCESS) return scan.status;
    if (scan.generation != approx->generation) return PFAC_STATUS_INVALID_PARAMETER;    /* another thread has replaced the set meanwhile: as after the call */
    const size_t total = approxOnHost(c->fa, *approx, reinterpret_cast<const unsigned char *>(h_input), size, pairs.ids, pairs.pos,
                                      (size_t)(scan.count > 0 ? scan.count : 0), h_ids, h_pos, h_mis, capacity);
    *h_num_matched = total;
    return truncatedIf(total, capacity);
}

PFAC_status_t PFACX_approxPairsFromDevice(PFACX_approx_t approx, const char *d_input, size_t size, const int *d_pairIds, const int *d_pairPos,
                                          size_t numPairs, int *d_ids, int *d_pos, int *d_mis, size_t capacity, size_t *h_num_matched)
{
    PFAC_status_t st = checkApproxArgs(approx, d_input, size, h_num_matched);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (numPairs > kMaxInt || capacity > SIZE_MAX / sizeof(int) || (numPairs && (!d_pairIds || !d_pairPos)) || (capacity && (!d_ids || !d_pos)))
        return PFAC_STATUS_INVALID_PARAMETER;
    if (capacity && numPairs) {
        const size_t in = numPairs * sizeof(int), out = capacity * sizeof(int);
        for (const int *array : {d_ids, d_pos, d_mis})
            if (array && (overlap(array, out, d_pairIds, in) || overlap(array, out, d_pairPos, in))) return PFAC_STATUS_INVALID_PARAMETER;
    }
    PFAC_context *c = approx->handle;
    if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(c->lock);
    st = checkSetGeneration(c, approx->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (size == 0 || numPairs == 0) { *h_num_matched = 0; return PFAC_STATUS_SUCCESS; }
    return approxRunLocked(approx, d_input, size, d_pairIds, d_pairPos, numPairs, d_ids, d_pos, d_mis, capacity, h_num_matched);
}

} /* extern "C" */
