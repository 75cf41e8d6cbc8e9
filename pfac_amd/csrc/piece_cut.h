/*
 * piece_cut.h -- the pigeonhole cut that PFACX_approxOpen and PFACX_editOpen share (approx_api.cpp, edit_api.cpp): a pattern with budget k is cut
 * into k + 1 disjoint parts, of which any occurrence within k mismatches -- or k edits -- leaves one untouched; the PIECE of a part is its head.
 * planPatterns checks the caller's CSR arrays, copies them and lays out the pieces and the piece set as the reader's text; buildPieceTables makes
 * the per-class entry tables and the blob of an object from the plan; getPieces is the getter of both families.  Loading the piece set and
 * checking that the handle holds it is verify_calls.h's adoptOverStrings.
 */
#ifndef PFAC_PIECE_CUT_H
#define PFAC_PIECE_CUT_H

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pfac_host.h"
#include "verify_calls.h"

namespace pfac_internal {

constexpr size_t kMaxCutPatternLen = 65535, kDefaultMaxPiece = 32, kDefaultMinPiece = 4, kMaxCutBudget = 7;
constexpr size_t kMaxCutPatternBytes = (size_t)1 << 32;

/* the caller's patterns, copied, with the pieces of each and the piece set as the reader's text */
struct PiecePlan {
    std::vector<unsigned char> bytes;                 /* all patterns back to back */
    std::vector<size_t> off;                          /* [S + 1] into bytes */
    std::vector<int> budget;                          /* by pattern id */
    size_t maxPiece = 0;
    std::vector<unsigned int> pieceOff;               /* [S + 2] by pattern id */
    std::vector<int> pieceId, pieceStart, pieceLen;   /* per piece */
    StringSet pieces;                                 /* by handle id - 1: the distinct pieces, and the piece set as the reader's text (verify_calls.h) */
};

/* part j of a pattern of len bytes with budget k starts here; part k ends at len */
inline size_t partStart(size_t j, size_t len, size_t k) { return j * len / (k + 1); }

/* The plan of S patterns in CSR form.  INVALID_PARAMETER with *badPattern = the id of the pattern: an offset that does not ascend (an empty
 * pattern), a pattern longer than 65 535 bytes, a budget outside [0, 7], a pattern shorter than (k + 1) minPieceLen, a piece that holds '\n' */
inline PFAC_status_t planPatterns(const unsigned char *h_bytes, const size_t *h_patOff, const int *h_budget, size_t numPatterns, size_t minPieceLen,
                                  size_t maxPieceLen, PiecePlan *plan, int *badPattern)
{
    const size_t S = numPatterns, cut = maxPieceLen ? maxPieceLen : kDefaultMaxPiece, least = minPieceLen ? minPieceLen : kDefaultMinPiece;
    size_t blobWords = 0, numPieces = 0;
    for (size_t i = 1; i <= S; i++) {                                       /* nothing is allocated before every pattern has passed */
        *badPattern = (int)i;
        if (h_patOff[i] <= h_patOff[i - 1] || h_patOff[i] - h_patOff[i - 1] > kMaxCutPatternLen) return PFAC_STATUS_INVALID_PARAMETER;
        const size_t len = h_patOff[i] - h_patOff[i - 1];
        if (h_budget[i - 1] < 0 || h_budget[i - 1] > (int)kMaxCutBudget) return PFAC_STATUS_INVALID_PARAMETER;
        const size_t k = (size_t)h_budget[i - 1];
        if (least > kMaxCutPatternLen || len < (k + 1) * least) return PFAC_STATUS_INVALID_PARAMETER;
        const unsigned char *pat = h_bytes + h_patOff[i - 1];
        for (size_t j = 0; j <= k; j++) {
            const size_t from = partStart(j, len, k), plen = std::min(partStart(j + 1, len, k) - from, cut);
            if (std::memchr(pat + from, '\n', plen) != nullptr) return PFAC_STATUS_INVALID_PARAMETER;   /* the pattern reader splits lines there */
        }
        blobWords += (len + 3) / 4;
        numPieces += k + 1;
    }
    *badPattern = 0;
    if (h_patOff[S] - h_patOff[0] > kMaxCutPatternBytes || blobWords > kMaxInt || numPieces > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    plan->maxPiece = cut;
    plan->off.assign(S + 1, 0);
    plan->budget.assign(S + 1, 0);
    plan->pieceOff.assign(S + 2, 0u);
    plan->bytes.assign(h_bytes + h_patOff[0], h_bytes + h_patOff[S]);
    plan->pieceId.reserve(numPieces);
    plan->pieceStart.reserve(numPieces);
    plan->pieceLen.reserve(numPieces);
    for (size_t i = 1; i <= S; i++) {
        const size_t len = h_patOff[i] - h_patOff[i - 1], k = (size_t)h_budget[i - 1];
        plan->off[i] = plan->off[i - 1] + len;
        plan->budget[i] = (int)k;
        const unsigned char *pat = plan->bytes.data() + plan->off[i - 1];
        for (size_t j = 0; j <= k; j++) {
            const size_t from = partStart(j, len, k), plen = std::min(partStart(j + 1, len, k) - from, cut);
            plan->pieceId.push_back(plan->pieces.idOf(std::string(reinterpret_cast<const char *>(pat) + from, plen)));
            plan->pieceStart.push_back((int)from);
            plan->pieceLen.push_back((int)plen);
        }
        plan->pieceOff[i + 1] = (unsigned int)plan->pieceId.size();
    }
    return PFAC_STATUS_SUCCESS;
}

/* the tables of `obj` from the plan: the classes by handle id, each by pattern id descending, then piece index descending, and the blob.  Obj
 * has numIds, numPatterns, maxPiece, entryOff, entries (of Entry {id, blobOff, start | L << 16, k | j << 8}), blob and the four piece arrays */
template <class Entry, class Obj>
inline void buildPieceTables(PiecePlan &plan, Obj *obj)
{
    const size_t S = plan.off.size() - 1, F = plan.pieces.size(), E = plan.pieceId.size();
    obj->numIds = F;
    obj->numPatterns = S;
    obj->maxPiece = plan.maxPiece;
    obj->entryOff.assign(F + 2, 0u);
    for (size_t e = 0; e < E; e++) obj->entryOff[(size_t)plan.pieceId[e] + 1]++;
    for (size_t q = 1; q <= F + 1; q++) obj->entryOff[q] += obj->entryOff[q - 1];  /* entryOff[q + 1] = the end of class q; entryOff[q]: its start */
    /* (entryOff[0] = entryOff[1] = 0: class 0 is empty) */
    std::vector<unsigned int> next(obj->entryOff.begin(), obj->entryOff.end());
    obj->entries.assign(E, Entry{0, 0, 0u, 0u});
    obj->blob.clear();
    for (size_t i = S; i >= 1; i--) {                                              /* pattern id descending within every class */
        const size_t at = plan.off[i - 1], len = plan.off[i] - at, blobAt = obj->blob.size(), k = (size_t)plan.budget[i];
        obj->blob.resize(blobAt + (len + 3) / 4, 0u);
        std::memcpy(obj->blob.data() + blobAt, plan.bytes.data() + at, len);
        for (size_t j = k + 1; j-- > 0;) {                                         /* ... then piece index descending */
            const size_t e = plan.pieceOff[i] + j;
            obj->entries[next[(size_t)plan.pieceId[e]]++] =
                Entry{(int)i, (int)blobAt, (unsigned int)plan.pieceStart[e] | (unsigned int)len << 16, (unsigned int)k | (unsigned int)j << 8};
        }
    }
    obj->pieceOff = std::move(plan.pieceOff);
    obj->pieceId = std::move(plan.pieceId);
    obj->pieceStart = std::move(plan.pieceStart);
    obj->pieceLen = std::move(plan.pieceLen);
}

/* the getter of both families, behind the caller's handle and generation checks */
template <class Obj>
inline PFAC_status_t getPieces(const Obj &obj, size_t *h_pieceOff, int *h_pieceId, int *h_pieceStart, int *h_pieceLen, size_t n)
{
    const size_t pieces = obj.pieceId.size();
    if ((h_pieceId || h_pieceStart || h_pieceLen) && n < pieces) return PFAC_STATUS_INVALID_PARAMETER;
    if (h_pieceOff)
        for (size_t i = 0; i < obj.pieceOff.size(); i++) h_pieceOff[i] = obj.pieceOff[i];
    const size_t bytes = pieces * sizeof(int);
    if (h_pieceId) std::memcpy(h_pieceId, obj.pieceId.data(), bytes);
    if (h_pieceStart) std::memcpy(h_pieceStart, obj.pieceStart.data(), bytes);
    if (h_pieceLen) std::memcpy(h_pieceLen, obj.pieceLen.data(), bytes);
    return PFAC_STATUS_SUCCESS;
}

} // namespace pfac_internal

#endif
