/*
 * scan_edit.hip -- patterns matched within k edits, insertions and deletions included (include/pfac_ext.h: PFACX_edit*): pattern i of
 * L bytes with budget k occurs at end e where D(e) = min over s of ed(pattern, in[s, e)) <= k (Sellers' recurrence); the handle's patterns are
 * the PIECES of the pigeonhole cut of scan_approx.hip -- an alignment with at most k edits over k + 1 disjoint parts leaves one part untouched --,
 * and an exact piece fixes only a DIAGONAL of the alignment, not its start: the verification is a banded dynamic program per candidate.
 *
 * The passes are one more instantiation of the expansion frame (scan_passes.h: expandCount / pfac_array_scan / expandWrite / pfac_host_done
 * through expandPasses), over an ordered list of LONGEST pairs as in scan_approx.hip: a thread per pair walks the prefix chain
 * (forEachChainMember) and, per member, the (pattern, piece) entries of its class in table order; this unit's own is the verification (verify):
 *   THE CANDIDATE of entry {id, blobOff, o | L << 16, k | j << 8} at pair position p has the diagonal d0 = p - o and covers the ends e with
 *   |e - L - d0| <= k inside [0, n].  d0 < -k (no start inside the input) and L + d0 - k > n (no end inside it) are dropped before any load.
 *   THE BAND.  Rows r = 0 .. L; row r holds the columns c = r + d0 - W + t, t = 0 .. 2 W, W = 2 K + 1, where K is the budget class of the launch
 *   (k <= 1, k <= 3, k <= 7: 7, 15 or 31 cells, all in registers, every loop over them unrolled).  K >= k, and a wider band is as exact as the
 *   one of 2 k + 1: an alignment with at most k edits that ends at a covered end, or next to one, stays within k diagonals of its end, hence
 *   within 2 k + 1 of d0, so for every covered end and for the neighbours the three-point rule looks at the band value equals D(e), start
 *   included, wherever D(e) <= k, and is above k wherever D(e) > k.
 *   A CELL is (cost, start) in one register: cost << 5 | (31 - (start - (d0 - W))), minimised by cost, then by the LARGER start, with a plain
 *   unsigned min; the cost saturates at k + 1 (min with (k + 1) << 5 | 31).  Row 0 is cost 0 with start c for 0 <= c <= n and saturated
 *   elsewhere; a cell with c < 0 has only such predecessors and stays saturated; a cell with c > n holds a value nothing reads: no cell with
 *   c <= n depends on it, and the ends are tested against n.  C[r][0] = r comes out of the vertical step from C[0][0].
 *   THE INPUT of a row is a window of the 4 K + 3 bytes in[r + d0 - W - 1 + t] in K + 1 dwords; a row shifts it by one byte (v_alignbyte) and
 *   loads ONE new byte, in[r + d0 + W - 1], where that index lies inside [0, n) -- a byte load, so no load leaves the caller's buffer at any
 *   pointer alignment; the band is never reloaded.  The pattern byte of a row comes from the dword blob, one load every 4 rows.
 *   EARLY EXIT.  Costs never fall along a path, so a row whose cells are all above k ends the candidate; it is tested every 4 rows (r & 3 == 0).
 *   THE ENDS.  Behind row L the cells t = W - k .. W + k are the covered ends, ascending; one holds where its cost <= k and e <= n, with
 *   bestEnds also D(e - 1) > D(e) and (e == n or D(e + 1) >= D(e)), both neighbours read from the same row.  Behind an end that holds runs
 *   the ownership test (coveredEarlier): it is dropped where a piece j' < j of the pattern is exact at some p' in [e - L + o_j' - k,
 *   e - L + o_j' + k] with the piece inside [0, n), or piece j itself at a p' in [e - L + o_j - k, p - 1]: every occurrence once, by the
 *   covering candidate with the smallest j and of those the smallest p.  It reads the input, not the pair list.
 * The write pass hands (pattern id, start) to the frame's emit and stores end and distance itself in front of it, under the emit's own slot and
 * capacity (scan_verify.h: emitWithAux, which also holds the class loop and the head of PFACX_editRun).
 * Table defence as in the siblings: an id outside [1, F] is a pair that counts nothing, a position outside [0, n) too, a class's range is
 * clamped to the table, an entry whose dwords leave the blob, or with k > K, j > k or L <= k, is skipped.
 * A thread per pair: a candidate that holds costs L x (4 K + 3) dependent cell updates in one lane, in the count pass and twice in the write
 * pass (DESIGN.md 5y says what the longest lane costs).
 * SCRATCH: 8 (blocks + 1) bytes rounded up to 256 (DeviceScratch::editSet), blocks = one per 256 pairs, eight per compute unit at most.
 * Plain C++ and vector stores only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_edit.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"
#include "scan_verify.h"

namespace {

constexpr unsigned int kEditBlock = 256;
constexpr uint32_t kCostOne = 32u, kStartMask = 31u;      /* a cell: cost << 5 | inverted relative start */
constexpr unsigned int kExitEvery = 4;                    /* rows between two tests of the early exit (a power of two) */

struct EditArgs {
    ExpandFrame f;                      /* the pairs, the chain table, the block cut, the caller's arrays (scan_passes.h); f.all is not read */
    InputView v;                        /* the caller's bytes (scan_verify.h) */
    const unsigned int *entryOff;       /* [numIds + 2] by piece id: the first entry of its class */
    const pfac::EditEntry *entries;     /* {pattern id, blobOff, o | L << 16, k | j << 8} */
    unsigned int numEntries;
    const uint32_t *blob;               /* per pattern: (L + 3) / 4 dwords of its bytes */
    unsigned int blobWords;
    unsigned int maxPiece;              /* a piece is the first min(part length, maxPiece) bytes of its part */
    unsigned int bestEnds;              /* the three-point rule */
    int *end;                           /* the ends, capacity entries, or null */
    int *dist;                          /* the distances, capacity entries, or null */
};

/* is a candidate with a smaller piece index, or the same piece at a smaller position than p, one that covers end e of the pattern {len, budget
 * k, bytes at blob[off ...]}?  Piece jj at o_jj covers e from the positions p' in [e - len + o_jj - k, e - len + o_jj + k] at which it is exact
 * and lies inside [0, n) */
__device__ __forceinline__ bool coveredEarlier(const EditArgs &a, unsigned int e, unsigned int len, unsigned int k, unsigned int j, unsigned int p,
                                               unsigned int off)
{
    const unsigned char *pat = reinterpret_cast<const unsigned char *>(a.blob + off);
    unsigned int from = 0;
    for (unsigned int jj = 0; jj <= j; jj++) {
        const unsigned int to = (jj + 1u) * len / (k + 1u);
        unsigned int plen = to - from;
        if (plen > a.maxPiece) plen = a.maxPiece;
        long long lo = (long long)e - (long long)len + (long long)from - (long long)k;
        long long hi = jj < j ? lo + 2ll * (long long)k : (long long)p - 1ll;
        if (lo < 0) lo = 0;
        if (hi > (long long)a.v.n - (long long)plen) hi = (long long)a.v.n - (long long)plen;
        for (long long q = lo; q <= hi; q++) {
            unsigned int t = 0;
            while (t < plen && a.v.in[q + t] == pat[from + t]) t++;
            if (t == plen) return true;
        }
        from = to;
    }
    return false;
}

/* The candidate (piece j at offset o of the pattern {len, k, bytes at blob[off ...]} at input position p): emit(id, start, end, distance) for
 * the ends it covers and owns, ascending; returns their number.  k <= K, len > k, the pattern's dwords lie inside the blob (the caller checks) */
template <int K, class Emit>
__device__ __forceinline__ unsigned int verify(const EditArgs &a, int id, unsigned int o, unsigned int len, unsigned int k, unsigned int j, unsigned int off,
                                               unsigned int p, Emit emit)
{
    constexpr int W = 2 * K + 1, NB = 4 * K + 3, ND = K + 1;
    if ((long long)p - (long long)o < -(long long)k) return 0u;                                   /* every start lies in front of the input */
    if ((long long)len + (long long)p - (long long)o - (long long)k > (long long)a.v.n) return 0u;    /* every covered end behind it */
    /* ub = d0 + W >= 0: column c of cell t in row r is ub + r + t - 2 W, the window's byte t of row r is in[ub + r + t - 2 W - 1] */
    const unsigned int ub = p + (unsigned int)W - o;
    const uint32_t inf = ((k + 1u) << 5) | kStartMask;
    uint32_t cell[NB], win[ND];
#pragma unroll
    for (int i = 0; i < ND; i++) win[i] = 0u;
#pragma unroll
    for (int t = 0; t < NB; t++) {
        const unsigned int x = ub + (unsigned int)t;                                             /* c + 2 W */
        const bool inside = x >= 2u * W && x - 2u * W <= a.v.n;
        cell[t] = inside ? kStartMask - (uint32_t)t : inf;
        uint32_t b = 0u;                                                                         /* the window of row 0: in[c - 1] */
        if (x >= 2u * W + 1u && x - (2u * W + 1u) < a.v.n) b = a.v.in[x - (2u * W + 1u)];
        win[t >> 2] |= b << (8 * (t & 3));
    }
    uint32_t pw = 0u;
    for (unsigned int r = 1; r <= len; r++) {
        pw = ((r - 1u) & 3u) == 0u ? a.blob[off + ((r - 1u) >> 2)] : pw >> 8;
        const uint32_t pb = (pw & 0xFFu) * 0x01010101u;
        const unsigned int at = ub + r - 1u;                                                     /* the one new byte: in[r + d0 + W - 1] */
        const uint32_t nb = at < a.v.n ? (uint32_t)a.v.in[at] : 0u;
        uint32_t x[ND];
#pragma unroll
        for (int i = 0; i + 1 < ND; i++) win[i] = __builtin_amdgcn_alignbyte(win[i + 1], win[i], 1u);
        win[ND - 1] = (win[ND - 1] >> 8) | nb << 16;
#pragma unroll
        for (int i = 0; i < ND; i++) x[i] = win[i] ^ pb;
        uint32_t left = inf;
#pragma unroll
        for (int t = 0; t < NB; t++) {
            uint32_t v = cell[t] + ((x[t >> 2] >> (8 * (t & 3))) & 0xFFu ? kCostOne : 0u);         /* the diagonal step */
            if (t + 1 < NB) v = min(v, cell[t + 1] + kCostOne);                                  /* the vertical one: a pattern byte left out */
            v = min(min(v, left + kCostOne), inf);                                               /* the horizontal one: an input byte put in */
            cell[t] = v;
            left = v;
        }
        if ((r & (kExitEvery - 1u)) == 0u) {
            uint32_t least = cell[0];
#pragma unroll
            for (int t = 1; t < NB; t++) least = min(least, cell[t]);
            if ((least >> 5) > k) return 0u;
        }
    }
    unsigned int found = 0;
#pragma unroll
    for (int t = W - K; t <= W + K; t++) {
        const unsigned int away = (unsigned int)(t < W ? W - t : t - W);
        const uint32_t v = cell[t], d = v >> 5;
        const unsigned int x = ub + len + (unsigned int)t;                                       /* e + 2 W */
        if (away > k || d > k || x - 2u * W > a.v.n) continue;                                     /* (d <= k: the cell's column is >= 0) */
        const unsigned int e = x - 2u * W;
        if (a.bestEnds && ((cell[t - 1] >> 5) <= d || (e != a.v.n && (cell[t + 1] >> 5) < d))) continue;
        if (coveredEarlier(a, e, len, k, j, p, off)) continue;
        emit(id, (int)(ub + (kStartMask - (v & kStartMask)) - 2u * W), (int)e, (int)d);
        found++;
    }
    return found;
}

/* The ends that hold along pair i's chain, longest piece first, table order within a piece, ends ascending within an entry: emit(pattern id,
 * start, end, distance) for each of them; returns their number */
template <int K, class Emit>
__device__ __forceinline__ unsigned int walkPair(const EditArgs &a, size_t i, Emit emit)
{
    const int id = a.f.pairIds[i], p = a.f.pairPos[i];
    if (p < 0 || (unsigned int)p >= a.v.n) return 0u;
    unsigned int found = 0;
    forEachChainMember(a.f.table, a.f.numIds, id, [&](int q) {
        forEachClassEntry(a.entryOff, a.numEntries, q, [&](unsigned int v) {
            const pfac::EditEntry e = a.entries[v];
            const unsigned int o = e.startLen & 0xFFFFu, len = e.startLen >> 16, k = e.budgetPiece & 0xFFu, j = (e.budgetPiece >> 8) & 0xFFu;
            if (k > (unsigned int)K || j > k || len <= k || o >= len) return;
            const unsigned int off = (unsigned int)e.blobOff;
            if (e.blobOff < 0 || !inBlob(a.blobWords, off, (len + 3u) >> 2)) return;                 /* (a table of the library's own: never) */
            found += verify<K>(a, e.id, o, len, k, j, off, (unsigned int)p, emit);
        });
        return true;
    });
    return found;
}

template <int K>
__global__ __launch_bounds__(kEditBlock) void pfac_edit_count(EditArgs a)
{
    expandCount<kEditBlock>(a.f, [&](size_t i) -> unsigned long long { return walkPair<K>(a, i, [](int, int, int, int) {}); });
}

template <int K>
__global__ __launch_bounds__(kEditBlock) void pfac_edit_write(EditArgs a)
{
    expandWrite<kEditBlock>(
        a.f, [&](size_t i) -> unsigned long long { return walkPair<K>(a, i, [](int, int, int, int) {}); },
        [&](size_t i, auto emit) {
            (void)walkPair<K>(a, i, [&](int id, int s, int e, int d) { emitWithAux(emit, id, s, a.end, e, a.dist, d); });
        });
}

} // namespace

extern "C" {

PFAC_status_t PFACX_editRun(PFAC_handle_t handle, const PFACX_editRun_t *run, size_t *h_total)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!run || !verifyRunOk(run->v, h_total) || !run->v.d_blob || !run->d_entryOff || !run->d_entries || run->numEntries > (size_t)0x7fffffff ||
        run->maxPieceLen == 0 || run->maxBudget > 7u)
        return PFAC_STATUS_INVALID_PARAMETER;
    *h_total = 0;
    if (run->v.count == 0) return PFAC_STATUS_SUCCESS;
    PFAC_context *c = handle;
    EditArgs a{};
    a.v = verifyInput(run->v);
    a.entryOff = run->d_entryOff;
    a.entries = static_cast<const pfac::EditEntry *>(run->d_entries);
    a.numEntries = (unsigned int)run->numEntries;
    a.blob = run->v.d_blob;
    a.blobWords = (unsigned int)run->v.blobWords;
    a.maxPiece = (unsigned int)(run->maxPieceLen < (size_t)0xFFFF ? run->maxPieceLen : (size_t)0xFFFF);    /* no part is longer than a pattern */
    a.bestEnds = run->bestEnds ? 1u : 0u;
    a.end = run->v.capacity ? run->d_end : nullptr;
    a.dist = run->v.capacity ? run->d_dist : nullptr;
    a.f = verifyFrame(run->v);
    const bool wantWrite = a.f.capacity != 0;
    /* the budget class of the launch: the band of the largest budget of the table */
    if (run->maxBudget <= 1u)
        return expandPasses(c, c->scratch.editSet, pfac::kHostEdit, a, pfac_edit_count<1>, pfac_edit_write<1>, kEditBlock, wantWrite, h_total);
    if (run->maxBudget <= 3u)
        return expandPasses(c, c->scratch.editSet, pfac::kHostEdit, a, pfac_edit_count<3>, pfac_edit_write<3>, kEditBlock, wantWrite, h_total);
    return expandPasses(c, c->scratch.editSet, pfac::kHostEdit, a, pfac_edit_count<7>, pfac_edit_write<7>, kEditBlock, wantWrite, h_total);
}

} /* extern "C" */
