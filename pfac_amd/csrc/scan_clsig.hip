/*
 * scan_clsig.hip -- signatures of byte classes with bounded repeats (include/pfac_ext.h: PFACX_clsig*): a signature is a sequence of
 * PARTS after fusion, each either a LITERAL part -- a fixed string of bytes -- or a CLASS part (C, lo, hi): lo .. hi bytes that all lie in the
 * byte class C; the handle's patterns are the ANCHORS -- one run of bytes inside one literal part of each signature --, and of the signatures whose
 * anchor a scan found, the (signature, start) for which a choice of run lengths exists under which every part holds in the caller's input and the
 * bytes around it pass the signature's boundary classes, each listed once, with the largest (or, by a flag, the smallest) end over all such choices.
 *
 * The frame is scan_verify.h's, as in scan_gapsig.hip: every anchor that starts at p is a prefix of the longest one that starts there, so the candidates at p are
 * the longest one's prefix chain (scan_all.hip), and behind a member q stands its CLASS OF SIGNATURES: those that chose q as their anchor, highest
 * signature id first, each {id, first part, number of parts | anchor part << 16, offset of the anchor inside that part} {notBefore, notAfter};
 * a part is {0, len, blobOff} or {1, class, lo, hi} (clsig_api.cpp builds the tables).  The passes work on an ordered list of LONGEST pairs -- the
 * handle's pair scratch behind PFACX_allReduce, or a list of the caller's -- and look at the input again:
 *   pfac_clsig_count     a thread per pair: the chain from the longest member down, for each member the signatures of its class in table order,
 *                        for each signature the search below.  The value of a pair is the number of (signature, start) it OWNS; the block's
 *                        total goes to blockBase[block] (scan_passes.h: expandCount)
 *   pfac_array_scan      exclusive scan of the block totals (one block; 64-bit), the length of the list to mapped host memory
 *   pfac_clsig_write     the block's pairs again (expandWrite): each thread runs the same search once more -- one function, so both passes
 *                        decide alike -- and hands (signature id, start) to the frame (ExpandEmit with a position); the end goes to end[slot]
 *                        in front of the frame's store (scan_verify.h: emitWithAux)
 *   pfac_host_done       the call's sequence number to mapped host memory (scan_passes.h: HostHandoff)
 * The walk along the chain, both passes, the capacity-checked store and the launches are the expansion frame of scan_passes.h, unchanged; this
 * unit's own is the search (searchSignature) and its part steps.
 * THE SEARCH.  A BOUNDARY j is the offset at which part j starts (boundary m: the end).  The slack of a signature, the sum of hi - lo over its class
 * parts, is at most 63, so where a boundary can lie relative to its TIGHTEST offset (every run in between at lo) is a set of at most 64 distances:
 * one 64-bit mask; bit t = t bytes behind (forwards) or in front of (backwards) the tightest offset.  A STEP carries a mask across one part:
 *   literal part   the bits at which the part holds (literalWhere: a dword compare per set bit; a bit whose part would leave [0, n) is dropped
 *                  before any load)
 *   class part     (C, lo, hi), forwards: from start bit t the new bits are t .. t + (run_t - lo), run_t the length of the run of bytes of C from
 *                  that start, cut at hi and at n; run_t < lo: none.  ONE walk over the window from its far end towards its near end keeps the
 *                  running run length: at most hi + 64 bytes a part, not a walk per set bit.  Backwards: the mirror image, runs that END in front
 *                  of a boundary, one walk from the low end of the window upwards
 * A step is a union over the set bits of what each bit gives (the span of a class part depends on the bit it starts from), so a step over three
 * masks of which two are subsets of the first is one walk: each start bit adds its span to every mask that holds it (linearity).
 * With the anchor part a at x = p - anchorOff (x < 0: nothing, before any load):
 *   1. part a holds at x; backwards from boundary a at {x} to boundary 0: its bits are the candidate starts; those with in[s - 1] in the
 *      signature's notBefore class are dropped
 *   2. for each start s, ascending: forwards from boundary 0 at {s} to boundary a: the bits A are where part a can start over a head that holds
 *   3. forwards through parts a .. m - 1, ONE walk with three masks: `all` from A, `lt` from the bits of A below x, `eq` from x alone.  Behind the
 *      last part the ends e with in[e] in notAfter are dropped from all three.  eq empty -- no valid embedding at s has part a at x --, or lt not
 *      empty -- one has it at a smaller offset, and the pair there owns (id, s) --: nothing.  Else (id, s) is this pair's, and its end is the highest
 *      (PFACX_CLSIG_SHORTEST_END: the lowest) bit of `all`, which holds every valid end there is
 * Every loop is bounded by the tables' own limits: at most 64 parts, 64 bits, 64 starts, hi + 64 bytes.
 * CLASS LOOKUPS.  A class is 256 bits in eight dwords; membership of byte b is bit b & 31 of dword b >> 5, read from memory by its index, never
 * out of eight registers.  The first kClSigStaged classes of the table are staged in LDS by every block (2 KiB; a supposition, not measured), the
 * others are read from device memory.
 * THE COMPARE of a literal part is the bounds-safe dword compare without a mask (scan_verify.h: bytesEqual, which scan_case.hip uses too).
 * Every index into the input is checked against [0, n) before the load; an id outside [1, F] is a pair that counts nothing, a walk ends after
 * chainLen steps whatever the table says, signature and part ranges and class indices are clamped to their tables, a part whose dwords do not lie
 * inside the blob holds nowhere: a caller's list cannot make a pass read or write outside the buffers.  A thread per pair: DESIGN.md 5z says what
 * that costs.
 * A BATCH (PFACX_clsigBatch*): the same search inside a WINDOW [lo, hi), the segment that holds the pair's position, wherever the
 * text above says 0 and n (alignedDword alone keeps testing against the buffer: a dword that straddles a segment edge is loaded, and only bytes of
 * [s, s + len) enter a compare); pfac_clsig_bounds, pfac_clsig_batch_count and pfac_clsig_batch_write stand further down with their own text.
 * SCRATCH: 8 (blocks + 1) bytes rounded up to 256 (DeviceScratch::clsigSet), blocks = one per 256 pairs, eight per compute unit at most; a batch
 * takes 4 (numSegments + 1) bytes rounded up to 256 behind them.
 * Plain C++ and vector stores only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_clsig.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"
#include "scan_verify.h"

namespace {

constexpr unsigned int kClSigBlock = 256;
constexpr unsigned int kClSigMaxParts = 64;       /* pfac_ext.h: a signature has at most this many parts after fusion */
constexpr unsigned int kClSigMaxSlack = 63;       /* pfac_ext.h: PFACX_CLSIG_MAX_SLACK */
constexpr unsigned int kClSigMaxRepeat = 65535;   /* pfac_ext.h: hi <= 65 535, a literal part has at most as many bytes */
constexpr unsigned int kClSigStaged = 64;         /* the classes every block stages in LDS (pfac_amd/api.py: PFACX_CLSIG_STAGED_CLASSES) */

struct ClSigArgs {
    ExpandFrame f;                      /* the pairs, the chain table, the block cut, the caller's arrays (scan_passes.h); f.all is not read */
    InputView v;                        /* the caller's bytes (scan_verify.h) */
    const unsigned int *sigOff;         /* [numIds + 2] by anchor id: the first signature of its class */
    const pfac::ClSigEntry *sigs;
    unsigned int numSigs;
    const pfac::ClSigPart *parts;
    unsigned int numParts;
    const uint32_t *blob;               /* per literal part: (len + 3) / 4 value dwords */
    unsigned int blobWords;
    const uint32_t *classes;            /* [8 numClasses] */
    unsigned int numClasses;
    unsigned int shortest;              /* PFACX_CLSIG_SHORTEST_END */
    int *end;                           /* the ends, capacity entries, or null */
};

/* The bounds passes: the plain arguments and the segments of a batch */
struct ClSigBatchArgs : ClSigArgs {
    const unsigned int *bounds;         /* [numSegments + 1] ascending, inside [0, n] (pfac_clsig_bounds) */
    unsigned int numSegments;
    unsigned long long *segFirst;       /* [numSegments + 1], or null */
};

/* THE WINDOW [lo, hi) of a search: the bytes that exist for it.  The plain passes search the whole buffer -- lo a constant, hi the n of the
 * arguments, so they compile to what they were --, the batch passes the segment that holds the pair's position */
struct WholeBuffer {
    static constexpr unsigned int lo = 0u;
    unsigned int hi;
};
struct Segment {
    unsigned int lo, hi;
};

/* where a boundary can lie: every offset, those of embeddings with the anchor part below x, those with it at x (lt and eq: subsets of all) */
struct Reach {
    uint64_t all, lt, eq;
};

/* is byte b in class c (c < numClasses: the caller has checked)?  One bit of 256, the dword by its index out of LDS or device memory */
__device__ __forceinline__ bool inClass(const ClSigArgs &a, const uint32_t *staged, unsigned int c, unsigned int b)
{
    const unsigned int w = 8u * c + (b >> 5);
    const uint32_t word = c < kClSigStaged ? staged[w] : a.classes[w];
    return (word >> (b & 31u) & 1u) != 0u;
}

/* the bits t of m at which literal part q holds at offset base + dir * t: inside the window -- tested before any load -- and every byte equal.  A
 * part that is empty or whose dwords do not lie inside the blob holds nowhere */
template <class W>
__device__ __forceinline__ uint64_t literalWhere(const ClSigArgs &a, const W &w, const pfac::ClSigPart &q, long long base, int dir, uint64_t m)
{
    const unsigned int len = q.a, need = (len + 3u) >> 2;
    if (len == 0u || len > kClSigMaxRepeat || !inBlob(a.blobWords, q.b, need)) return 0ull;
    uint64_t held = 0;
    while (m != 0ull) {                                   /* at most 64 rounds */
        const int t = __builtin_ctzll(m);
        m &= m - 1ull;
        const long long o = base + (long long)dir * t;
        if (o < (long long)w.lo || o + (long long)len > (long long)w.hi) continue;
        if (bytesEqual(a.v, a.blob + q.b, (unsigned int)o, len)) held |= 1ull << t;
    }
    return held;
}

/* bits t .. t + extra of a mask (extra >= 0); what passes bit 63 is gone */
__device__ __forceinline__ uint64_t spanFrom(int t, unsigned int extra) { return (extra >= 63u ? ~0ull : (1ull << (extra + 1u)) - 1ull) << t; }

/* may a search take class part q?  (a table of the library's own: always) */
__device__ __forceinline__ bool classUsable(const ClSigArgs &a, const pfac::ClSigPart &q)
{
    return q.a < a.numClasses && q.c >= q.b && q.c <= kClSigMaxRepeat && q.c - q.b <= kClSigMaxSlack;
}

/* class part q = (C, lo, hi) FORWARDS: bit t of r = the part starts at base + t; behind it bit t' = the next part starts at base + lo + t'.  One
 * walk from the far end of the window to its near end, `run` the length of the run of bytes of C that starts at o, counted inside the window */
template <class W>
__device__ __forceinline__ Reach classForward(const ClSigArgs &a, const W &w, const uint32_t *staged, const pfac::ClSigPart &q, long long base, const Reach &r)
{
    Reach out{0ull, 0ull, 0ull};
    if (r.all == 0ull || !classUsable(a, q)) return out;
    const unsigned int lo = q.b, hi = q.c;
    long long far = base + (63 - __builtin_clzll(r.all)) + (long long)hi, near = base + __builtin_ctzll(r.all);
    if (far > (long long)w.hi) far = (long long)w.hi;     /* nothing behind the window exists: a run ends there */
    if (near < (long long)w.lo) near = (long long)w.lo;
    unsigned int run = 0;
    for (long long o = far; o >= near; o--) {             /* at most hi + 64 rounds */
        if (o < far) run = inClass(a, staged, q.a, a.v.in[o]) ? run + 1u : 0u;
        const long long t = o - base;
        if (t > 63 || !(r.all >> t & 1ull)) continue;
        const unsigned int len = run < hi ? run : hi;
        if (len < lo) continue;
        const uint64_t span = spanFrom((int)t, len - lo);
        out.all |= span;
        if (r.lt >> t & 1ull) out.lt |= span;
        if (r.eq >> t & 1ull) out.eq |= span;
    }
    return out;
}

/* the same BACKWARDS: bit t of m = the part ends in front of base - t; bit t' of the result = it starts at base - lo - t'.  One walk upwards,
 * `run` the length of the run of bytes of C that ends in front of o, counted inside the window */
template <class W>
__device__ __forceinline__ uint64_t classBackward(const ClSigArgs &a, const W &w, const uint32_t *staged, const pfac::ClSigPart &q, long long base, uint64_t m)
{
    if (m == 0ull || !classUsable(a, q)) return 0ull;
    const unsigned int lo = q.b, hi = q.c;
    long long low = base - (63 - __builtin_clzll(m)) - (long long)hi, high = base - __builtin_ctzll(m);
    if (low < (long long)w.lo) low = (long long)w.lo;     /* nothing in front of the window exists: a run starts there */
    if (high > (long long)w.hi) high = (long long)w.hi;
    uint64_t out = 0ull;
    unsigned int run = 0;
    for (long long o = low; o <= high; o++) {             /* at most hi + 64 rounds */
        if (o > low) run = inClass(a, staged, q.a, a.v.in[o - 1]) ? run + 1u : 0u;
        const long long t = base - o;
        if (t > 63 || !(m >> t & 1ull)) continue;
        const unsigned int len = run < hi ? run : hi;
        if (len >= lo) out |= spanFrom((int)t, len - lo);
    }
    return out;
}

/* The (start, end) that the pair at p, a position inside the window w, owns of signature e (the header says how): emit(e.id, start, end) for
 * each, starts ascending; returns their number */
template <class W, class Emit>
__device__ __forceinline__ unsigned int searchSignature(const ClSigArgs &a, const W &w, const uint32_t *staged, const pfac::ClSigEntry &e, int p, Emit emit)
{
    const unsigned int count = e.partsAnchor & 0xFFFFu, anchor = e.partsAnchor >> 16;
    if (count < 1u || count > kClSigMaxParts || anchor >= count || e.firstPart >= a.numParts || a.numParts - e.firstPart < count) return 0u;
    if (e.anchorOff > (unsigned int)p - w.lo) return 0u;                                             /* x in front of the window: before any load */
    const pfac::ClSigPart *parts = a.parts + e.firstPart;
    const pfac::ClSigPart pa = parts[anchor];
    if (pa.kind != 0u) return 0u;
    const long long x = (long long)p - (long long)e.anchorOff;
    /* 1. backwards: bit t of `back` = the boundary lies t bytes in front of `tight`, its offset with every run up to part a at lo */
    uint64_t back = literalWhere(a, w, pa, x, 1, 1ull);
    long long tight = x;
    for (unsigned int j = anchor; j > 0u && back != 0ull; j--) {
        const pfac::ClSigPart q = parts[j - 1u];
        if (q.kind == 0u) {
            tight -= (long long)q.a;
            back = literalWhere(a, w, q, tight, -1, back);
        } else {
            back = classBackward(a, w, staged, q, tight, back);
            tight -= (long long)q.b;
        }
    }
    if ((unsigned int)e.notBefore < a.numClasses) {                                                  /* the starts behind a byte of notBefore */
        uint64_t m = back;
        while (m != 0ull) {
            const int t = __builtin_ctzll(m);
            m &= m - 1ull;
            const long long s = tight - t;
            if (s > (long long)w.lo && s <= (long long)w.hi && inClass(a, staged, (unsigned int)e.notBefore, a.v.in[s - 1])) back &= ~(1ull << t);
        }
    }
    unsigned int found = 0;
    while (back != 0ull) {                                                                           /* the starts, ascending: the highest bit first */
        const int tb = 63 - __builtin_clzll(back);
        back &= ~(1ull << tb);
        const long long s = tight - tb;
        if (s < (long long)w.lo) continue;                                                           /* (the steps drop them: never) */
        /* 2. forwards to boundary a: bit t = it lies t bytes behind `at`, its offset with every run from part 0 at lo */
        Reach r{1ull, 0ull, 0ull};
        long long at = s;
        for (unsigned int j = 0; j < anchor && r.all != 0ull; j++) {
            const pfac::ClSigPart q = parts[j];
            if (q.kind == 0u) {
                r.all = literalWhere(a, w, q, at, 1, r.all);
                at += (long long)q.a;
            } else {
                r = classForward(a, w, staged, q, at, r);
                at += (long long)q.b;
            }
        }
        const long long tx = x - at;
        if (tx < 0 || tx > 63) continue;                                                             /* (x is reachable from s: never) */
        r.eq = r.all & (1ull << tx);
        r.lt = r.all & ((1ull << tx) - 1ull);
        /* 3. forwards to the end: all, below x, x alone */
        for (unsigned int j = anchor; j < count && r.eq != 0ull; j++) {
            const pfac::ClSigPart q = parts[j];
            if (q.kind == 0u) {
                r.all = literalWhere(a, w, q, at, 1, r.all);
                r.lt &= r.all;
                r.eq &= r.all;
                at += (long long)q.a;
            } else {
                r = classForward(a, w, staged, q, at, r);
                at += (long long)q.b;
            }
        }
        if (r.eq == 0ull) continue;
        if ((unsigned int)e.notAfter < a.numClasses) {                                               /* the ends in front of a byte of notAfter */
            uint64_t m = r.all, valid = 0ull;
            while (m != 0ull) {
                const int t = __builtin_ctzll(m);
                m &= m - 1ull;
                const long long end = at + t;
                if (end >= (long long)w.hi || !inClass(a, staged, (unsigned int)e.notAfter, a.v.in[end])) valid |= 1ull << t;
            }
            r.all &= valid;
            r.lt &= valid;
            r.eq &= valid;
        }
        if (r.eq == 0ull || r.lt != 0ull) continue;                                                  /* not on a valid embedding at s, or not the first */
        emit(e.id, (int)s, (int)(at + (a.shortest ? __builtin_ctzll(r.all) : 63 - __builtin_clzll(r.all))));
        found++;
    }
    return found;
}

/* What pair k owns along its chain, longest anchor first, table order (signature id descending) within an anchor (scan_passes.h:
 * forEachChainMember), starts ascending within a signature: emit(signature id, start, end) for each; returns their number */
template <class W, class Emit>
__device__ __forceinline__ unsigned int walkChainAt(const ClSigArgs &a, const W &w, const uint32_t *staged, int id, int p, Emit emit)
{
    unsigned int found = 0;
    forEachChainMember(a.f.table, a.f.numIds, id, [&](int q) {
        forEachClassEntry(a.sigOff, a.numSigs, q, [&](unsigned int v) { found += searchSignature(a, w, staged, a.sigs[v], p, emit); });
        return true;
    });
    return found;
}

/* ... of the plain passes: the window is the buffer */
template <class Emit>
__device__ __forceinline__ unsigned int walkPair(const ClSigArgs &a, const uint32_t *staged, size_t k, Emit emit)
{
    const int id = a.f.pairIds[k], p = a.f.pairPos[k];
    if (p < 0 || (unsigned int)p >= a.v.n) return 0u;
    return walkChainAt(a, WholeBuffer{a.v.n}, staged, id, p, emit);
}

/* ------------------------------------------------------------------ the batch passes (PFACX_clsigBatch*)
 * THE PAIR'S SEGMENT comes from its POSITION p: u(p) = the number of bounds <= p; u in [1, numSegments]: segment u - 1 = [bounds[u - 1], bounds[u]),
 * which holds p; else (p in front of the first bound, at or behind the last, negative): no segment, the pair owns nothing.  An ordered list has
 * its u ascending, so a block searches the bounds ONCE for its first and its last pair, the whole wave at a time (waveLowerBound), and a lane then
 * searches only between the two (scan_groups.hip does the same over pair indices).  What a lane finds there is CHECKED against the two bounds
 * around it and, where it fails -- a caller's list that does not ascend --, searched for again over all bounds: the entries of a pair are right
 * whatever the order of the list.
 * WHO WRITES segFirst[k]: the thread of the first pair i with u(p_i) > k writes the list offset in front of its pair -- the entries k in
 * [u(p_(i-1)), u(p_i)), found by walking down from u(p_i) while the bound lies behind the position of the pair in front (pair 0: all of them);
 * the entries k >= u(the last pair's position) get the length of the list from a grid-stride loop of the same launch.  Over an ascending list
 * every entry has exactly one writer; over any other the stores stay inside segFirst and their values are unspecified. */

/* bounds[k] = the largest of the entries [0, k] of the caller's offsets, each clamped to [0, limit]; k < n = numSegments + 1 (a block of 1024
 * threads per 8192 entries that folds what lies in front of them itself: pfac_groups_bounds of scan_groups.hip over 64-bit offsets) */
constexpr unsigned int kBoundsPer = 8;
constexpr unsigned int kBoundsBlock = 1024 * kBoundsPer;          /* pfac_amd/api.py: PFACX_CLSIG_BOUNDS_BLOCK */

__device__ __forceinline__ unsigned int clampOffset(size_t o, unsigned int limit) { return o > (size_t)limit ? limit : (unsigned int)o; }

__global__ __launch_bounds__(1024) void pfac_clsig_bounds(const size_t *offsets, unsigned int n, unsigned int limit, unsigned int *bounds)
{
    __shared__ unsigned int waveOwn[16], waveFront[16];
    const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned int base = blockIdx.x * kBoundsBlock, i0 = base + threadIdx.x * kBoundsPer;
    unsigned int front = 0;                                             /* what lies in front of the block's entries: coalesced, from L2 */
    for (unsigned int q = threadIdx.x; q < base; q += 1024u) front = OpMax()(front, clampOffset(offsets[q], limit));
    unsigned int x[kBoundsPer], own = 0;
#pragma unroll
    for (unsigned int k = 0; k < kBoundsPer; k++) {
        x[k] = i0 + k < n ? clampOffset(offsets[i0 + k], limit) : 0u;   /* (i0 + k < 2^31 + 8192: no wrap) */
        own = OpMax()(own, x[k]);
    }
    const unsigned int incl = waveInclusive(own, OpMax());
    const unsigned int frontAll = waveReduce(front, OpMax());
    const unsigned int excl = waveExclusiveOf(incl);
    if (lane == 63) { waveOwn[wave] = incl; waveFront[wave] = frontAll; }
    __syncthreads();
    unsigned int run = excl;
    for (unsigned int w = 0; w < 16; w++) {
        run = OpMax()(run, waveFront[w]);
        if (w < wave) run = OpMax()(run, waveOwn[w]);
    }
#pragma unroll
    for (unsigned int k = 0; k < kBoundsPer; k++) {
        run = OpMax()(run, x[k]);
        if (i0 + k < n) bounds[i0 + k] = run;
    }
}

/* the first k of [lo, hi) with bounds[k] > p, else hi; a lane by itself (bounds[k] <= n < 2^31: the compare is signed) */
__device__ __forceinline__ unsigned int boundsBehind(const ClSigBatchArgs &a, unsigned int lo, unsigned int hi, int p)
{
    while (lo < hi) {                                       /* at most 32 rounds */
        const unsigned int mid = lo + ((hi - lo) >> 1);
        if ((int)a.bounds[mid] > p) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

/* where u of a block's pairs lies if its list ascends: inside [lo, hi]; found once per block, by every wave alike (all 64 lanes call it) */
struct BlockSegs { unsigned int lo, hi; };
__device__ __forceinline__ BlockSegs blockSegs(const ClSigBatchArgs &a)
{
    const size_t first = (size_t)blockIdx.x * a.f.per;
    const size_t end = a.f.count - first < a.f.per ? a.f.count : first + a.f.per;
    const int pLo = a.f.pairPos[first], pHi = a.f.pairPos[end - 1];
    BlockSegs b;
    b.lo = waveLowerBound(0u, a.numSegments + 1u, [&](unsigned int k) { return (int)a.bounds[k] > pLo; });
    b.hi = waveLowerBound(b.lo, a.numSegments + 1u, [&](unsigned int k) { return (int)a.bounds[k] > pHi; });
    return b;
}

/* u(p) of a pair of the block, and its segment's window (false: it lies in no segment) */
__device__ __forceinline__ bool segmentOfPair(const ClSigBatchArgs &a, const BlockSegs &b, int p, unsigned int &u, Segment &w)
{
    const unsigned int all = a.numSegments + 1u;
    u = boundsBehind(a, b.lo, b.hi, p);
    if ((u > 0u && (int)a.bounds[u - 1u] > p) || (u < all && (int)a.bounds[u] <= p)) u = boundsBehind(a, 0u, all, p);   /* the list does not ascend */
    if (u < 1u || u > a.numSegments) return false;
    w = Segment{a.bounds[u - 1u], a.bounds[u]};
    return true;
}

/* what pair k owns inside its segment */
template <class Emit>
__device__ __forceinline__ unsigned int walkBatchPair(const ClSigBatchArgs &a, const BlockSegs &b, const uint32_t *staged, size_t k, unsigned int &u, Emit emit)
{
    const int id = a.f.pairIds[k], p = a.f.pairPos[k];
    Segment w;
    if (!segmentOfPair(a, b, p, u, w)) return 0u;           /* (inside a segment: 0 <= p < n) */
    return walkChainAt(a, w, staged, id, p, emit);
}

/* the first kClSigStaged classes of the table into the block's LDS, by all of its threads; the block waits for them */
__device__ __forceinline__ void stageClasses(const ClSigArgs &a, uint32_t *staged)
{
    const unsigned int words = 8u * (a.numClasses < kClSigStaged ? a.numClasses : kClSigStaged);
    for (unsigned int w = threadIdx.x; w < words; w += kClSigBlock) staged[w] = a.classes[w];
    __syncthreads();
}

__global__ __launch_bounds__(kClSigBlock) void pfac_clsig_count(ClSigArgs a)
{
    __shared__ uint32_t staged[8u * kClSigStaged];
    stageClasses(a, staged);
    expandCount<kClSigBlock>(a.f, [&](size_t k) -> unsigned long long { return walkPair(a, staged, k, [](int, int, int) {}); });
}

__global__ __launch_bounds__(kClSigBlock) void pfac_clsig_write(ClSigArgs a)
{
    __shared__ uint32_t staged[8u * kClSigStaged];
    stageClasses(a, staged);
    expandWrite<kClSigBlock>(
        a.f, [&](size_t k) -> unsigned long long { return walkPair(a, staged, k, [](int, int, int) {}); },
        [&](size_t k, auto emit) {
            (void)walkPair(a, staged, k, [&](int id, int s, int end) { emitWithAux(emit, id, s, a.end, end); });
        });
}

__global__ __launch_bounds__(kClSigBlock) void pfac_clsig_batch_count(ClSigBatchArgs a)
{
    __shared__ uint32_t staged[8u * kClSigStaged];
    stageClasses(a, staged);
    const BlockSegs b = blockSegs(a);
    expandCount<kClSigBlock>(a.f, [&](size_t k) -> unsigned long long {
        unsigned int u;
        return walkBatchPair(a, b, staged, k, u, [](int, int, int) {});
    });
}

__global__ __launch_bounds__(kClSigBlock) void pfac_clsig_batch_write(ClSigBatchArgs a)
{
    __shared__ uint32_t staged[8u * kClSigStaged];
    stageClasses(a, staged);
    const BlockSegs b = blockSegs(a);
    /* the entries of segFirst that no pair owns: the bounds behind the last pair's position */
    if (a.segFirst != nullptr) {
        const int pLast = a.f.pairPos[a.f.count - 1];
        const unsigned int tail = waveLowerBound(0u, a.numSegments + 1u, [&](unsigned int k) { return (int)a.bounds[k] > pLast; });
        const unsigned long long total = a.f.blockBase[gridDim.x];
        for (size_t k = (size_t)tail + (size_t)blockIdx.x * kClSigBlock + threadIdx.x; k <= a.numSegments; k += (size_t)gridDim.x * kClSigBlock)
            a.segFirst[k] = total;
    }
    unsigned int u = 0u;                                        /* of the pair a thread has just valued: left to its hook */
    expandWrite<kClSigBlock>(
        a.f, [&](size_t k) -> unsigned long long { return walkBatchPair(a, b, staged, k, u, [](int, int, int) {}); },
        [&](size_t k, auto emit) {
            unsigned int again;
            (void)walkBatchPair(a, b, staged, k, again, [&](int id, int s, int end) { emitWithAux(emit, id, s, a.end, end); });
        },
        [&](size_t k, unsigned long long before) {
            if (a.segFirst == nullptr) return;                  /* every segment that starts behind the pair in front and at or in front of this one */
            const int prev = k > 0 ? a.f.pairPos[k - 1] : -1;
            for (unsigned int j = u; j > 0u && (int)a.bounds[j - 1u] > prev; j--) a.segFirst[j - 1u] = before;   /* (u <= numSegments + 1) */
        });
}

} // namespace

extern "C" {

PFAC_status_t PFACX_clsigRun(PFAC_handle_t handle, const PFACX_clsigRun_t *run, size_t *h_total)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!run || !verifyRunOk(run->v, h_total) || !run->v.d_blob || !run->d_sigOff || !run->d_sigs || run->numSigs > (size_t)0x7fffffff || !run->d_parts ||
        run->numParts > (size_t)0x7fffffff || !run->d_classes || run->numClasses == 0 || run->numClasses > (size_t)0xFFFF ||
        (run->flags & ~PFACX_CLSIG_SHORTEST_END) != 0u ||
        (run->d_offsets ? run->numSegments == 0 || run->numSegments >= (size_t)0x7fffffff : run->d_segFirst != nullptr))
        return PFAC_STATUS_INVALID_PARAMETER;
    *h_total = 0;
    if (run->v.count == 0) {                                      /* no pair: nothing to launch */
        if (!run->d_segFirst) return PFAC_STATUS_SUCCESS;
        return hipMemsetAsync(run->d_segFirst, 0, (run->numSegments + 1) * sizeof(size_t), nullptr) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess
                   ? PFAC_STATUS_SUCCESS
                   : PFAC_STATUS_INTERNAL_ERROR;
    }
    PFAC_context *c = handle;
    ClSigArgs a{};
    a.v = verifyInput(run->v);
    a.sigOff = run->d_sigOff;
    a.sigs = static_cast<const pfac::ClSigEntry *>(run->d_sigs);
    a.numSigs = (unsigned int)run->numSigs;
    a.parts = static_cast<const pfac::ClSigPart *>(run->d_parts);
    a.numParts = (unsigned int)run->numParts;
    a.blob = run->v.d_blob;
    a.blobWords = (unsigned int)run->v.blobWords;
    a.classes = run->d_classes;
    a.numClasses = (unsigned int)run->numClasses;
    a.shortest = run->flags & PFACX_CLSIG_SHORTEST_END;
    a.end = run->v.capacity ? run->d_end : nullptr;
    a.f = verifyFrame(run->v);
    if (run->d_offsets) {                                       /* a batch: the bounds in front of the passes, behind the block totals in the same scratch */
        ClSigBatchArgs b{};
        static_cast<ClSigArgs &>(b) = a;
        b.numSegments = (unsigned int)run->numSegments;
        static_assert(sizeof(size_t) == sizeof(unsigned long long), "segFirst is written as 64-bit words");
        b.segFirst = reinterpret_cast<unsigned long long *>(run->d_segFirst);
        unsigned int *bounds = nullptr;
        return expandPasses(
            c, c->scratch.clsigSet, pfac::kHostClSig, b, pfac_clsig_batch_count, pfac_clsig_batch_write, kClSigBlock, b.f.capacity != 0 || b.segFirst != nullptr,
            h_total, [&](ScratchCarver &k) { b.bounds = bounds = k.take<unsigned int>(run->numSegments + 1); }, false,
            [&]() {
                hipLaunchKernelGGL(pfac_clsig_bounds, dim3((b.numSegments + 1u + kBoundsBlock - 1u) / kBoundsBlock), dim3(1024), 0, 0, run->d_offsets,
                                   b.numSegments + 1u, b.v.n, bounds);
                return true;
            });
    }
    return expandPasses(c, c->scratch.clsigSet, pfac::kHostClSig, a, pfac_clsig_count, pfac_clsig_write, kClSigBlock, a.f.capacity != 0, h_total);
}

} /* extern "C" */
