/*
 * scan_clsig.hip -- signatures of byte classes with bounded repeats (include/pfac_ext.h: PFACX_clsig*): a signature is a sequence of
 * PARTS after fusion, each either a LITERAL part -- a fixed string of bytes -- or a CLASS part (C, lo, hi): lo .. hi bytes that all lie in the
 * byte class C; the handle's patterns are the ANCHORS -- one run of bytes inside one literal part of each signature --, and of the signatures whose
 * anchor a scan found, the (signature, start) for which a choice of run lengths exists under which every part holds in the caller's input and the
 * bytes around it pass the signature's boundary classes, each listed once, with the largest (or, by a flag, the smallest) end over all such choices.
 *
 * The frame is that of scan_gapsig.hip: every anchor that starts at p is a prefix of the longest one that starts there, so the candidates at p are
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
 *                        in front of the frame's store, as in scan_gapsig.hip
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
 * THE COMPARE of a literal part is the bounds-safe dword compare of scan_gapsig.hip without the mask (a copy: that unit stays as it is).
 * Every index into the input is checked against [0, n) before the load; an id outside [1, F] is a pair that counts nothing, a walk ends after
 * chainLen steps whatever the table says, signature and part ranges and class indices are clamped to their tables, a part whose dwords do not lie
 * inside the blob holds nowhere: a caller's list cannot make a pass read or write outside the buffers.  A thread per pair: DESIGN.md 5z says what
 * that costs.
 * SCRATCH: 8 (blocks + 1) bytes rounded up to 256 (DeviceScratch::clsigSet), blocks = one per 256 pairs, eight per compute unit at most.
 * Plain C++ and vector stores only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_clsig.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"

namespace {

constexpr unsigned int kClSigBlock = 256;
constexpr unsigned int kClSigMaxParts = 64;       /* pfac_ext.h: a signature has at most this many parts after fusion */
constexpr unsigned int kClSigMaxSlack = 63;       /* pfac_ext.h: PFACX_CLSIG_MAX_SLACK */
constexpr unsigned int kClSigMaxRepeat = 65535;   /* pfac_ext.h: hi <= 65 535, a literal part has at most as many bytes */
constexpr unsigned int kClSigStaged = 64;         /* the classes every block stages in LDS (pfac_amd/api.py: PFACX_CLSIG_STAGED_CLASSES) */

struct ClSigArgs {
    ExpandFrame f;                      /* the pairs, the chain table, the block cut, the caller's arrays (scan_passes.h); f.all is not read */
    const unsigned char *in;            /* the caller's bytes */
    unsigned int n;
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

/* the aligned dword of the input whose first byte is in[o] (o: any sign; in + o is dword-aligned): one load where it lies inside [0, n), else its
 * bytes inside the buffer, zero for the others */
__device__ __forceinline__ uint32_t alignedDword(const ClSigArgs &a, long long o)
{
    if (o >= 0 && o + 4 <= (long long)a.n) return *reinterpret_cast<const uint32_t *>(a.in + o);
    uint32_t w = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const long long i = o + b;
        if (i >= 0 && i < (long long)a.n) w |= (uint32_t)a.in[i] << (8 * b);
    }
    return w;
}

/* in[s + k] == value[k] for every k < len?  s + len <= n and the part's (len + 3) / 4 dwords at blob[off ...] lie inside the blob (the caller has
 * checked both) */
__device__ __forceinline__ bool literalEqual(const ClSigArgs &a, unsigned int s, unsigned int len, unsigned int off)
{
    const unsigned int words = len >> 2, r = (unsigned int)(reinterpret_cast<uintptr_t>(a.in + s) & 3u);
    const uint32_t *val = a.blob + off;
    uint32_t diff = 0;
    if (r == 0) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(a.in + s);       /* whole dwords inside [s, s + len) */
        for (unsigned int k = 0; k < words; k++) {
            diff |= src[k] ^ val[k];
            if ((k & 3u) == 3u && diff != 0) return false;
        }
    } else {
        const long long base = (long long)s - (long long)r;                     /* the aligned dword that holds in[s] */
        uint32_t lo = words ? alignedDword(a, base) : 0u;
        for (unsigned int k = 0; k < words; k++) {
            const uint32_t hi = alignedDword(a, base + 4ll * (k + 1u));
            diff |= __builtin_amdgcn_alignbyte(hi, lo, r) ^ val[k];
            if ((k & 3u) == 3u && diff != 0) return false;
            lo = hi;
        }
    }
    if (diff != 0) return false;
    const unsigned int tail = len & 3u;
    if (tail) {
        const uint32_t v = val[words];
        for (unsigned int b = 0; b < tail; b++)
            if ((((uint32_t)a.in[s + 4u * words + b] ^ (v >> (8u * b))) & 0xFFu) != 0u) return false;
    }
    return true;
}

/* the bits t of m at which literal part q holds at offset base + dir * t: inside [0, n) -- tested before any load -- and every byte equal.  A
 * part that is empty or whose dwords do not lie inside the blob holds nowhere */
__device__ __forceinline__ uint64_t literalWhere(const ClSigArgs &a, const pfac::ClSigPart &q, long long base, int dir, uint64_t m)
{
    const unsigned int len = q.a, need = (len + 3u) >> 2;
    if (len == 0u || len > kClSigMaxRepeat || q.b >= a.blobWords || a.blobWords - q.b < need) return 0ull;
    uint64_t held = 0;
    while (m != 0ull) {                                   /* at most 64 rounds */
        const int t = __builtin_ctzll(m);
        m &= m - 1ull;
        const long long o = base + (long long)dir * t;
        if (o < 0 || o + (long long)len > (long long)a.n) continue;
        if (literalEqual(a, (unsigned int)o, len, q.b)) held |= 1ull << t;
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
__device__ __forceinline__ Reach classForward(const ClSigArgs &a, const uint32_t *staged, const pfac::ClSigPart &q, long long base, const Reach &r)
{
    Reach out{0ull, 0ull, 0ull};
    if (r.all == 0ull || !classUsable(a, q)) return out;
    const unsigned int lo = q.b, hi = q.c;
    long long far = base + (63 - __builtin_clzll(r.all)) + (long long)hi, near = base + __builtin_ctzll(r.all);
    if (far > (long long)a.n) far = (long long)a.n;       /* nothing behind n exists: a run ends there */
    if (near < 0) near = 0;
    unsigned int run = 0;
    for (long long o = far; o >= near; o--) {             /* at most hi + 64 rounds */
        if (o < far) run = inClass(a, staged, q.a, a.in[o]) ? run + 1u : 0u;
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
__device__ __forceinline__ uint64_t classBackward(const ClSigArgs &a, const uint32_t *staged, const pfac::ClSigPart &q, long long base, uint64_t m)
{
    if (m == 0ull || !classUsable(a, q)) return 0ull;
    const unsigned int lo = q.b, hi = q.c;
    long long low = base - (63 - __builtin_clzll(m)) - (long long)hi, high = base - __builtin_ctzll(m);
    if (low < 0) low = 0;                                 /* nothing in front of 0 exists: a run starts there */
    if (high > (long long)a.n) high = (long long)a.n;
    uint64_t out = 0ull;
    unsigned int run = 0;
    for (long long o = low; o <= high; o++) {             /* at most hi + 64 rounds */
        if (o > low) run = inClass(a, staged, q.a, a.in[o - 1]) ? run + 1u : 0u;
        const long long t = base - o;
        if (t > 63 || !(m >> t & 1ull)) continue;
        const unsigned int len = run < hi ? run : hi;
        if (len >= lo) out |= spanFrom((int)t, len - lo);
    }
    return out;
}

/* The (start, end) that the pair at p owns of signature e (the header says how): emit(e.id, start, end) for each, starts ascending; returns
 * their number */
template <class Emit>
__device__ __forceinline__ unsigned int searchSignature(const ClSigArgs &a, const uint32_t *staged, const pfac::ClSigEntry &e, int p, Emit emit)
{
    const unsigned int count = e.partsAnchor & 0xFFFFu, anchor = e.partsAnchor >> 16;
    if (count < 1u || count > kClSigMaxParts || anchor >= count || e.firstPart >= a.numParts || a.numParts - e.firstPart < count) return 0u;
    if (e.anchorOff > (unsigned int)p) return 0u;                                                    /* x < 0: before any load */
    const pfac::ClSigPart *parts = a.parts + e.firstPart;
    const pfac::ClSigPart pa = parts[anchor];
    if (pa.kind != 0u) return 0u;
    const long long x = (long long)p - (long long)e.anchorOff;
    /* 1. backwards: bit t of `back` = the boundary lies t bytes in front of `tight`, its offset with every run up to part a at lo */
    uint64_t back = literalWhere(a, pa, x, 1, 1ull);
    long long tight = x;
    for (unsigned int j = anchor; j > 0u && back != 0ull; j--) {
        const pfac::ClSigPart q = parts[j - 1u];
        if (q.kind == 0u) {
            tight -= (long long)q.a;
            back = literalWhere(a, q, tight, -1, back);
        } else {
            back = classBackward(a, staged, q, tight, back);
            tight -= (long long)q.b;
        }
    }
    if ((unsigned int)e.notBefore < a.numClasses) {                                                  /* the starts behind a byte of notBefore */
        uint64_t m = back;
        while (m != 0ull) {
            const int t = __builtin_ctzll(m);
            m &= m - 1ull;
            const long long s = tight - t;
            if (s > 0 && s <= (long long)a.n && inClass(a, staged, (unsigned int)e.notBefore, a.in[s - 1])) back &= ~(1ull << t);
        }
    }
    unsigned int found = 0;
    while (back != 0ull) {                                                                           /* the starts, ascending: the highest bit first */
        const int tb = 63 - __builtin_clzll(back);
        back &= ~(1ull << tb);
        const long long s = tight - tb;
        if (s < 0) continue;                                                                         /* (the steps drop them: never) */
        /* 2. forwards to boundary a: bit t = it lies t bytes behind `at`, its offset with every run from part 0 at lo */
        Reach r{1ull, 0ull, 0ull};
        long long at = s;
        for (unsigned int j = 0; j < anchor && r.all != 0ull; j++) {
            const pfac::ClSigPart q = parts[j];
            if (q.kind == 0u) {
                r.all = literalWhere(a, q, at, 1, r.all);
                at += (long long)q.a;
            } else {
                r = classForward(a, staged, q, at, r);
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
                r.all = literalWhere(a, q, at, 1, r.all);
                r.lt &= r.all;
                r.eq &= r.all;
                at += (long long)q.a;
            } else {
                r = classForward(a, staged, q, at, r);
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
                if (end >= (long long)a.n || !inClass(a, staged, (unsigned int)e.notAfter, a.in[end])) valid |= 1ull << t;
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
template <class Emit>
__device__ __forceinline__ unsigned int walkPair(const ClSigArgs &a, const uint32_t *staged, size_t k, Emit emit)
{
    const int id = a.f.pairIds[k], p = a.f.pairPos[k];
    if (p < 0 || (unsigned int)p >= a.n) return 0u;
    unsigned int found = 0;
    forEachChainMember(a.f.table, a.f.numIds, id, [&](int q) {
        const unsigned int first = a.sigOff[q];
        unsigned int end = a.sigOff[q + 1];
        if (end > a.numSigs) end = a.numSigs;
        for (unsigned int v = first; v < end; v++) found += searchSignature(a, staged, a.sigs[v], p, emit);
        return true;
    });
    return found;
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
            (void)walkPair(a, staged, k, [&](int id, int s, int end) {
                if (a.end != nullptr && emit.o < emit.f.capacity) a.end[emit.o] = end;                /* the slot the frame's store takes next */
                emit(id, s);
            });
        });
}

} // namespace

extern "C" {

PFAC_status_t PFACX_clsigRun(PFAC_handle_t handle, const PFACX_clsigRun_t *run, size_t *h_total)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!run || !h_total || !run->d_input || run->size == 0 || run->size > (size_t)0x7fffffff || run->numIds > (size_t)0x7ffffffe || !run->d_sigOff ||
        !run->d_sigs || run->numSigs > (size_t)0x7fffffff || !run->d_parts || run->numParts > (size_t)0x7fffffff ||
        run->blobWords > (size_t)0x7fffffff || !run->d_blob || !run->d_classes || run->numClasses == 0 || run->numClasses > (size_t)0xFFFF ||
        (run->flags & ~PFACX_CLSIG_SHORTEST_END) != 0u || run->count > (size_t)0x7fffffff || (run->count && (!run->d_pairIds || !run->d_pairPos)) ||
        (run->capacity && (!run->d_ids || !run->d_pos)))
        return PFAC_STATUS_INVALID_PARAMETER;
    *h_total = 0;
    if (run->count == 0) return PFAC_STATUS_SUCCESS;
    PFAC_context *c = handle;
    ClSigArgs a{};
    a.in = reinterpret_cast<const unsigned char *>(run->d_input);
    a.n = (unsigned int)run->size;
    a.sigOff = run->d_sigOff;
    a.sigs = static_cast<const pfac::ClSigEntry *>(run->d_sigs);
    a.numSigs = (unsigned int)run->numSigs;
    a.parts = static_cast<const pfac::ClSigPart *>(run->d_parts);
    a.numParts = (unsigned int)run->numParts;
    a.blob = run->d_blob;
    a.blobWords = (unsigned int)run->blobWords;
    a.classes = run->d_classes;
    a.numClasses = (unsigned int)run->numClasses;
    a.shortest = run->flags & PFACX_CLSIG_SHORTEST_END;
    a.end = run->capacity ? run->d_end : nullptr;
    a.f = ExpandFrame{run->d_pairIds, run->d_pairPos, run->count, static_cast<const pfac::Int2 *>(run->d_table), (unsigned int)run->numIds,
                      1u, 0, nullptr, run->d_ids, run->d_pos, run->capacity};
    return expandPasses(c, c->scratch.clsigSet, pfac::kHostClSig, a, pfac_clsig_count, pfac_clsig_write, kClSigBlock, a.f.capacity != 0, h_total);
}

} /* extern "C" */
