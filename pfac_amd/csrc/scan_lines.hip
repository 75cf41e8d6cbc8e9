/*
 * scan_lines.hip -- lines (include/pfac_ext.h: PFACX_matchLines* / PFACX_gatherLines*): the lines of a buffer that contain a
 * pattern, or that contain none, and their text.
 *
 * No pattern contains '\n' (the pattern format ends a pattern there), so no match crosses a line end: the plain compacted scan of the whole
 * buffer is exact per line, and all that is left is to say which line a pair falls into.  Everything below is indexed by q = p + mis, the
 * position p counted from the aligned 16-byte block that holds the first input byte (mis = address & 15): a misaligned caller pointer costs
 * nothing but that offset.  A line is named by the '\n' that ends it; an input whose last byte is none gets a VIRTUAL newline at q = mis + size,
 * so the unterminated last line is a line like every other.  A BLOCK is 2048 positions = 64 bitmap words = one wave, one word per lane.
 *
 *   pfac_lines_bitmap      one streaming pass over the input, a wave per block, 16-byte loads (two per lane; the granules that are not whole
 *                          inside the buffer -- at most two of a launch -- byte by byte with bounds).  16 bytes become 16 bits by a SWAR compare;
 *                          two shuffles hand every lane the 32 bits of its word.  Writes the newline bitmap, a zero word of the line-hit
 *                          bitmap, the number of newlines of the block in front of each word (ushort) and the block's count
 *   pfac_block_scan<sum>   the exclusive prefix of the block counts: the line number at each block's start (scan_passes.h: a block of 1024
 *                          threads per 8192 counts that folds what lies in front of them itself); the total goes to mapped host memory
 *   [the compacted scan, its pairs left unordered in the caller's arrays: scan_module.hip]
 *   pfac_lines_mark        a thread per pair: line = block base + rank of the word + set bits below the position; atomicOr into the hit bitmap
 *   pfac_lines_select<0>   a wave per block: the lines that end in a word are consecutive, so their hit bits are one 64-bit funnel; counts
 *                          the selected ones (hit ^ invert) per block and notes the block's last newline
 *   pfac_block_scan<sum, max>  the same for the selected lines and, in the same launch, the running maximum of the blocks' last newline: the
 *                          first selected line of each block, the last newline in front of each block
 *   pfac_lines_select<1>   the same walk again, writing (start, len, index) in order over the scan's pair list
 *   pfac_host_done         the call's sequence number to mapped host memory (scan_passes.h: HostHandoff)
 * Only the first pass and the scan touch O(size) bytes; the rest reads size / 8 bytes of bitmaps and the pairs.
 * SCRATCH of a select call, B = (mis + size) / 2048 + 1 blocks: 256 B (newline bitmap) + 256 B + 256 once (hit bitmap and the word a funnel may
 * read behind it) + 128 B (ranks) + 2 x (4 (B + 1) + 4 (B + 1) + 4 B) bytes (lines, selected lines and last newline per block, and their scans), each part
 * rounded up to 256 bytes: 0.32 bytes per input byte, whatever the data.
 *
 * The gather: pfac_lines_gather_count / pfac_array_scan (scan_passes.h) / pfac_lines_gather_offsets give every line its 64-bit offset in the text (len + 1
 * per line, (start, len) clamped to the input), pfac_lines_gather_copy cuts the TEXT, not the list, into tiles of 4 KiB: a tile finds its
 * first line by binary search in the offsets, stages the offsets of its lines (at most 4096) in LDS, and every thread assembles 16 output
 * bytes -- one 3 MiB line and a million 20-byte lines are the same work per byte.  Tiles are aligned on the output address, a tile stops at
 * outCapacity.  SCRATCH of a gather: 8 (numSelected + 1) bytes of offsets + 8 bytes per 256 .. 2048 lines of block sums.
 *
 * Context (PFACX_matchLinesContext*): the lines within `before` in front of and `after` behind a line of H, the lines the plain call
 * selects.  It is a dilation of the line-hit bitmap in the LINE-INDEX domain -- bit k is line k; a LINE BLOCK is 2048 lines = 64 words = one wave
 * -- between pfac_lines_mark and the select passes, entered from PFACX_linesSelectContext only:
 *   pfac_lines_members     the hit bitmap becomes H's in place: hit ^ invert, the bits at and beyond the number of lines cleared (under INVERT
 *                          they are all ones: they must be gone before anything is widened).  Per line block: H's last member + 1, the
 *                          complement of its first (nearer = larger, so that the scan below is a maximum too; stored back to front), and
 *                          H's popcount added to one word: the number of matching lines
 *   pfac_block_scan<max, max>  in one launch the nearest member in front of each line block and -- the second column runs back to front --
 *                          the nearest behind it
 *   pfac_lines_widen       a word per lane: the nearest members in front of and behind the word by a wave prefix and a wave suffix maximum on
 *                          top of the block's two values.  A member in front reaches the word's low bits, a member behind its high bits, the
 *                          word's own members are smeared by min(after, 31) and min(before, 31) in five doubling shifts: the work is the same
 *                          for every before and after.  Writes the widened bitmap, and the GROUP STARTS -- selected lines whose predecessor
 *                          is not -- in front of each word of its line block (ushort) and per line block
 *   pfac_block_scan<sum>   the group starts in front of each line block; the total is the number of groups
 *   pfac_lines_select<0 / 1, ContextArgs>  the plain walk over the widened bitmap; the emit pass also writes the tag: the group from the group
 *                          starts in front of the word's first line, counted on along its lines, and the member bit from H's bitmap
 * SCRATCH of the stage, B as above (a buffer of its own: a plain call allocates none of it): 256 B + 256 once (widened bitmap) + 128 B (group
 * ranks) + 4 B + 4 B + 4 (B + 1) + 4 B + 4 B + 4 (B + 1) + 4 bytes (per line block: the two nearest members and their scans, the group starts
 * and their scan; the matching lines), each part rounded up to 256 bytes: 0.20 bytes per input byte.
 * Plain C++ and vector stores only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_lines.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"

namespace {

constexpr unsigned int kLinesThreads = 256;                /* four waves, a block of positions each */
constexpr unsigned int kBlockShift = 11;                   /* 2048 positions per block ... */
constexpr unsigned int kBlockWords = 64;                   /* ... = 64 bitmap words, one per lane */

struct LinesArgs {
    const unsigned char *in;            /* the caller's bytes */
    size_t n;
    unsigned int mis;                   /* address of in & 15: q = p + mis */
    unsigned int blocks;
    uint32_t *nlBits;                   /* [blocks * 64] bit q: a line ends at q */
    uint32_t *hitBits;                  /* [blocks * 64 + 64] bit k: line k holds a match */
    uint16_t *rank;                     /* [blocks * 64] newlines of the block in front of the word */
    unsigned int *lineCount, *lineBase; /* [blocks] newlines per block; [blocks + 1] lines in front of the block, [blocks] = the number of lines */
    unsigned int *selCount, *selBase;   /* the same for the selected lines */
    unsigned int *lastNl, *prevNl;      /* [blocks] q + 1 of the block's last newline (0: none; q itself may pass 2^31); of the last newline in front of the block */
    uint32_t invert;                    /* 0 or 0xFFFFFFFF */
    int *lineStart, *lineLen, *lineIndex;
};

/* the same with context: bitmaps and counts by LINE NUMBER, a line block = 2048 lines = 64 words.  hitBits holds H once pfac_lines_members has run */
struct ContextArgs : LinesArgs {
    uint32_t *selBits;                  /* [blocks * 64 + 64] bit k: line k is selected */
    uint16_t *groupRank;                /* [blocks * 64] group starts of the line block in front of the word */
    unsigned int *memberTop, *memberNext;   /* [blocks] k + 1 of the line block's last member of H (0: none); ~k of its first, block b at blocks - 1 - b */
    unsigned int *prevMember, *nextMember;  /* [blocks + 1], [blocks] their running maxima: the nearest member in front of / behind the line block */
    unsigned int *groupCount, *groupBase;   /* [blocks] group starts per line block; [blocks + 1] in front of it, [blocks] = the number of groups */
    unsigned int *matching;             /* one word, zero when pfac_lines_members starts: |H| */
    unsigned int *hostMatching;         /* the same in mapped host memory, or null */
    uint32_t membersInvert;             /* 0 or 0xFFFFFFFF: H = hit ^ this (invert itself stays 0: the select passes read selBits as it is) */
    unsigned int before, after;
    int *lineTag;
};

/* bit i: byte i of x is '\n' (scan_passes.h: bytesEqual4) */
__device__ __forceinline__ uint32_t newlines4(uint32_t x) { return bytesEqual4(x, 0x0A0A0A0Au); }

/* the 16 bits of granule g (positions q in [16 g, 16 g + 16)) */
__device__ __forceinline__ uint32_t granuleBits(const LinesArgs &a, size_t g)
{
    const long long p0 = (long long)(g * 16) - (long long)a.mis;
    if (p0 >= 0 && (size_t)p0 + 16 <= a.n) {
        const pfacmod::u32x4 v = *reinterpret_cast<const pfacmod::u32x4 *>(a.in + p0);
        return newlines4(v.x) | newlines4(v.y) << 4 | newlines4(v.z) << 8 | newlines4(v.w) << 12;
    }
    uint32_t bits = 0;
    for (int i = 0; i < 16; i++) {
        const long long p = p0 + i;
        if (p >= 0 && (size_t)p < a.n) bits |= (a.in[p] == '\n' ? 1u : 0u) << i;
        else if ((size_t)p == a.n && p > 0) bits |= (a.in[p - 1] != '\n' ? 1u : 0u) << i;      /* the virtual newline of an unterminated last line */
    }
    return bits;
}

__global__ __launch_bounds__(kLinesThreads) void pfac_lines_bitmap(LinesArgs a)
{
    const unsigned int lane = threadIdx.x & 63u;
    const unsigned int waves = gridDim.x * (kLinesThreads / 64);
    for (unsigned int b = blockIdx.x * (kLinesThreads / 64) + (threadIdx.x >> 6); b < a.blocks; b += waves) {
        const size_t g = (size_t)b * 128 + lane;
        const uint32_t lo = granuleBits(a, g), hi = granuleBits(a, g + 64);
        /* word w of the block = granules 2 w and 2 w + 1: the low halves of lanes 2 w, 2 w + 1 (w < 32), else the high halves of lanes 2 w - 64 ... */
        const uint32_t both = lo | hi << 16;
        const int src = (int)((2u * lane) & 63u);
        const uint32_t x0 = (uint32_t)__shfl((int)both, src), x1 = (uint32_t)__shfl((int)both, src + 1);
        const uint32_t word = lane < 32u ? (x0 & 0xFFFFu) | (x1 << 16) : (x0 >> 16) | (x1 & 0xFFFF0000u);
        const uint32_t c = (uint32_t)__popc(word);
        const uint32_t incl = waveInclusiveScan(c);
        const size_t w = (size_t)b * kBlockWords + lane;
        a.nlBits[w] = word;
        a.hitBits[w] = 0;
        a.rank[w] = (uint16_t)(incl - c);
        if (lane == 63u) a.lineCount[b] = incl;
    }
}

/* a thread per pair of the scan's list: the line that holds the position */
__global__ __launch_bounds__(kLinesThreads) void pfac_lines_mark(LinesArgs a, const int *pos, unsigned int count)
{
    for (unsigned int i = blockIdx.x * kLinesThreads + threadIdx.x; i < count; i += gridDim.x * kLinesThreads) {
        const int p = pos[i];
        if (p < 0 || (size_t)p >= a.n) continue;
        const size_t q = (size_t)p + a.mis;
        const size_t w = q >> 5;
        const unsigned int line = a.lineBase[q >> kBlockShift] + a.rank[w] + (unsigned int)__popc(a.nlBits[w] & ((1u << (q & 31u)) - 1u));
        const uint32_t bit = 1u << (line & 31u);
        uint32_t *word = &a.hitBits[line >> 5];                /* line <= p: inside the bitmap whatever the pair says */
        if ((__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) == 0) atomicOr(word, bit);
    }
}

/* the bitmap by line number that the select passes read: the hits, or with context the widened bitmap (invert == 0 there) */
__device__ __forceinline__ const uint32_t *selectBits(const LinesArgs &a) { return a.hitBits; }
__device__ __forceinline__ const uint32_t *selectBits(const ContextArgs &a) { return a.selBits; }

/* WRITE == 0: the selected lines that end in each block, and the block's last newline; WRITE == 1: their (start, len, index) -- and, with
 * context (Args = ContextArgs), their tags */
template <int WRITE, class Args = LinesArgs>
__global__ __launch_bounds__(kLinesThreads) void pfac_lines_select(Args a)
{
    constexpr bool kContext = std::is_same<Args, ContextArgs>::value;
    const uint32_t *const bits = selectBits(a);
    const unsigned int lane = threadIdx.x & 63u;
    const unsigned int waves = gridDim.x * (kLinesThreads / 64);
    for (unsigned int b = blockIdx.x * (kLinesThreads / 64) + (threadIdx.x >> 6); b < a.blocks; b += waves) {
        const size_t w = (size_t)b * kBlockWords + lane;
        uint32_t word = a.nlBits[w];
        const uint32_t c = (uint32_t)__popc(word);
        const unsigned int first = a.lineBase[b] + a.rank[w];           /* the lines that end in this word: [first, first + c) */
        const uint32_t h0 = bits[first >> 5], h1 = bits[(first >> 5) + 1];
        const uint32_t hits = (uint32_t)((((uint64_t)h1 << 32) | h0) >> (first & 31u));
        const uint32_t sel = (hits ^ a.invert) & (c >= 32u ? 0xFFFFFFFFu : (1u << c) - 1u);
        const uint32_t ns = (uint32_t)__popc(sel);
        const uint32_t incl = waveInclusiveScan(ns);
        const unsigned int qWord = (b << kBlockShift) + lane * 32u;
        const unsigned int last = word ? qWord + 32u - (unsigned int)__clz((int)word) : 0u;            /* q + 1 */
        if constexpr (WRITE == 0) {
            const unsigned int top = waveReduce(last, OpMax());
            if (lane == 63u) { a.selCount[b] = incl; a.lastNl[b] = top; }
        } else {
            /* q + 1 of the last newline in front of this word: where its first line starts */
            unsigned int prev = OpMax()(a.prevNl[b], waveExclusiveOf(waveInclusive(last, OpMax())));
            size_t o = (size_t)a.selBase[b] + (incl - ns);
            /* with context: H's bits of these lines, the group starts up to the first of them, whether the line in front of it is selected */
            uint32_t members = 0, behind = 0;
            unsigned int groups = 0;
            if constexpr (kContext) {
                if (a.lineTag != nullptr && c != 0) {
                    const unsigned int wi = first >> 5, r = first & 31u;
                    const uint32_t m0 = a.hitBits[wi], m1 = a.hitBits[wi + 1];
                    members = (uint32_t)((((uint64_t)m1 << 32) | m0) >> r);
                    const uint32_t carry = wi ? bits[wi - 1] >> 31 : 0u;
                    const uint32_t starts = h0 & ~((h0 << 1) | carry);
                    groups = a.groupBase[wi >> 6] + a.groupRank[wi] + (unsigned int)__popc(starts & ((1u << r) - 1u));
                    behind = r ? (h0 >> (r - 1u)) & 1u : carry;
                }
            }
            for (unsigned int j = 0; word; j++) {
                const unsigned int q = qWord + (unsigned int)__ffs((int)word) - 1u;
                word &= word - 1u;
                if ((sel >> j) & 1u) {
                    const unsigned int startQ = prev > a.mis ? prev : a.mis;
                    a.lineStart[o] = (int)(startQ - a.mis);
                    a.lineLen[o] = (int)(q - startQ);
                    if (a.lineIndex != nullptr) a.lineIndex[o] = (int)(first + j);
                    if constexpr (kContext) {
                        if (a.lineTag != nullptr) {
                            groups += behind ^ 1u;                         /* a selected line behind one that is not: the next group */
                            a.lineTag[o] = (int)(((groups - 1u) << 1) | ((members >> j) & 1u));
                        }
                    }
                    o++;
                }
                if constexpr (kContext) behind = (sel >> j) & 1u;
                prev = q + 1u;
            }
        }
    }
}

/* ------------------------------------------------------------------ context: the dilation of H by line number */

/* the bits of word w of a bitmap by line number that stand for lines: those below numLines */
__device__ __forceinline__ uint32_t lineBitsOf(unsigned int numLines, unsigned int k0)
{
    return k0 >= numLines ? 0u : (numLines - k0 >= 32u ? 0xFFFFFFFFu : (1u << (numLines - k0)) - 1u);
}

/* x with every bit also set in the s <= 31 places above it (below it): shifts of 1, 2, 4, ... that add up to s reach every distance up to s */
__device__ __forceinline__ uint32_t smearUp(uint32_t x, uint32_t s)
{
    for (uint32_t d = 1; s != 0; d <<= 1) {
        const uint32_t t = d < s ? d : s;
        x |= x << t;
        s -= t;
    }
    return x;
}
__device__ __forceinline__ uint32_t smearDown(uint32_t x, uint32_t s)
{
    for (uint32_t d = 1; s != 0; d <<= 1) {
        const uint32_t t = d < s ? d : s;
        x |= x >> t;
        s -= t;
    }
    return x;
}

/* a word h of H's bitmap whose first line is k0: k + 1 of its last member (0: none), and ~k of its first -- the nearer to k0, the larger; never 0
 * for a member, k < 2^31 */
__device__ __forceinline__ unsigned int lastMemberOf(uint32_t h, unsigned int k0) { return h ? k0 + 32u - (unsigned int)__clz((int)h) : 0u; }
__device__ __forceinline__ unsigned int firstMemberOf(uint32_t h, unsigned int k0) { return h ? ~(k0 + (unsigned int)__ffs((int)h) - 1u) : 0u; }

/* a wave per line block: the hit bitmap becomes H's, and what the line block hands to the two running maxima and to |H| */
__global__ __launch_bounds__(kLinesThreads) void pfac_lines_members(ContextArgs a)
{
    const unsigned int lane = threadIdx.x & 63u;
    const unsigned int waves = gridDim.x * (kLinesThreads / 64);
    const unsigned int numLines = a.lineBase[a.blocks];
    for (unsigned int b = blockIdx.x * (kLinesThreads / 64) + (threadIdx.x >> 6); b < a.blocks; b += waves) {
        if ((b << kBlockShift) >= numLines) {                  /* no line here (most line blocks: a line has a byte or more): nothing reads these words */
            if (lane == 63u) { a.memberTop[b] = 0; a.memberNext[a.blocks - 1u - b] = 0; }
            continue;
        }
        const size_t w = (size_t)b * kBlockWords + lane;
        const unsigned int k0 = (b << kBlockShift) + lane * 32u;
        const uint32_t h = (a.hitBits[w] ^ a.membersInvert) & lineBitsOf(numLines, k0);
        a.hitBits[w] = h;
        const unsigned int top = waveReduce(lastMemberOf(h, k0), OpMax()), next = waveReduce(firstMemberOf(h, k0), OpMax());
        const uint32_t members = waveInclusiveScan((uint32_t)__popc(h));
        if (lane == 63u) {
            a.memberTop[b] = top;
            a.memberNext[a.blocks - 1u - b] = next;
            if (members != 0) atomicAdd(a.matching, members);
        }
    }
}

/* a wave per line block, a word per lane: the widened bitmap and its group starts */
__global__ __launch_bounds__(kLinesThreads) void pfac_lines_widen(ContextArgs a)
{
    const unsigned int lane = threadIdx.x & 63u;
    const unsigned int waves = gridDim.x * (kLinesThreads / 64);
    const unsigned int numLines = a.lineBase[a.blocks];
    const uint32_t up = a.after < 31u ? a.after : 31u, down = a.before < 31u ? a.before : 31u;
    if (blockIdx.x == 0 && threadIdx.x == 0) storeToHost(a.hostMatching, *a.matching);
    for (unsigned int b = blockIdx.x * (kLinesThreads / 64) + (threadIdx.x >> 6); b < a.blocks; b += waves) {
        if ((b << kBlockShift) >= numLines) {
            if (lane == 63u) a.groupCount[b] = 0;
            continue;
        }
        const size_t w = (size_t)b * kBlockWords + lane;
        const unsigned int k0 = (b << kBlockShift) + lane * 32u;
        const uint32_t h = a.hitBits[w];
        /* k + 1 of the nearest member in front of line k0; ~k of the nearest from line k0 + 32 on: the suffix is a prefix over the lanes back to front */
        const unsigned int prev = OpMax()(a.prevMember[b], waveExclusiveOf(waveInclusive(lastMemberOf(h, k0), OpMax())));
        const unsigned int back = (unsigned int)__shfl((int)firstMemberOf(h, k0), (int)(63u - lane));
        const unsigned int suffix = (unsigned int)__shfl((int)waveExclusiveOf(waveInclusive(back, OpMax())), (int)(63u - lane));
        const unsigned int next = OpMax()(a.nextMember[a.blocks - 1u - b], suffix);
        uint32_t sel = smearUp(h, up) | smearDown(h, down);
        uint32_t behind = 0;                                    /* line k0 - 1 is selected */
        if (prev != 0) {
            const unsigned long long reach = (unsigned long long)(prev - 1u) + a.after;        /* the last line that member selects */
            if (reach >= k0) sel |= reach - k0 >= 31u ? 0xFFFFFFFFu : (2u << (unsigned int)(reach - k0)) - 1u;
            behind = reach + 1u >= k0 ? 1u : 0u;
        }
        if (next != 0) {
            const unsigned int m = ~next, from = m > a.before ? m - a.before : 0u;              /* the first line that member selects */
            if (from <= k0 + 31u) sel |= from > k0 ? 0xFFFFFFFFu << (from - k0) : 0xFFFFFFFFu;
        }
        const unsigned int near = h ? ~firstMemberOf(h, k0) : ~next;                             /* the nearest member from line k0 on, if h | next */
        if ((h | next) != 0 && (near > a.before ? near - a.before : 0u) < k0) behind = 1u;
        sel &= lineBitsOf(numLines, k0);
        const uint32_t starts = sel & ~((sel << 1) | behind);
        const uint32_t c = (uint32_t)__popc(starts);
        const uint32_t incl = waveInclusiveScan(c);
        a.selBits[w] = sel;
        a.groupRank[w] = (uint16_t)(incl - c);
        if (lane == 63u) a.groupCount[b] = incl;
    }
}

/* ------------------------------------------------------------------ the gather */

struct GatherArgs {
    const unsigned char *in;
    size_t n;
    const int *start, *len;             /* the caller's lines: clamped, never trusted */
    size_t count;
    size_t per;                         /* lines per block of the count / offsets passes: a multiple of kLinesThreads */
    unsigned int blocks;
    unsigned long long *blockBase;      /* [blocks + 1] block totals -> their exclusive prefix; [blocks] = the size of the text */
    unsigned long long *off;            /* [count] offset of each line in the text */
    unsigned char *out;
    size_t outCapacity;
    unsigned int misOut;                /* address of out & 15 */
};

/* line i as input bytes [s, s + l) */
__device__ __forceinline__ size_t lineOf(const GatherArgs &g, size_t i, size_t &s)
{
    size_t e;
    clampSpan(g.start[i], g.len[i], g.n, s, e);
    return e - s;
}

/* line i in the text: its bytes and its newline */
__device__ __forceinline__ unsigned long long textOf(const GatherArgs &g, size_t i)
{
    size_t s;
    return lineOf(g, i, s) + 1;
}

__global__ __launch_bounds__(kLinesThreads) void pfac_lines_gather_count(GatherArgs g)
{
    offsetsBlockTotal<kLinesThreads>(g.count, g.per, g.blockBase, [&](size_t i) { return textOf(g, i); });
}

__global__ __launch_bounds__(kLinesThreads) void pfac_lines_gather_offsets(GatherArgs g)
{
    offsetsOfBlock<kLinesThreads>(g.count, g.per, g.blockBase, [&](size_t i) { return textOf(g, i); }, [&](size_t i, unsigned long long o) { g.off[i] = o; });
}

/* the text, a tile of kOutTile output bytes at a time.  Tiles are cut in v = o + misOut, the output offset counted from the aligned 16-byte block that
 * holds out[0]: a thread's 16 bytes are one aligned store unless they hang over an end of the text */
__global__ __launch_bounds__(kLinesThreads) void pfac_lines_gather_copy(GatherArgs g)
{
    __shared__ unsigned int rel[kOutTile + 1];              /* offsets of the tile's lines behind its first, relative to the tile's first byte */
    __shared__ size_t sFirst;
    __shared__ unsigned int sCount;
    const unsigned long long total = g.blockBase[g.blocks];
    const unsigned long long limit = total < g.outCapacity ? total : g.outCapacity;
    const unsigned int t = threadIdx.x;
    for (unsigned long long vLo = (unsigned long long)blockIdx.x * kOutTile; vLo < limit + g.misOut; vLo += (unsigned long long)gridDim.x * kOutTile) {
        const TileFrame<unsigned long long> f = tileFrame(vLo, g.misOut, limit);
        const unsigned long long oLo = f.oLo, oHi = f.oHi;
        if (t == 0) {
            /* the last line that starts at or in front of oLo (off[0] == 0), and the last that starts in front of oHi */
            size_t lo = 0, hi = g.count;
            while (hi - lo > 1) {
                const size_t mid = lo + (hi - lo) / 2;
                if (g.off[mid] <= oLo) lo = mid; else hi = mid;
            }
            size_t lo2 = lo, hi2 = g.count;
            while (hi2 - lo2 > 1) {
                const size_t mid = lo2 + (hi2 - lo2) / 2;
                if (g.off[mid] < oHi) lo2 = mid; else hi2 = mid;
            }
            sFirst = lo;
            const size_t c = lo2 - lo + 1;              /* offsets are strictly ascending: at most kOutTile lines start inside a tile */
            sCount = c > kOutTile ? kOutTile : (unsigned int)c;
        }
        __syncthreads();
        const size_t first = sFirst;
        const unsigned int cnt = sCount;
        for (unsigned int j = t; j < cnt; j += kLinesThreads) rel[j] = j == 0 ? 0u : (unsigned int)(g.off[first + j] - oLo);
        __syncthreads();
        const unsigned long long cLo = f.cLo;
        if (f.nb != 0) {
            const unsigned int r = (unsigned int)(cLo - oLo);
            unsigned int lo = 0, hi = cnt;
            while (hi - lo > 1) {
                const unsigned int mid = (lo + hi) / 2;
                if (rel[mid] <= r) lo = mid; else hi = mid;
            }
            size_t i = first + lo;
            unsigned long long k = lo == 0 ? cLo - g.off[first] : (unsigned long long)(r - rel[lo]);     /* bytes of line i in front of cLo */
            size_t s, l = lineOf(g, i, s);
            auto next = [&]() -> uint32_t {
                uint32_t byte = '\n';
                if (k < l) {
                    byte = g.in[s + k];
                    k++;
                } else {                                 /* the line's newline: on to the next line */
                    k = 0;
                    i++;
                    if (i < g.count) l = lineOf(g, i, s); else l = 0;
                }
                return byte;
            };
            uint32_t x[4] = {0, 0, 0, 0};
#pragma unroll
            for (unsigned int b = 0; b < 16; b++)
                if (b < f.nb) x[b >> 2] |= next() << (8 * (b & 3));
            tileStore(g.out, f, pfacmod::u32x4{x[0], x[1], x[2], x[3]});
        }
        __syncthreads();                                 /* rel is rewritten by the next tile */
    }
}

/* the arguments of the passes over the n bytes at `in`, their arrays carved from the handle's lines scratch (grow-only; exactly what a call needs:
 * a fixed function of its size): the newline pass's (select == false) or those of a whole select call.  false: no memory */
bool linesArgs(PFAC_context *c, const void *in, size_t n, bool select, LinesArgs &a)
{
    a.in = static_cast<const unsigned char *>(in);
    a.n = n;
    a.mis = (unsigned int)(reinterpret_cast<uintptr_t>(in) & 15u);
    const size_t blocks = ((size_t)a.mis + n) / (size_t(1) << kBlockShift) + 1, words = blocks * kBlockWords;      /* positions q in [0, mis + n] */
    a.blocks = (unsigned int)blocks;
    return carveScratch(c->scratch.lines, [&](ScratchCarver &k) {
        a.nlBits = k.take<uint32_t>(words);
        a.hitBits = k.take<uint32_t>(words, 256);              /* and the word a funnel may read behind it */
        a.rank = k.take<uint16_t>(words);
        if (select) {
            a.lineBase = k.take<unsigned int>(blocks + 1);
            a.lineCount = k.take<unsigned int>(blocks + 1);
            a.selBase = k.take<unsigned int>(blocks + 1);
            a.selCount = k.take<unsigned int>(blocks + 1);
            a.prevNl = k.take<unsigned int>(blocks);
            a.lastNl = k.take<unsigned int>(blocks);
        } else {
            a.lineCount = k.take<unsigned int>(blocks);
        }
    }) == PFAC_STATUS_SUCCESS;
}

/* ... and what the context stage adds, from the handle's context scratch (a buffer of its own: a plain lines call allocates none of it) */
bool contextArgs(PFAC_context *c, ContextArgs &a)
{
    const size_t blocks = a.blocks, words = blocks * kBlockWords;
    return carveScratch(c->scratch.linesContext, [&](ScratchCarver &k) {
        a.selBits = k.take<uint32_t>(words, 256);               /* and the word a funnel may read behind it */
        a.groupRank = k.take<uint16_t>(words);
        a.memberTop = k.take<unsigned int>(blocks);
        a.memberNext = k.take<unsigned int>(blocks);
        a.prevMember = k.take<unsigned int>(blocks + 1);
        a.nextMember = k.take<unsigned int>(blocks);
        a.groupCount = k.take<unsigned int>(blocks);
        a.groupBase = k.take<unsigned int>(blocks + 1);
        a.matching = k.take<unsigned int>(1);
    }) == PFAC_STATUS_SUCCESS;
}

/* the grid of the passes that take a block of positions per wave */
unsigned int waveGridFor(const PFAC_context *c, unsigned int blocks) { return (blocks + 3) / 4 < gridCap(c, 8) ? (blocks + 3) / 4 : gridCap(c, 8); }

} // namespace

extern "C" {

PFAC_status_t PFACX_linesSelect(PFAC_handle_t handle, const char *d_input, char *d_scan, size_t size, int invert, int hashed, int *d_lineStart,
                                int *d_lineLen, int *d_lineIndex, size_t *h_numLines, size_t *h_numSelected)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!d_input || !d_scan || !d_lineStart || !d_lineLen || !h_numLines || !h_numSelected || size == 0 || size > (size_t)0x7fffffff)
        return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = handle;
    LinesArgs a{};
    if (!linesArgs(c, d_input, size, true, a)) return PFAC_STATUS_CUDA_ALLOC_FAILED;
    a.invert = invert ? 0xFFFFFFFFu : 0u;
    a.lineStart = d_lineStart;
    a.lineLen = d_lineLen;
    a.lineIndex = d_lineIndex;
    const HostHandoff counts(c, pfac::kHostLines);             /* the lines, then the selected lines */
    const unsigned int waveGrid = waveGridFor(c, a.blocks);

    /* the line index in front of the scan, on the same stream */
    hipLaunchKernelGGL(pfac_lines_bitmap, dim3(waveGrid), dim3(kLinesThreads), 0, 0, a);
    blockScan<OpSum>({{a.lineCount}, {a.lineBase}}, a.blocks, counts.word(0), nullptr);
    if (hipGetLastError() != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;

    /* the compacted scan, pairs in any order (the four ordering launches are not paid for): ids in d_lineStart, positions in d_lineLen */
    size_t count = 0;
    const PFAC_status_t st = compactedScan(handle, d_scan, size, hashed, d_lineStart, d_lineLen, false, &count);
    if (st != PFAC_STATUS_SUCCESS) return st;

    if (count > 0) hipLaunchKernelGGL(pfac_lines_mark, dim3(gridFor(c, count)), dim3(kLinesThreads), 0, 0, a, (const int *)d_lineLen, (unsigned int)count);
    hipLaunchKernelGGL(pfac_lines_select<0>, dim3(waveGrid), dim3(kLinesThreads), 0, 0, a);
    blockScan<OpSum, OpMax, 2>({{a.selCount, a.lastNl}, {a.selBase, a.prevNl}}, a.blocks, counts.word(1), nullptr);
    hipLaunchKernelGGL(pfac_lines_select<1>, dim3(waveGrid), dim3(kLinesThreads), 0, 0, a);
    unsigned int lines[2] = {0, 0};                            /* all, selected */
    if (!counts.finish(lines, a.lineBase + a.blocks, a.selBase + a.blocks)) return PFAC_STATUS_INTERNAL_ERROR;
    if (lines[0] > size || lines[1] > lines[0]) return PFAC_STATUS_INTERNAL_ERROR;
    *h_numLines = lines[0];
    *h_numSelected = lines[1];
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_linesSelectContext(PFAC_handle_t handle, const char *d_input, char *d_scan, size_t size, int invert, int hashed,
                                       unsigned int before, unsigned int after, int *d_lineStart, int *d_lineLen, int *d_lineIndex, int *d_lineTag,
                                       size_t *h_numLines, size_t *h_numSelected, size_t *h_numMatching, size_t *h_numGroups)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!d_input || !d_scan || !d_lineStart || !d_lineLen || !h_numLines || !h_numSelected || !h_numMatching || !h_numGroups || size == 0 ||
        size > (size_t)0x7fffffff)
        return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = handle;
    ContextArgs a{};
    if (!linesArgs(c, d_input, size, true, a) || !contextArgs(c, a)) return PFAC_STATUS_CUDA_ALLOC_FAILED;
    a.invert = 0;                                               /* the select passes read the widened bitmap as it is */
    a.membersInvert = invert ? 0xFFFFFFFFu : 0u;
    a.before = before;
    a.after = after;
    a.lineStart = d_lineStart;
    a.lineLen = d_lineLen;
    a.lineIndex = d_lineIndex;
    a.lineTag = d_lineTag;
    const HostHandoff counts(c, pfac::kHostLinesContext);      /* the lines, the selected lines, the matching lines, the groups */
    a.hostMatching = counts.word(2);
    const unsigned int waveGrid = waveGridFor(c, a.blocks);

    /* the head of a plain call: the line index, the scan, the marks; the scan of the line counts also clears the word |H| is added up in */
    hipLaunchKernelGGL(pfac_lines_bitmap, dim3(waveGrid), dim3(kLinesThreads), 0, 0, static_cast<const LinesArgs &>(a));
    blockScan<OpSum>({{a.lineCount}, {a.lineBase}}, a.blocks, counts.word(0), a.matching);
    if (hipGetLastError() != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
    size_t count = 0;
    const PFAC_status_t st = compactedScan(handle, d_scan, size, hashed, d_lineStart, d_lineLen, false, &count);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (count > 0)
        hipLaunchKernelGGL(pfac_lines_mark, dim3(gridFor(c, count)), dim3(kLinesThreads), 0, 0, static_cast<const LinesArgs &>(a), (const int *)d_lineLen,
                           (unsigned int)count);

    /* the context stage: H, the nearest members around each line block, the widened bitmap, the group starts in front of each line block */
    hipLaunchKernelGGL(pfac_lines_members, dim3(waveGrid), dim3(kLinesThreads), 0, 0, a);
    blockScan<OpMax, OpMax, 2>({{a.memberTop, a.memberNext}, {a.prevMember, a.nextMember}}, a.blocks, nullptr, nullptr);
    hipLaunchKernelGGL(pfac_lines_widen, dim3(waveGrid), dim3(kLinesThreads), 0, 0, a);
    blockScan<OpSum>({{a.groupCount}, {a.groupBase}}, a.blocks, counts.word(3), nullptr);

    /* the tail of a plain call, over the widened bitmap */
    hipLaunchKernelGGL((pfac_lines_select<0, ContextArgs>), dim3(waveGrid), dim3(kLinesThreads), 0, 0, a);
    blockScan<OpSum, OpMax, 2>({{a.selCount, a.lastNl}, {a.selBase, a.prevNl}}, a.blocks, counts.word(1), nullptr);
    hipLaunchKernelGGL((pfac_lines_select<1, ContextArgs>), dim3(waveGrid), dim3(kLinesThreads), 0, 0, a);

    unsigned int v[4] = {0, 0, 0, 0};                           /* lines, selected, matching, groups */
    if (counts.mapped()) {
        counts.queueDone();
        if (!counts.wait()) return PFAC_STATUS_INTERNAL_ERROR;
        for (int k = 0; k < 4; k++) v[k] = __atomic_load_n(const_cast<const unsigned int *>(counts.h_value) + k, __ATOMIC_ACQUIRE);
    } else {
        const unsigned int *const from[4] = {a.lineBase + a.blocks, a.selBase + a.blocks, a.matching, a.groupBase + a.blocks};
        if (hipGetLastError() != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
        for (int k = 0; k < 4; k++)
            if (hipMemcpy(&v[k], from[k], sizeof(unsigned int), hipMemcpyDeviceToHost) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
    }
    if (v[0] > size || v[1] > v[0] || v[2] > v[1] || v[3] > v[2] || (v[1] != 0) != (v[2] != 0)) return PFAC_STATUS_INTERNAL_ERROR;
    *h_numLines = v[0];
    *h_numSelected = v[1];
    *h_numMatching = v[2];
    *h_numGroups = v[3];
    return PFAC_STATUS_SUCCESS;
}

/* measurement only: the newline pass alone over the first n bytes of d_in, into the handle's lines scratch */
double PFACX_linesBitmapProbe(PFAC_handle_t handle, const void *d_in, size_t n, int launches)
{
    if (!handle || !d_in || n == 0 || n > (size_t)0x7fffffff || launches < 1) return -1.0;
    PFAC_context *c = handle;
    LinesArgs a{};
    if (!linesArgs(c, d_in, n, false, a)) return -1.0;
    const unsigned int grid = waveGridFor(c, a.blocks);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    double ms = -1.0;
    if (hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
        for (int r = 0; r < 3; r++) hipLaunchKernelGGL(pfac_lines_bitmap, dim3(grid), dim3(kLinesThreads), 0, 0, a);
        (void)hipEventRecord(e0, 0);
        for (int r = 0; r < launches; r++) hipLaunchKernelGGL(pfac_lines_bitmap, dim3(grid), dim3(kLinesThreads), 0, 0, a);
        (void)hipEventRecord(e1, 0);
        float t = 0;
        if (hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&t, e0, e1) == hipSuccess && hipGetLastError() == hipSuccess) ms = (double)t / launches;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return ms;
}

PFAC_status_t PFACX_linesGather(PFAC_handle_t handle, const char *d_input, size_t size, const int *d_lineStart, const int *d_lineLen,
                                size_t numSelected, char *d_out, size_t outCapacity, size_t *h_outBytes)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!h_outBytes || !d_lineStart || !d_lineLen || numSelected == 0 || (!d_input && size) || (!d_out && outCapacity) || size > (size_t)0x7fffffff ||
        numSelected > (size_t)0x7fffffff)
        return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = handle;
    GatherArgs g{};
    g.in = reinterpret_cast<const unsigned char *>(d_input);
    g.n = size;
    g.start = d_lineStart;
    g.len = d_lineLen;
    g.count = numSelected;
    g.out = reinterpret_cast<unsigned char *>(d_out);
    g.outCapacity = outCapacity;
    g.misOut = (unsigned int)(reinterpret_cast<uintptr_t>(d_out) & 15u);
    g.blocks = offsetBlocks(c, numSelected, kLinesThreads, g.per);
    const PFAC_status_t carved = carveScratch(c->scratch.lines, [&](ScratchCarver &k) {
        g.blockBase = k.take<unsigned long long>((size_t)g.blocks + 1);
        g.off = k.take<unsigned long long>(numSelected);
    });
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    const HostHandoff text(c, pfac::kHostGather);
    hipLaunchKernelGGL(pfac_lines_gather_count, dim3(g.blocks), dim3(kLinesThreads), 0, 0, g);
    hipLaunchKernelGGL(pfac_array_scan<unsigned long long>, dim3(1), dim3(1024), 0, 0, g.blockBase, g.blocks, g.blockBase + g.blocks,
                       reinterpret_cast<unsigned long long *>(text.d_value));
    hipLaunchKernelGGL(pfac_lines_gather_offsets, dim3(g.blocks), dim3(kLinesThreads), 0, 0, g);
    /* the text is at most (size + 1) bytes per line; whatever it is, a launch never needs more tiles than outCapacity has */
    if (outCapacity) {
        const unsigned long long bound = (unsigned long long)numSelected * (size + 1);
        const unsigned long long most = (bound < outCapacity ? bound : (unsigned long long)outCapacity) + g.misOut;
        const unsigned long long tiles = (most + kOutTile - 1) / kOutTile;
        hipLaunchKernelGGL(pfac_lines_gather_copy, dim3((unsigned int)(tiles < gridCap(c, 8) * 4ull ? tiles : gridCap(c, 8) * 4ull)), dim3(kLinesThreads), 0, 0, g);
    }
    unsigned long long total = 0;
    if (!text.finish(&total, g.blockBase + g.blocks)) return PFAC_STATUS_INTERNAL_ERROR;
    *h_outBytes = (size_t)total;
    return total > outCapacity ? PFACX_STATUS_OUTPUT_TRUNCATED : PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
