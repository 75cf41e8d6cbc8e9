/*
 * scan_verify.h -- the device frame of the six VERIFY units (scan_case.hip, scan_sig.hip, scan_approx.hip, scan_gapsig.hip, scan_edit.hip,
 * scan_clsig.hip).  Each expands an ordered list of LONGEST pairs along the prefix chains (scan_passes.h: the expansion frame), walks the class
 * of every chain member in a per-id table and verifies every candidate against the CALLER's bytes.  What is here once:
 *   InputView, alignedDword      the caller's bytes [0, n) at any alignment, and the one load that may touch their edges
 *   walkDwords, walkTail         THE DWORD WALK: the input side of [s, s + 4 words) dword by dword -- whole loads where in + s is dword-aligned, else
 *                                composed from the two aligned dwords around each with v_alignbyte, lo and hi carried --, a test every fourth
 *                                dword that may end it, and the len & 3 bytes behind the last whole dword byte by byte
 *   maskedEqual, bytesEqual, byteDistance
 *                                the three compares on it: (x ^ v) & m ORed up (sig, gapsig), x ^ v ORed up (case, clsig), the differing bytes
 *                                counted against a budget (approx)
 *   forEachClassEntry, inBlob    a class's range of its table, clamped to the table; an entry's dwords inside the blob
 *   emitWithAux                  the write pass's store of a unit with further arrays: their values at the slot the frame's store takes next
 *   verifyRunOk, verifyFrame, verifyInput
 *                                the head of every PFACX_*Run (pfac_module.h: PFACX_verifyRun_t) checked and turned into the frame and the view
 * An aligned dword that would reach outside [0, n) -- in front of in[0] where the caller's pointer is misaligned and s < 3, behind in[n - 1] at the
 * end -- is put together from its bytes inside the buffer (three at most): no load of any function here leaves [0, n), given s + len <= n.
 * Everything is __forceinline__ in an unnamed namespace: each unit its own copy, its kernels the shape they had with the code written out
 * (profiles/verify_frame_resources.txt).  scan_case.hip keeps its own class loop: it reads a flag bit of the first offset before the second and
 * ends the whole chain walk from inside the loop.
 * Plain C++ and vector stores only.
 */
#ifndef PFAC_SCAN_VERIFY_H_
#define PFAC_SCAN_VERIFY_H_

#include <cstdint>

#include "scan_passes.h"

namespace {

/* the caller's bytes: never a folded copy */
struct InputView {
    const unsigned char *in;
    unsigned int n;
};

/* the aligned dword of the input whose first byte is in[o] (o: any sign; in + o is dword-aligned): one load where it lies inside [0, n), else its
 * bytes inside the buffer, zero for the others */
__device__ __forceinline__ uint32_t alignedDword(const InputView &v, long long o)
{
    if (o >= 0 && o + 4 <= (long long)v.n) return *reinterpret_cast<const uint32_t *>(v.in + o);
    uint32_t w = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const long long i = o + b;
        if (i >= 0 && i < (long long)v.n) w |= (uint32_t)v.in[i] << (8 * b);
    }
    return w;
}

/* fold(k, x) for x = the dword in[s + 4 k ...], k < words, ascending; behind every fourth of them over() is asked, and true ends the walk: the
 * return value.  s + 4 words <= n (the caller has checked) */
template <class Fold, class Over>
__device__ __forceinline__ bool walkDwords(const InputView &v, unsigned int s, unsigned int words, Fold fold, Over over)
{
    const unsigned int r = (unsigned int)(reinterpret_cast<uintptr_t>(v.in + s) & 3u);
    if (r == 0) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(v.in + s);       /* whole dwords inside [s, s + 4 words) */
        for (unsigned int k = 0; k < words; k++) {
            fold(k, src[k]);
            if ((k & 3u) == 3u && over()) return true;
        }
    } else {
        const long long base = (long long)s - (long long)r;                     /* the aligned dword that holds in[s] */
        uint32_t lo = words ? alignedDword(v, base) : 0u;
        for (unsigned int k = 0; k < words; k++) {
            const uint32_t hi = alignedDword(v, base + 4ll * (k + 1u));
            fold(k, __builtin_amdgcn_alignbyte(hi, lo, r));
            if ((k & 3u) == 3u && over()) return true;
            lo = hi;
        }
    }
    return false;
}

/* differs(b, x) for x = the byte in[s + 4 (len / 4) + b], b < len & 3: the bytes behind the last whole dword; true ends it: the return value */
template <class Differs>
__device__ __forceinline__ bool walkTail(const InputView &v, unsigned int s, unsigned int len, Differs differs)
{
    const unsigned int tail = len & 3u, at = s + (len & ~3u);
    for (unsigned int b = 0; b < tail; b++)
        if (differs(b, (uint32_t)v.in[at + b])) return true;
    return false;
}

/* ((in[s + k] ^ value[k]) & mask[k]) == 0 for every k < len?  val: the (len + 3) / 4 value dwords, as many mask dwords behind them.  s + len <= n
 * and the dwords lie inside their blob (the caller has checked both) */
__device__ __forceinline__ bool maskedEqual(const InputView &v, const uint32_t *val, unsigned int s, unsigned int len)
{
    const unsigned int words = len >> 2;
    const uint32_t *mask = val + ((len + 3u) >> 2);
    uint32_t diff = 0;
    if (walkDwords(v, s, words, [&](unsigned int k, uint32_t x) { diff |= (x ^ val[k]) & mask[k]; }, [&]() { return diff != 0; })) return false;
    if (diff != 0) return false;
    if (len & 3u) {
        const uint32_t tv = val[words], tm = mask[words];
        if (walkTail(v, s, len, [&](unsigned int b, uint32_t x) { return ((x ^ (tv >> (8u * b))) & (tm >> (8u * b)) & 0xFFu) != 0u; })) return false;
    }
    return true;
}

/* in[s, s + len) == the len bytes at pat?  s + len <= n and the (len + 3) / 4 dwords lie inside their blob (the caller has checked both) */
__device__ __forceinline__ bool bytesEqual(const InputView &v, const uint32_t *pat, unsigned int s, unsigned int len)
{
    const unsigned int words = len >> 2;
    uint32_t diff = 0;
    if (walkDwords(v, s, words, [&](unsigned int k, uint32_t x) { diff |= x ^ pat[k]; }, [&]() { return diff != 0; })) return false;
    if (diff != 0) return false;
    if (len & 3u) {
        const uint32_t last = pat[words];
        if (walkTail(v, s, len, [&](unsigned int b, uint32_t x) { return ((x ^ (last >> (8u * b))) & 0xFFu) != 0u; })) return false;
    }
    return true;
}

/* the number of non-zero bytes of x: bit 7 of a byte is set iff its low seven bits carry into it or it is set itself, then a popcount */
__device__ __forceinline__ unsigned int differingBytes(uint32_t x)
{
    return (unsigned int)__popc((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u);
}

/* #{t < len : in[s + t] != pat[t]}, or some value > budget where it is more than budget: a candidate that is far off ends early.  s + len <= n
 * and the (len + 3) / 4 dwords lie inside their blob (the caller has checked both) */
__device__ __forceinline__ unsigned int byteDistance(const InputView &v, const uint32_t *pat, unsigned int s, unsigned int len, unsigned int budget)
{
    const unsigned int words = len >> 2;
    unsigned int d = 0;
    if (walkDwords(v, s, words, [&](unsigned int k, uint32_t x) { d += differingBytes(x ^ pat[k]); }, [&]() { return d > budget; })) return d;
    if (len & 3u) {
        const uint32_t last = pat[words];
        (void)walkTail(v, s, len, [&](unsigned int b, uint32_t x) { d += (x ^ (last >> (8u * b))) & 0xFFu ? 1u : 0u; return false; });
    }
    return d;
}

/* f(e) for the entries e of class q of a table in CSR form by id (off: numIds + 2 entries), the range clamped to the table's numEntries */
template <class F>
__device__ __forceinline__ void forEachClassEntry(const unsigned int *off, unsigned int numEntries, int q, F f)
{
    const unsigned int first = off[q];
    unsigned int end = off[q + 1];
    if (end > numEntries) end = numEntries;
    for (unsigned int e = first; e < end; e++) f(e);
}

/* do the `need` dwords at blob[off ...] lie inside a blob of blobWords?  (a table of the library's own: always) */
__device__ __forceinline__ bool inBlob(unsigned int blobWords, unsigned int off, unsigned int need) { return off < blobWords && blobWords - off >= need; }

/* The store of a write pass with one further array, or two: each value goes to the slot the frame's store takes next -- a null array is skipped
 * --, under the emit's own slot and capacity, then (id, at) through the frame (scan_passes.h: ExpandEmit) */
template <class Emit>
__device__ __forceinline__ void emitWithAux(const Emit &emit, int id, int at, int *aux, int value)
{
    if (aux != nullptr && emit.o < emit.f.capacity) aux[emit.o] = value;
    emit(id, at);
}
template <class Emit>
__device__ __forceinline__ void emitWithAux(const Emit &emit, int id, int at, int *aux1, int value1, int *aux2, int value2)
{
    if (emit.o < emit.f.capacity) {
        if (aux1 != nullptr) aux1[emit.o] = value1;
        if (aux2 != nullptr) aux2[emit.o] = value2;
    }
    emit(id, at);
}

/* what every PFACX_*Run checks of the head of its run (the blob: where it has dwords; a unit that needs one says so itself) */
inline bool verifyRunOk(const PFACX_verifyRun_t &v, const size_t *h_total)
{
    constexpr size_t kMax = 0x7fffffff;
    return h_total && v.d_input && v.size != 0 && v.size <= kMax && v.numIds <= kMax - 1 && v.blobWords <= kMax && (v.blobWords == 0 || v.d_blob) &&
           v.count <= kMax && (v.count == 0 || (v.d_pairIds && v.d_pairPos)) && (v.capacity == 0 || (v.d_ids && v.d_pos));
}

/* ... and makes of it: the expansion frame (the block cut and blockBase are expandPasses') and the view */
inline ExpandFrame verifyFrame(const PFACX_verifyRun_t &v, unsigned int all = 1u)
{
    return ExpandFrame{v.d_pairIds, v.d_pairPos, v.count, static_cast<const pfac::Int2 *>(v.d_table), (unsigned int)v.numIds, all, 0, nullptr, v.d_ids, v.d_pos,
                       v.capacity};
}
inline InputView verifyInput(const PFACX_verifyRun_t &v) { return InputView{reinterpret_cast<const unsigned char *>(v.d_input), (unsigned int)v.size}; }

} // namespace

#endif
