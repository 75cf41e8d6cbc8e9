/*
 * scan_passes.h -- what the passes around the scan share (scan_module.hip with scan_order.inc, scan_batch.hip, scan_all.hip, scan_fold.hip,
 * scan_stream.hip, scan_flows.hip, scan_lines.hip, scan_spans.hip, scan_count.hip, scan_disjoint.hip, scan_rules.hip, scan_words.hip, scan_segcount.hip, scan_groups.hip, scan_case.hip, scan_sig.hip, scan_approx.hip and, through scan_cuts.h, scan_split.hip and scan_locate.hip; the product kernels' units do
 * not include it): launch sizes, the layout of a call's scratch and its carving out of a buffer of the handle (ScratchCarver, carveScratch), the
 * compacted scan as a pass runs it, the hand-off of a call's result to the host through mapped memory (HostHandoff; storeToHost on the device),
 * the device fold byte, the exact SWAR test of four bytes against one (bytesEqual4), the clamp of a caller's (start, len), 16 bytes out of two aligned blocks (funnel, loadBytes16), the frame of an output
 * tile and its store tail (kOutTile, tileFrame, tileStore), wave and block prefixes
 * under a sum or a maximum, the 64-ary search of a wave (waveLowerBound), the two scan kernels (pfac_array_scan: one block, in place;
 * pfac_block_scan: a block per 8192 values that folds what lies in front of them), the two passes that give items of 64-bit values their offsets
 * (offsetBlocks, offsetsBlockTotal, offsetsOfBlock), the frame and the launches of a pass that takes whole segments and works their pairs
 * through windows of an LDS table (clampFirstPair, SegmentFrame, segmentWindows, carveSegFirst, segmentWindowPasses: the rules and the
 * count-batch passes), the walk along a pattern's prefix chain (forEachChainMember: the one such loop on the device) with the frame and the
 * launches of a pass that expands longest pairs into the members of their chains (ExpandFrame, expandCount, expandWrite, expandPasses: the
 * all-match, the words, the groups, the case, the signature and the approximate passes), the pairs of an ordered scan with the head, the tail and the finish kernel of a select call over them (PairArgs,
 * pairsSelectHead, pairsSelectTail, pfac_pairs_finish), the seam of a stream.  Like scan_common.h, everything is in an unnamed namespace: inline
 * device code, each unit its own copy.
 */
#ifndef PFAC_SCAN_PASSES_H_
#define PFAC_SCAN_PASSES_H_

#include "scan_common.h"
#include "pfac_module.h"

namespace pfacmod {
/* scan_module.hip: queues pfac_host_done, the one-store kernel that writes `seq` to a word of mapped host memory, on the default stream */
void queueHostDone(unsigned int *d_done, unsigned int seq);
}

namespace {

/* ------------------------------------------------------------------ launch and scratch sizes */

inline size_t round256(size_t b) { return (b + 255) & ~size_t(255); }

/* the most blocks a grid-stride launch asks for: perCu per compute unit */
inline unsigned int gridCap(const PFAC_context *c, unsigned int perCu) { return (unsigned int)(c->multiProcessorCount > 0 ? c->multiProcessorCount : 256) * perCu; }

/* blocks of 256 threads for `items` items, one at least, eight per compute unit at most */
inline unsigned int gridFor(const PFAC_context *c, size_t items)
{
    const size_t cap = gridCap(c, 8), blocks = (items + 255) / 256;
    return (unsigned int)(blocks < 1 ? 1 : blocks > cap ? cap : blocks);
}

/* The layout of a call's scratch: regions in the order they are taken, each rounded up to 256 bytes (extraBytes: what a region holds behind its
 * `count` entries).  Without a base it only counts: a layout function runs once for `bytes`, and again over the reserved buffer for the pointers */
struct ScratchCarver {
    char *base = nullptr;
    size_t bytes = 0;
    template <class T>
    T *take(size_t count, size_t extraBytes = 0)
    {
        T *at = base ? reinterpret_cast<T *>(base + bytes) : nullptr;
        bytes += round256(count * sizeof(T) + extraBytes);
        return at;
    }
};

/* A call's regions out of one of the handle's grow-only buffers: `layout` (it takes a ScratchCarver &) runs once without a base for the bytes and
 * again over the buffer for the pointers; *bytes (where given) = what the regions take.  A buffer that has to grow loses its contents; halfMore:
 * it is then reserved with half as much again as the call needs (the all-match expansion).  No memory: the status of the reserve, and no pointer
 * is valid */
template <class Layout>
inline PFAC_status_t carveScratch(pfac::DeviceBuffer<char> &buffer, Layout layout, size_t *bytes = nullptr, bool halfMore = false)
{
    ScratchCarver k;
    layout(k);
    if (buffer.count() < k.bytes) {
        const PFAC_status_t st = buffer.reserve(k.bytes + (halfMore ? k.bytes / 2 : 0));
        if (st != PFAC_STATUS_SUCCESS) return st;
    }
    if (bytes != nullptr) *bytes = k.bytes;
    k = ScratchCarver{buffer.get()};
    layout(k);
    return PFAC_STATUS_SUCCESS;
}

/* The compacted scan of d_scan[0, size) as a pass runs it: the (id, position) pairs into d_ids / d_pos (`size` entries each), in position order or
 * -- the four ordering launches not paid for -- in any; *count is inside [0, size].  The handle's own setting is put back */
inline PFAC_status_t compactedScan(PFAC_handle_t handle, char *d_scan, size_t size, int hashed, int *d_ids, int *d_pos, bool ordered, size_t *count)
{
    int found = 0;
    const bool wasUnordered = handle->reduceUnordered;
    handle->reduceUnordered = !ordered;
    const PFAC_status_t st = (hashed ? PFAC_reduce_inplace_kernel : PFAC_reduce_kernel)(handle, reinterpret_cast<int *>(d_scan), (int)size, d_ids, d_pos, &found, nullptr, nullptr);
    handle->reduceUnordered = wasUnordered;
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (found < 0 || (size_t)found > size) return PFAC_STATUS_INTERNAL_ERROR;
    *count = (size_t)found;
    return PFAC_STATUS_SUCCESS;
}

/* ------------------------------------------------------------------ the hand-off to the host */

/* The host's wait for the sequence number (never 0) that the last launch of a call writes into a word of the handle's mapped host memory: polled for
 * 20 ms, then a stream sync.  Says how it ended */
enum class HostWait { Polled, Synced, SyncFailed };
inline HostWait waitHostSeq(const volatile unsigned int *word, unsigned int seq)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned int spins = 0; __atomic_load_n(const_cast<const unsigned int *>(word), __ATOMIC_ACQUIRE) != seq; spins++) {
        if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20))
            return hipStreamSynchronize(0) == hipSuccess ? HostWait::Synced : HostWait::SyncFailed;
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#endif
    }
    return HostWait::Polled;
}

inline bool hostMapped(const PFAC_context *c) { return c->h_modeHint != nullptr && c->d_modeHint != nullptr; }

/* One call's hand-off through a slot of the handle's mapped words (pfac_context.h: HostSlot; the handle has them: hostMapped).  The call's
 * launches write what they hand over at d_value and, behind everything else, `seq` at d_done -- the call's last kernel where that kernel stores
 * the value too, else pfac_host_done (queueDone); the host then waits and reads h_value.  A slot's done word is only ever compared with the
 * number issued to the call that waits on it, so the handle counts all its calls with one counter.  On a handle without mapped words the
 * hand-off is empty (d_value is null: the kernels skip their host stores) and finish() copies from device memory instead */
struct HostHandoff {
    unsigned int *d_value = nullptr, *d_done = nullptr;
    volatile unsigned int *h_value = nullptr, *h_done = nullptr;
    unsigned int seq = 0;

    HostHandoff() = default;
    HostHandoff(PFAC_context *c, pfac::HostSlot slot)
    {
        if (!hostMapped(c)) return;
        d_value = c->d_modeHint + slot.value;
        d_done = c->d_modeHint + slot.done;
        h_value = c->h_modeHint + slot.value;
        h_done = c->h_modeHint + slot.done;
        c->hostSeq = c->hostSeq + 1u ? c->hostSeq + 1u : 1u;
        seq = c->hostSeq;
    }
    void queueDone() const { pfacmod::queueHostDone(d_done, seq); }
    /* true: every launch was queued and the done word holds the call's number (a wait that ended in a stream sync included) */
    bool wait(HostWait *how = nullptr) const
    {
        if (hipGetLastError() != hipSuccess) return false;
        const HostWait w = waitHostSeq(h_done, seq);
        if (how != nullptr) *how = w;
        return w == HostWait::Polled || (w == HostWait::Synced && __atomic_load_n(const_cast<const unsigned int *>(h_done), __ATOMIC_ACQUIRE) == seq);
    }
    bool mapped() const { return d_done != nullptr; }
    /* the device address of word k of the value (null: none) */
    unsigned int *word(unsigned int k) const { return mapped() ? d_value + k : nullptr; }
    /* The end of the call, behind its last launch: out[0] (and out[1], given d_second) = what the launches handed over -- queueDone, wait and the
     * mapped value, or, without mapped words, the values the launches left at d_first (and d_second), copied.  false: a launch or the wait failed */
    template <class T>
    bool finish(T *out, const T *d_first, const T *d_second = nullptr) const
    {
        if (!mapped())
            return hipGetLastError() == hipSuccess && hipMemcpy(out, d_first, sizeof(T), hipMemcpyDeviceToHost) == hipSuccess &&
                   (d_second == nullptr || hipMemcpy(out + 1, d_second, sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
        queueDone();
        if (!wait()) return false;
        const T *h = reinterpret_cast<const T *>(const_cast<const unsigned int *>(h_value));
        for (int k = 0; k < (d_second ? 2 : 1); k++) out[k] = __atomic_load_n(h + k, __ATOMIC_ACQUIRE);
        return true;
    }
};

/* a kernel's side of it: v (and v1 in the word behind it) to the call's mapped host words, if the handle has them.  No sequence number: the
 * call's done word is written by a later launch (scan_stream.hip and scan_flows.hip release theirs in the same kernel, and do not use this) */
template <class T>
__device__ __forceinline__ void storeToHost(T *host, T v)
{
    if (host == nullptr) return;
    __hip_atomic_store(host, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
}
template <class T>
__device__ __forceinline__ void storeToHost(T *host, T v, T v1)
{
    if (host == nullptr) return;
    __hip_atomic_store(host, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(host + 1, v1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
}

/* ------------------------------------------------------------------ the fold of a byte */

/* pfac::asciiFold on the device, for a caseless set (fold != 0) */
__device__ __forceinline__ unsigned char foldByte(unsigned char b, uint32_t fold) { return (unsigned char)(b + ((fold != 0 && (unsigned)(b - 'A') < 26u) ? 32 : 0)); }

/* ------------------------------------------------------------------ four bytes against one (scan_lines.hip, scan_cuts.h) */

/* bits 7, 15, 23, 31 of m -- one per byte -- as a nibble, byte 0 in bit 0: the four products land on bits 21..24 and nothing carries */
__device__ __forceinline__ uint32_t nibbleOf(uint32_t m) { return (((m >> 7) * 0x00204081u) >> 21) & 0xFu; }

/* bit i: byte i of x equals byte i of rep, the wanted byte in all four places (exact: the carry of a byte's low seven bits never leaves it) */
__device__ __forceinline__ uint32_t bytesEqual4(uint32_t x, uint32_t rep)
{
    const uint32_t t = x ^ rep;
    return nibbleOf(~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u);
}

/* ------------------------------------------------------------------ a caller's (start, len); 16 bytes off alignment */

/* a caller's (start, len) as [s, e) inside [0, n]: clamped where it is read, never trusted (I: the width the caller counts bytes in) */
template <class I>
__device__ __forceinline__ void clampSpan(int start, int len, I n, I &s, I &e)
{
    s = start < 0 ? (I)0 : ((I)start > n ? n : (I)start);
    e = len <= 0 ? s : ((I)len > n - s ? n : s + (I)len);
}

/* 16 bytes starting m = 4 Q + r bytes into the 32 of a | b: four v_alignbyte */
template <int Q>
__device__ __forceinline__ u32x4 funnel(u32x4 a, u32x4 b, uint32_t r)
{
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    return u32x4{__builtin_amdgcn_alignbyte(w[Q + 1], w[Q], r), __builtin_amdgcn_alignbyte(w[Q + 2], w[Q + 1], r),
                 __builtin_amdgcn_alignbyte(w[Q + 3], w[Q + 2], r), __builtin_amdgcn_alignbyte(w[Q + 4], w[Q + 3], r)};
}

/* in[o, o + 16) of a buffer of n bytes, o + 16 <= n: one aligned load, two and a funnel, or -- where an aligned block would reach outside the buffer -- sixteen bytes */
__device__ __forceinline__ u32x4 loadBytes16(const unsigned char *in, unsigned int n, unsigned int o)
{
    const unsigned int m = (unsigned int)(reinterpret_cast<uintptr_t>(in + o) & 15u);         /* the redaction: the same in every thread of a launch */
    if (m == 0) return __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(in + o));
    if (o >= m && o - m + 32u <= n) {
        const u32x4 *blk = reinterpret_cast<const u32x4 *>(in + o - m);
        const u32x4 x = __builtin_nontemporal_load(blk), y = __builtin_nontemporal_load(blk + 1);
        switch (m >> 2) {
        case 0: return funnel<0>(x, y, m & 3u);
        case 1: return funnel<1>(x, y, m & 3u);
        case 2: return funnel<2>(x, y, m & 3u);
        default: return funnel<3>(x, y, m & 3u);
        }
    }
    uint32_t w[4];
#pragma unroll
    for (int d = 0; d < 4; d++)
        w[d] = (uint32_t)in[o + 4 * d] | (uint32_t)in[o + 4 * d + 1] << 8 | (uint32_t)in[o + 4 * d + 2] << 16 | (uint32_t)in[o + 4 * d + 3] << 24;
    return u32x4{w[0], w[1], w[2], w[3]};
}

/* ------------------------------------------------------------------ output tiles (the gather, the redaction, the replacement) */

/* An output of `limit` bytes is written a TILE of kOutTile bytes at a time by blocks of 256 threads, 16 bytes a thread.  Tiles are cut in
 * v = o + misOut, the output offset counted from the aligned 16-byte block that holds out[0] (misOut = address of out & 15): a thread's 16 bytes
 * are one aligned store unless they hang over an end of the output */
constexpr unsigned int kOutTile = 4096;

/* the tile that starts at vLo (a multiple of kOutTile) as output bytes [oLo, oHi), and this thread's bytes of it, [cLo, cLo + nb) (nb == 0: none;
 * whole: all sixteen, aligned).  I: the width the caller counts output bytes in */
template <class I>
struct TileFrame {
    I oLo, oHi, cLo;
    unsigned int nb;
    bool whole;
};
template <class I>
__device__ __forceinline__ TileFrame<I> tileFrame(unsigned long long vLo, unsigned int misOut, I limit)
{
    TileFrame<I> f;
    f.oLo = vLo > misOut ? (I)(vLo - misOut) : (I)0;
    const unsigned long long oEnd = vLo + kOutTile - misOut;
    f.oHi = oEnd < limit ? (I)oEnd : limit;
    const unsigned long long v0 = vLo + (unsigned long long)threadIdx.x * 16;
    f.cLo = v0 > misOut ? (I)(v0 - misOut) : (I)0;
    const I cHi = v0 + 16 > misOut ? (v0 + 16 - misOut < f.oHi ? (I)(v0 + 16 - misOut) : f.oHi) : (I)0;
    f.nb = f.cLo < cHi ? (unsigned int)(cHi - f.cLo) : 0u;
    f.whole = f.nb == 16u && v0 >= misOut;
    return f;
}

/* the thread's bytes out (byte b: bits 8 (b & 3) of word b >> 2 of x): one aligned 16-byte store, or bytes where the 16 hang over an end */
template <class I>
__device__ __forceinline__ void tileStore(unsigned char *out, const TileFrame<I> &f, u32x4 x)
{
    if (f.whole) {
        __builtin_nontemporal_store(x, reinterpret_cast<u32x4 *>(out + f.cLo));
    } else {
        const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (unsigned int b = 0; b < 16; b++)
            if (b < f.nb) out[f.cLo + b] = (unsigned char)(w[b >> 2] >> (8 * (b & 3)));
    }
}

/* ------------------------------------------------------------------ wave and block prefixes */

/* the operators of a prefix: the sum, and the maximum of unsigned values; 0 is the identity of both */
struct OpSum {
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct OpMax {
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; }
};

/* inclusive prefix over the 64 lanes: 32-bit sums by DPP (waveInclusiveScan), everything else by shuffles */
template <class T, class Op = OpSum>
__device__ __forceinline__ T waveInclusive(T v, Op op = Op())
{
    if constexpr (sizeof(T) == 4 && std::is_same<Op, OpSum>::value) {
        return (T)waveInclusiveScan((uint32_t)v);
    } else {
        const unsigned int lane = threadIdx.x & 63u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const T up = __shfl_up(v, d);
            if ((int)lane >= d) v = op(v, up);
        }
        return v;
    }
}

/* what an inclusive prefix leaves in front of each lane: the identity in front of lane 0 */
template <class T>
__device__ __forceinline__ T waveExclusiveOf(T incl)
{
    const T up = __shfl_up(incl, 1);
    return (threadIdx.x & 63u) == 0 ? (T)0 : up;
}

/* all 64 lanes' values under op, in every lane */
template <class T, class Op>
__device__ __forceinline__ T waveReduce(T v, Op op)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d));
    return v;
}

/* the first i of [lo, hi) with pred(i), hi if there is none, for a pred that is false, then true (any other pred: some index of [lo, hi]); the
 * whole wave calls it and gets the same answer: a probe per lane and round, the range shrinks 65-fold a round */
template <class P>
__device__ __forceinline__ unsigned int waveLowerBound(unsigned int lo, unsigned int hi, P pred)
{
    const unsigned int lane = threadIdx.x & 63u;
    while (hi - lo > 64u) {
        const unsigned long long width = hi - lo;
        const unsigned int at = lo + (unsigned int)(width * (lane + 1u) / 65u);                  /* ascending, distinct, inside [lo, hi) */
        const unsigned long long yes = __ballot(pred(at));
        if (yes == 0) {
            lo = lo + (unsigned int)(width * 64u / 65u) + 1u;
        } else {
            const unsigned int f = (unsigned int)__ffsll((long long)yes) - 1u;
            hi = lo + (unsigned int)(width * (f + 1u) / 65u);
            if (f > 0) lo = lo + (unsigned int)(width * f / 65u) + 1u;
        }
    }
    const unsigned long long yes = __ballot(lane < hi - lo && pred(lo + lane));
    return yes == 0 ? hi : lo + (unsigned int)__ffsll((long long)yes) - 1u;
}

/* exclusive prefix of `own` over the block's BLOCK threads, and the block's total (every thread calls it, every thread gets both);
 * waveSum: BLOCK / 64 entries of LDS, free again at the next call */
template <unsigned int BLOCK, class T, class Op = OpSum>
__device__ __forceinline__ T blockExclusive(T own, T *waveSum, T &total, Op op = Op())
{
    const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const T incl = waveInclusive(own, op);
    T excl;
    if constexpr (std::is_same<Op, OpSum>::value) excl = incl - own;
    else excl = waveExclusiveOf(incl);
    __syncthreads();                                    /* waveSum may still be read from the previous call */
    if (lane == 63) waveSum[wave] = incl;
    __syncthreads();
    T before = 0;
    total = 0;
#pragma unroll
    for (unsigned int w = 0; w < BLOCK / 64; w++) {
        const T s = waveSum[w];
        before = w < wave ? op(before, s) : before;
        total = op(total, s);
    }
    return op(before, excl);
}

/* exclusive prefix sum of v[0, n) in place, the sum to *total (callers that keep it pass v + n) and *hostTotal where given: one block of
 * 1024 threads walks the array 1024 entries at a time */
template <class T>
__global__ __launch_bounds__(1024) void pfac_array_scan(T *v, unsigned int n, T *total, T *hostTotal)
{
    __shared__ T waveSum[16];
    __shared__ T carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (unsigned int base = 0; base < n; base += 1024) {
        const unsigned int i = base + threadIdx.x;
        const T x = i < n ? v[i] : (T)0;
        const T incl = waveInclusive(x);
        if (lane == 63) waveSum[wave] = incl;
        __syncthreads();
        T before = carry;
        for (unsigned int w = 0; w < wave; w++) before += waveSum[w];
        if (i < n) v[i] = before + incl - x;
        __syncthreads();
        if (threadIdx.x == 1023) carry = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (total != nullptr) *total = carry;
        storeToHost(hostTotal, carry);
    }
}

/* The block-value scan: for each of COLS columns of n values, out[0, n) = the exclusive prefix of in[0, n) under the column's operator (Op0, Op1;
 * 0 in front of the first).  A block of 1024 threads per kScanBlock values; block k folds everything in front of its values itself -- coalesced,
 * from L2, at most 4 n bytes a column -- so no block waits on another and there is no chain of steps (one block walking the 512 Ki counts of a
 * 1 GiB input took longer than the newline pass).  in and out are different arrays: the blocks read each other's input.  The first column also
 * gets its total: to out[n] and, where given, to *hostTotal (mapped host memory); a second column has n entries of out and rides along in the
 * same launch.  zero (or null): a word that block 0 clears for the launches behind this one */
constexpr unsigned int kScanPer = 8;                            /* values per thread */
constexpr unsigned int kScanBlock = 1024 * kScanPer;            /* values per block: whole 16-byte loads in front of every block */
static_assert(kScanBlock % 4 == 0, "the front of a block is folded four values a load");

struct ScanColumns {
    const unsigned int *in[2];
    unsigned int *out[2];
};

template <class Op0, class Op1 = Op0, unsigned int COLS = 1>
__global__ __launch_bounds__(1024) void pfac_block_scan(ScanColumns s, unsigned int n, unsigned int *hostTotal, unsigned int *zero)
{
    struct ColumnOp {                                           /* c is a constant wherever the loops over the columns are unrolled */
        unsigned int c;
        __device__ __forceinline__ unsigned int operator()(unsigned int a, unsigned int b) const { return c == 0 ? Op0()(a, b) : Op1()(a, b); }
    };
    __shared__ unsigned int waveOwn[COLS][16], waveFront[COLS][16];
    const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned int base = blockIdx.x * kScanBlock;
    const unsigned int i0 = base + threadIdx.x * kScanPer;
    if (zero != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *zero = 0;
    unsigned int front[COLS], x[COLS][kScanPer], excl[COLS];
#pragma unroll
    for (unsigned int c = 0; c < COLS; c++) front[c] = 0;
    for (unsigned int q = threadIdx.x; q < base / 4u; q += 1024u) {
#pragma unroll
        for (unsigned int c = 0; c < COLS; c++) {
            const ColumnOp op{c};
            const u32x4 v = reinterpret_cast<const u32x4 *>(s.in[c])[q];
            front[c] = op(front[c], op(op(v.x, v.y), op(v.z, v.w)));
        }
    }
#pragma unroll
    for (unsigned int c = 0; c < COLS; c++) {
        const ColumnOp op{c};
        unsigned int own = 0;
#pragma unroll
        for (unsigned int k = 0; k < kScanPer; k++) {
            x[c][k] = i0 + k < n ? s.in[c][i0 + k] : 0u;
            own = op(own, x[c][k]);
        }
        const unsigned int incl = waveInclusive(own, op);
        const unsigned int frontAll = waveReduce(front[c], op);
        excl[c] = waveExclusiveOf(incl);
        if (lane == 63) { waveOwn[c][wave] = incl; waveFront[c][wave] = frontAll; }
    }
    __syncthreads();
#pragma unroll
    for (unsigned int c = 0; c < COLS; c++) {
        const ColumnOp op{c};
        unsigned int before = 0;                                /* the fronts of all waves, and the values of the waves in front of this one */
        for (unsigned int w = 0; w < 16; w++) {
            before = op(before, waveFront[c][w]);
            if (w < wave) before = op(before, waveOwn[c][w]);
        }
        unsigned int run = op(before, excl[c]);
#pragma unroll
        for (unsigned int k = 0; k < kScanPer; k++) {
            if (i0 + k < n) s.out[c][i0 + k] = run;
            run = op(run, x[c][k]);
        }
        if (c == 0 && blockIdx.x == gridDim.x - 1 && threadIdx.x == 1023) {       /* the last thread of the last block has seen everything */
            s.out[0][n] = run;
            storeToHost(hostTotal, run);
        }
    }
}

/* the launch: the one place that knows the grid */
template <class Op0, class Op1 = Op0, unsigned int COLS = 1>
inline void blockScan(const ScanColumns &s, unsigned int n, unsigned int *hostTotal, unsigned int *zero)
{
    hipLaunchKernelGGL((pfac_block_scan<Op0, Op1, COLS>), dim3((n + kScanBlock - 1) / kScanBlock), dim3(1024), 0, 0, s, n, hostTotal, zero);
}

/* ------------------------------------------------------------------ offsets of items with 64-bit values (the gather's lines, the replacement's tokens, the expansion's pairs, the bounded members of a words call) */

/* the cut of `count` items for the two passes below: blocks of `threads` threads, eight per compute unit at most; per: the items of a block, a
 * multiple of `threads` (no items: no blocks) */
inline unsigned int offsetBlocks(const PFAC_context *c, size_t count, unsigned int threads, size_t &per)
{
    size_t blocks = (count + threads - 1) / threads;
    if (blocks > gridCap(c, 8)) blocks = gridCap(c, 8);
    per = blocks ? ((count + blocks - 1) / blocks + threads - 1) / threads * threads : threads;
    return (unsigned int)((count + per - 1) / per);
}

/* the first pass, by a block of BLOCK threads: blockBase[blockIdx.x] = the sum of value(k) over the block's items */
template <unsigned int BLOCK, class Value>
__device__ __forceinline__ void offsetsBlockTotal(size_t count, size_t per, unsigned long long *blockBase, Value value)
{
    __shared__ unsigned long long waveSum[BLOCK / 64];
    const size_t first = (size_t)blockIdx.x * per;
    const size_t end = count - first < per ? count : first + per;
    unsigned long long own = 0;
    for (size_t k = first + threadIdx.x; k < end; k += BLOCK) own += value(k);
    unsigned long long total = 0;
    (void)blockExclusive<BLOCK>(own, waveSum, total);
    if (threadIdx.x == 0) blockBase[blockIdx.x] = total;
}

/* the second, behind the scan of blockBase: store(k, the sum of the values in front of item k).  A thread calls store(k, ...) right behind its
 * value(k): a value may leave what it loaded to its store */
template <unsigned int BLOCK, class Value, class Store>
__device__ __forceinline__ void offsetsOfBlock(size_t count, size_t per, const unsigned long long *blockBase, Value value, Store store)
{
    __shared__ unsigned long long waveSum[BLOCK / 64];
    const size_t first = (size_t)blockIdx.x * per;
    const size_t end = count - first < per ? count : first + per;
    unsigned long long base = blockBase[blockIdx.x];
    for (size_t k0 = first; k0 < end; k0 += BLOCK) {                   /* the same trip count for every thread of the block */
        const size_t k = k0 + threadIdx.x;
        const bool has = k < end;
        const unsigned long long v = has ? value(k) : 0ull;
        unsigned long long stepTotal = 0;
        const unsigned long long before = base + blockExclusive<BLOCK>(v, waveSum, stepTotal);
        base += stepTotal;
        if (has) store(k, before);
    }
}

/* ------------------------------------------------------------------ the segment-window frame (scan_rules.hip, scan_segcount.hip) */

/* a caller's first pair inside [0, count] (scan_groups.hip too) */
__device__ __forceinline__ unsigned int clampFirstPair(int f, unsigned int count) { return f < 0 ? 0u : ((unsigned int)f < count ? (unsigned int)f : count); }

/* What the arguments of a segment-window pass start with.  A pass turns the ordered longest pairs of each segment into a list of entries per
 * segment, ascending within the segment, in CSR form: the count pass (EMIT == false) writes each segment's number of entries to segFirst[k],
 * pfac_array_scan turns them into first entries, the emit pass writes the entries below `capacity` */
struct SegmentFrame {
    unsigned int count;                 /* the pairs */
    const int *segFirstPairs;           /* [numSegments + 1], clamped where read; null: one segment of all pairs */
    unsigned int numSegments;
    unsigned long long *segFirst;       /* [numSegments + 1] */
    unsigned long long capacity;
};
constexpr unsigned int kNoWindow = 0xFFFFFFFFu;

/* The frame of both passes, by a block of BLOCK threads that takes whole segments, k = blockIdx.x, + gridDim.x, ...  What an entry is keyed by
 * (a rule, a pattern id) is cut into WINDOWS of 2^LOG2 keys; `table` is the unit's LDS table of one window, a word per SLOT, all zero between
 * windows.  For a window the block walks the segment's pairs, one per thread and trip: pair(i, w0, touch, beyond) works pair i into the table of
 * the window that starts at key w0, calls touch(r) where it saw slot r go from zero (the touched list: TOUCHED 16-bit slots; a list that overflows
 * only counts on, and the sweep then covers the whole table) and beyond(w) for a key of a later window w (nextWindow, an LDS atomic minimum: the
 * block goes on with the next window any pair of the segment has a key in, so a segment costs the windows it touches).  Then every touched slot
 * with decide(value, key) sets its bit in a bitmap of the window; the bitmap's words are swept in order, one per thread -- popcounts under a block
 * prefix give the number of entries and, with EMIT, the write position: emit(o, k, key, value) for the entries below capacity, ascending without
 * a sort.  segment(k) runs once per segment, in front of its windows.
 * RESET_IN_SWEEP says where a slot returns to zero.  false: where it is decided -- the sweep is then for the entries alone: skipped for a window
 * in which nothing was decided for (anyMarked), ended at capacity, and emit's value is 0.  true: under its bit in the sweep, behind its emit --
 * every touched window is swept to its end in both passes.
 * Whatever path a segment takes -- touched list, overflow sweep, truncation, no pair at all -- the table, the bitmap, the touched count and
 * nextWindow are as the prologue left them when the segment ends.  EMIT: a segment with no entry below capacity is left at once.
 * verify (NoVerify: none, and nothing of it is compiled) is a hook between the decisions and the sweep: verify(bits, w0, first, last) is called by
 * the whole block, behind a barrier, for a window whose bitmap `bits` is complete -- bit r: key w0 + r was decided for -- over the segment's pairs
 * [first, last); it may clear bits, in both passes alike, and returns behind a barrier of its own.  A cleared bit is an entry that never was */
struct NoVerify {};
template <bool EMIT, unsigned int LOG2, unsigned int TOUCHED, unsigned int BLOCK, bool RESET_IN_SWEEP, class Segment, class Pair, class Decide, class Emit,
          class Verify = NoVerify>
__device__ __forceinline__ void segmentWindows(const SegmentFrame &f, unsigned int *table, Segment segment, Pair pair, Decide decide, Emit emit,
                                               Verify verify = Verify())
{
    constexpr unsigned int WINDOW = 1u << LOG2;
    static_assert(WINDOW / 32 == BLOCK, "the sweep gives every thread one word of the bitmap");
    static_assert(WINDOW <= 65536, "the touched list holds 16-bit slots");
    __shared__ unsigned int bits[WINDOW / 32];
    __shared__ unsigned short touched[TOUCHED];
    __shared__ unsigned int waveSum[BLOCK / 64];
    __shared__ unsigned int words[RESET_IN_SWEEP ? 2 : 3];
    unsigned int &numTouched = words[0], &nextWindow = words[1];
    const unsigned int t = threadIdx.x;
    const auto resetWords = [&]() {
        numTouched = 0;
        nextWindow = kNoWindow;
        if constexpr (!RESET_IN_SWEEP) words[2] = 0;                                /* anyMarked */
    };
    for (unsigned int i = t; i < WINDOW; i += BLOCK) table[i] = 0;
    bits[t] = 0;
    if (t == 0) resetWords();
    __syncthreads();

    const auto touch = [&](unsigned int r) {
        const unsigned int slot = atomicAdd(&numTouched, 1u);
        if (slot < TOUCHED) touched[slot] = (unsigned short)r;
    };
    const auto beyond = [&](unsigned int w) { atomicMin(&nextWindow, w); };
    for (unsigned int k = blockIdx.x; k < f.numSegments; k += gridDim.x) {          /* (numSegments < 2^31: k + gridDim.x does not wrap) */
        unsigned long long base = 0;
        if constexpr (EMIT) {
            base = f.segFirst[k];
            if (f.segFirst[k + 1] == base || base >= f.capacity) continue;          /* no entry here, or none of them fits: the whole block leaves */
        }
        unsigned int first = 0, last = f.count;
        if (f.segFirstPairs != nullptr) {
            first = clampFirstPair(f.segFirstPairs[k], f.count);
            last = clampFirstPair(f.segFirstPairs[k + 1], f.count);
            if (last < first) last = first;                                         /* hostile offsets: an empty segment */
        }
        segment(k);
        unsigned int entries = 0;                                                   /* of this segment so far: the same in every thread */
        unsigned int window = first < last ? 0u : kNoWindow;
        while (window != kNoWindow) {
            const unsigned int w0 = window << LOG2;
            for (unsigned int i = first + t; i < last; i += BLOCK) pair(i, w0, touch, beyond);
            __syncthreads();
            const unsigned int n = numTouched, next = nextWindow;
            if (n != 0) {                                                           /* the same in every thread */
                const auto mark = [&](unsigned int r, unsigned int value) {         /* a slot that is not zero */
                    if (decide(value, w0 + r)) {
                        atomicOr(&bits[r >> 5], 1u << (r & 31u));
                        if constexpr (!RESET_IN_SWEEP) words[2] = 1u;
                    }
                    if constexpr (!RESET_IN_SWEEP) table[r] = 0;
                };
                if (n <= TOUCHED) {
                    for (unsigned int j = t; j < n; j += BLOCK) {
                        const unsigned int r = touched[j];
                        mark(r, table[r]);
                    }
                } else {                                                            /* more slots than the list holds: every slot of the table */
                    for (unsigned int r = t; r < WINDOW; r += BLOCK) {
                        const unsigned int value = table[r];
                        if (value != 0) mark(r, value);
                    }
                }
                __syncthreads();
                bool sweep = true;
                if constexpr (!RESET_IN_SWEEP) sweep = words[2] != 0;               /* the same in every thread: read behind the barrier, reset behind the next */
                if (sweep) {
                    if constexpr (!std::is_same<Verify, NoVerify>::value) verify(bits, w0, first, last);
                    unsigned int word = bits[t];
                    bits[t] = 0;
                    unsigned int total = 0;
                    const unsigned int before = blockExclusive<BLOCK>((unsigned int)__popc(word), waveSum, total);
                    unsigned long long o = base + entries + before;
                    while (word != 0 && (RESET_IN_SWEEP || (EMIT && o < f.capacity))) {
                        const unsigned int r = t * 32u + (unsigned int)__ffs((int)word) - 1u;
                        word &= word - 1u;
                        if constexpr (EMIT) {
                            if (o < f.capacity) emit(o, k, w0 + r, RESET_IN_SWEEP ? table[r] : 0u);
                            o++;
                        }
                        if constexpr (RESET_IN_SWEEP) table[r] = 0;
                    }
                    entries += total;
                }
            }
            __syncthreads();                                                        /* everyone has read the words */
            if (t == 0) resetWords();
            __syncthreads();
            window = next;
        }
        if constexpr (!EMIT) {
            if (t == 0) f.segFirst[k] = entries;
        }
    }
}

/* The launches of such a call, behind its argument checks.  carveSegFirst: segFirst[numSegments + 1] and `extraBytes` behind it, one region of
 * `scratch`.  segmentWindowPasses (a: the filled arguments, Args::f their SegmentFrame; list: the call's hand-off): the count pass, the scan of
 * the counts -- the length of the list to segFirst[numSegments] and to the hand-off's first value --, the emit pass where the caller has room
 * for an entry, segFirst to d_segFirst where given.  The caller ends the call: list.finish, behind what else it hands over.  false: a copy failed */
inline PFAC_status_t carveSegFirst(pfac::DeviceBuffer<char> &scratch, SegmentFrame &f, size_t extraBytes)
{
    return carveScratch(scratch, [&](ScratchCarver &k) { f.segFirst = k.take<unsigned long long>((size_t)f.numSegments + 1, extraBytes); });
}
template <class Args>
inline bool segmentWindowPasses(const PFAC_context *c, const Args &a, void (*count)(Args), void (*emit)(Args), unsigned int block, const HostHandoff &list,
                                size_t *d_segFirst)
{
    static_assert(sizeof(size_t) == sizeof(unsigned long long), "the caller's segFirst is 64-bit");
    const SegmentFrame &f = a.f;
    const unsigned int grid = f.numSegments < gridCap(c, 4) ? f.numSegments : gridCap(c, 4);
    hipLaunchKernelGGL(count, dim3(grid), dim3(block), 0, 0, a);
    hipLaunchKernelGGL(pfac_array_scan<unsigned long long>, dim3(1), dim3(1024), 0, 0, f.segFirst, f.numSegments, f.segFirst + f.numSegments,
                       reinterpret_cast<unsigned long long *>(list.d_value));
    if (f.capacity) hipLaunchKernelGGL(emit, dim3(grid), dim3(block), 0, 0, a);
    return d_segFirst == nullptr ||
           hipMemcpyAsync(d_segFirst, f.segFirst, ((size_t)f.numSegments + 1) * sizeof(unsigned long long), hipMemcpyDeviceToDevice, nullptr) == hipSuccess;
}

/* ------------------------------------------------------------------ the prefix chain of a pattern; the expansion frame (scan_all.hip, scan_words.hip, scan_groups.hip, scan_case.hip, scan_sig.hip, scan_approx.hip) */

/* pfac_host.h's forEachChainMember on the device: visit(q) for the patterns that occur where pattern id is the longest -- id, then along
 * prefixPattern through `table` ([numIds + 1] {prefixPattern, chainLen} by id; null: every chain is the pair itself): at most
 * max(1, chainLen[id]) of them, none for an id outside [1, numIds]; ends at such an id, or where visit returns false.  The one place where an id
 * is checked before it indexes the table and where a walk is bounded whatever the table says: the chain walks of scan_words.hip, scan_groups.hip, scan_case.hip, scan_sig.hip, scan_approx.hip,
 * scan_count.hip and scan_segcount.hip are calls of this (scan_rules.hip keeps its two loops, profiles/expand_refactor_resources.txt says why;
 * scan_all.hip writes a fixed number of slots per pair) */
template <class Visit>
__device__ __forceinline__ void forEachChainMember(const pfac::Int2 *table, unsigned int numIds, int id, Visit visit)
{
    if ((unsigned int)id - 1u >= numIds) return;
    int steps = table != nullptr ? table[id].y : 1;
    if (steps < 1) steps = 1;                                   /* an id the trie does not hold stands for itself alone */
    int q = id;
    for (int s = 0; s < steps && (unsigned int)q - 1u < numIds; s++) {
        if (!visit(q)) return;
        q = table != nullptr ? table[q].x : 0;
    }
}

/* What the arguments of an expansion start with.  An expansion turns an ordered list of longest pairs into the list of the members of their
 * prefix chains that a unit keeps, pair by pair, each chain longest first: the count pass leaves every block's number of entries in blockBase,
 * pfac_array_scan turns them into first entries, the write pass stores (id, position) into the slots below `capacity` */
struct ExpandFrame {
    const int *pairIds;                 /* the ordered longest pairs */
    const int *pairPos;
    size_t count;
    const pfac::Int2 *table;            /* [numIds + 1] {prefixPattern, chainLen} by id, or null: every chain is the pair itself */
    unsigned int numIds;
    unsigned int all;                   /* every member that is kept, else the longest one */
    size_t per;                         /* pairs per block: a multiple of the block size (offsetBlocks) */
    unsigned long long *blockBase;      /* [blocks + 1]: block totals -> their exclusive prefix; [blocks] = the length of the list */
    int *ids;                           /* the caller's arrays: capacity entries each */
    int *pos;
    size_t capacity;
};

/* Both passes, by blocks of BLOCK threads, a thread per pair and trip.  value(k): the number of entries of pair k.  members(k, emit): the same
 * entries again, emit(q) for each in order; the frame gives them the slots behind the entries in front of pair k, checks every slot against the
 * capacity and stores (q, the pair's position) -- the one pair store of an expansion; emit(q, at) stores (q, at) instead: a unit whose entries
 * lie elsewhere than their pair (scan_sig.hip: the start of a signature in front of its anchor; scan_approx.hip also reads emit.o and emit.f.capacity
 * to put a third value into the same slot).  hook(k, before), where given, runs for every
 * pair in front of its store, whatever the capacity.  A thread runs hook and members right behind its value(k), which may leave them what it loaded */
struct NoExpandHook { __device__ __forceinline__ void operator()(size_t, unsigned long long) const {} };
struct ExpandEmit {
    const ExpandFrame &f;
    unsigned long long &o;              /* the next slot of the thread's pair */
    const int &p;                       /* the pair's position */
    __device__ __forceinline__ void operator()(int q, int at) const
    {
        if (o < f.capacity) {
            f.ids[o] = q;
            f.pos[o] = at;
        }
        o++;
    }
    __device__ __forceinline__ void operator()(int q) const { (*this)(q, p); }
};
template <unsigned int BLOCK, class Value>
__device__ __forceinline__ void expandCount(const ExpandFrame &f, Value value) { offsetsBlockTotal<BLOCK>(f.count, f.per, f.blockBase, value); }
template <unsigned int BLOCK, class Value, class Members, class Hook = NoExpandHook>
__device__ __forceinline__ void expandWrite(const ExpandFrame &f, Value value, Members members, Hook hook = Hook())
{
    /* the pair's position: loaded with its value, in front of the block prefix, whatever the capacity (a unit's argument checks refuse pairs without positions) */
    int p = 0;
    const auto valued = [&](size_t k) -> unsigned long long { p = f.pairPos[k]; return value(k); };
    offsetsOfBlock<BLOCK>(f.count, f.per, f.blockBase, valued, [&](size_t k, unsigned long long before) {
        hook(k, before);
        if (before >= f.capacity) return;
        unsigned long long o = before;
        members(k, ExpandEmit{f, o, p});
    });
}

/* The launches of an expansion, behind the unit's argument checks (a: the filled arguments, Args::f their ExpandFrame): the cut of the pairs
 * into blocks of `block` threads, blockBase[blocks + 1] and what carve(ScratchCarver &) takes behind it out of `scratch` (halfMore: carveScratch),
 * front() -- the unit's own launches in front of the passes; false: one failed --, the hand-off through `slot`, the count pass, the scan of the
 * block totals, the write pass where wantWrite, behind(the device address of the total) -- the unit's own launches behind them --, the end of the
 * call; *h_total = the length of the whole list.  A list of no pairs has no blocks: only the scan runs, over nothing */
struct ExpandNothing {
    void operator()(ScratchCarver &) const {}
    bool operator()() const { return true; }
    void operator()(const unsigned long long *) const {}
};
template <class Args, class Carve = ExpandNothing, class Front = ExpandNothing, class Behind = ExpandNothing>
inline PFAC_status_t expandPasses(PFAC_context *c, pfac::DeviceBuffer<char> &scratch, pfac::HostSlot slot, Args &a, void (*count)(Args), void (*write)(Args),
                                  unsigned int block, bool wantWrite, size_t *h_total, Carve carve = Carve(), bool halfMore = false, Front front = Front(),
                                  Behind behind = Behind())
{
    ExpandFrame &f = a.f;
    const unsigned int blocks = offsetBlocks(c, f.count, block, f.per);
    const PFAC_status_t carved = carveScratch(scratch, [&](ScratchCarver &k) {
        f.blockBase = k.take<unsigned long long>((size_t)blocks + 1);
        carve(k);
    }, nullptr, halfMore);
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    if (!front()) return PFAC_STATUS_INTERNAL_ERROR;
    const HostHandoff list(c, slot);
    if (blocks) hipLaunchKernelGGL(count, dim3(blocks), dim3(block), 0, 0, a);
    hipLaunchKernelGGL(pfac_array_scan<unsigned long long>, dim3(1), dim3(1024), 0, 0, f.blockBase, blocks, f.blockBase + blocks,
                       reinterpret_cast<unsigned long long *>(list.d_value));
    if (blocks && wantWrite) hipLaunchKernelGGL(write, dim3(blocks), dim3(block), 0, 0, a);
    behind(f.blockBase + blocks);
    unsigned long long total = 0;
    if (!list.finish(&total, f.blockBase + blocks)) return PFAC_STATUS_INTERNAL_ERROR;
    *h_total = (size_t)total;
    return PFAC_STATUS_SUCCESS;
}

/* ------------------------------------------------------------------ the pairs of an ordered scan (scan_spans.hip, scan_disjoint.hip) */

/* what the arguments of both select calls start with */
struct PairArgs {
    const int *ids, *pos;               /* the scan's ordered pairs (the caller's arrays) */
    unsigned int count, n;
    const int *patternLen;              /* by id, numIds entries */
    unsigned int numIds;
};

/* position and end of pair i, both inside [0, n] whatever the pair says */
__device__ __forceinline__ void pairOf(const PairArgs &a, unsigned int i, unsigned int &p, unsigned int &e)
{
    const int id = a.ids[i];
    clampSpan(a.pos[i], (unsigned int)id < a.numIds ? a.patternLen[id] : 0, a.n, p, e);
}

/* the last launch of a select call: min(*total, bound) | *covered << 32, both counts as one 64-bit value, to *value and to the host (a template
 * like the scan kernels: only a unit that launches it has a copy) */
template <class T>
__global__ void pfac_pairs_finish(const T *total, T bound, const T *covered, unsigned long long *value, unsigned long long *hostValue)
{
    const T all = *total, kept = all < bound ? all : bound;
    const unsigned long long v = (unsigned long long)kept | (unsigned long long)*covered << 32;
    *value = v;
    storeToHost(hostValue, v);
}

/* The head of a select call: the compacted scan WITH its ordering launches into the caller's arrays (ids in d_ids, positions in d_pos, ascending),
 * both outputs zeroed, the common arguments filled in.  a.count == 0 behind a success: nothing found, the call is over */
inline PFAC_status_t pairsSelectHead(PFAC_handle_t handle, char *d_scan, size_t size, int hashed, const int *d_patternLen, size_t numIds, int *d_ids,
                                     int *d_pos, size_t *h_count, size_t *h_covered, PairArgs &a)
{
    size_t count = 0;
    const PFAC_status_t st = compactedScan(handle, d_scan, size, hashed, d_ids, d_pos, true, &count);
    if (st != PFAC_STATUS_SUCCESS) return st;
    *h_count = 0;
    *h_covered = 0;
    a.ids = d_ids;
    a.pos = d_pos;
    a.count = (unsigned int)count;
    a.n = (unsigned int)size;
    a.patternLen = d_patternLen;
    a.numIds = (unsigned int)(numIds < (size_t)0x7fffffff ? numIds : (size_t)0x7fffffff);
    return PFAC_STATUS_SUCCESS;
}

/* The tail, behind the call's own launches: pfac_pairs_finish over *d_total and the word `covered` that lies behind *d_value, the hand-off through
 * `slot`, and (count, covered) unpacked: 1 <= count <= bound (the entries the call had room for) and count <= covered <= size, or the call failed */
template <class T>
inline PFAC_status_t pairsSelectTail(PFAC_context *c, pfac::HostSlot slot, const T *d_total, size_t bound, size_t size, unsigned long long *d_value,
                                     size_t *h_count, size_t *h_covered)
{
    const HostHandoff counts(c, slot);
    hipLaunchKernelGGL(pfac_pairs_finish<T>, dim3(1), dim3(1), 0, 0, d_total, (T)bound, reinterpret_cast<const T *>(d_value + 1), d_value,
                       reinterpret_cast<unsigned long long *>(counts.d_value));
    unsigned long long v = 0;
    if (!counts.finish(&v, d_value)) return PFAC_STATUS_INTERNAL_ERROR;
    const size_t count = (size_t)(v & 0xFFFFFFFFull), covered = (size_t)(v >> 32);
    if (count == 0 || count > bound || covered < count || covered > size) return PFAC_STATUS_INTERNAL_ERROR;
    *h_count = count;
    *h_covered = covered;
    return PFAC_STATUS_SUCCESS;
}

/* ------------------------------------------------------------------ the seam of a stream (scan_stream.hip, scan_flows.hip) */

/* one piece of one stream, as its seam sees it */
struct SeamPiece {
    const unsigned char *carry;                /* `carried` bytes */
    const unsigned char *piece;                /* `size` bytes (not read when size == 0) */
    unsigned char *carryNext;                  /* nextCarried bytes are written: the last min(M - 1, carried + size) bytes of [carry | piece] */
    uint32_t carried, staged;                  /* staged = carried + min(size, M - 1) */
    uint32_t numFinal;                         /* start positions [0, numFinal) of the staged bytes are walked, numFinal <= carried */
    uint32_t nextCarried;
    uint32_t fold;                             /* a caseless set: the piece's bytes are folded where they are staged or carried on */
    size_t size;
};

/* byte j of [carry | piece] (I: uint32_t where the caller knows that carried + size fits, else size_t) */
template <class I>
__device__ __forceinline__ unsigned char seamByte(const SeamPiece &s, I j) { return j < s.carried ? s.carry[j] : foldByte(s.piece[j - s.carried], s.fold); }

/* [carry | head of the piece] into `stage`, by `threads` threads of which this is thread tid */
__device__ __forceinline__ void seamStage(const SeamPiece &s, unsigned char *stage, uint32_t tid, uint32_t threads)
{
    for (uint32_t i = tid; i < s.staged; i += threads) stage[i] = seamByte(s, i);
}

/* ... and the stream's next carry into its other buffer */
__device__ __forceinline__ void seamCarryOn(const SeamPiece &s, uint32_t tid, uint32_t threads)
{
    const size_t first = (size_t)s.carried + s.size - s.nextCarried;
    for (uint32_t i = tid; i < s.nextCarried; i += threads) s.carryNext[i] = seamByte(s, first + i);
}

/* a hit at staged position p: positions count from the piece's first byte (negative) */
__device__ __forceinline__ void seamEmit(const SeamPiece &s, int *ids, int *pos, uint32_t at, int id, uint32_t p)
{
    ids[at] = id;
    pos[at] = (int)p - (int)s.carried;
}

/* The seam by one block of BLOCK threads (0: blockDim.x; whole waves): stages the bytes, writes the next carry, walks the carried start positions
 * that the piece makes final through the chained table, one position per thread and trip, every read checked against the end of the staged bytes
 * (boundedWalk), and writes the (id, position) pairs in position order from ids[0] / pos[0] on -- wave ballot, the waves' counts added up through
 * waveCount (LDS, a word per wave).  Returns the number of pairs, the same in every thread */
template <uint32_t BLOCK>
__device__ __forceinline__ uint32_t seamBlock(const ScanArgs &a, const SeamPiece &s, unsigned char *stage, int *ids, int *pos, uint32_t *waveCount)
{
    const uint32_t threads = BLOCK ? BLOCK : blockDim.x, waves = threads >> 6;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    seamStage(s, stage, tid, threads);
    seamCarryOn(s, tid, threads);
    __threadfence_block();
    __syncthreads();

    const ChainCtx<false> ctx(a);
    uint32_t written = 0;
    for (uint32_t base = 0; base < s.numFinal; base += threads) {
        const uint32_t p = base + tid;
        const int m = p < s.numFinal ? boundedWalk<false>(ctx, stage, p, s.staged) : 0;
        const uint64_t hits = __ballot(m > 0);
        if (lane == 0) waveCount[wave] = (uint32_t)__popcll(hits);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < waves; w++) {
            const uint32_t cnt = waveCount[w];
            before += w < wave ? cnt : 0u;
            total += cnt;
        }
        if (m > 0) seamEmit(s, ids, pos, written + before + laneRankIn(hits), m, p);
        written += total;
        __syncthreads();                       /* waveCount is rewritten by the next trip */
    }
    return written;
}

} // namespace

#endif /* PFAC_SCAN_PASSES_H_ */
