/*
 * scan_passes.h -- what the passes around the scan share (scan_module.hip with scan_order.inc, scan_batch.hip, scan_all.hip, scan_fold.hip,
 * scan_stream.hip, scan_flows.hip, scan_lines.hip, scan_spans.hip; the product kernels' units do not include it): launch sizes, the hand-off of a call's
 * result to the host through mapped memory, the device fold byte, block prefix sums, the seam of a stream.  Like scan_common.h, everything is
 * in an unnamed namespace: inline device code, each unit its own copy.
 */
#ifndef PFAC_SCAN_PASSES_H_
#define PFAC_SCAN_PASSES_H_

#include "scan_common.h"

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
 * number issued to the call that waits on it, so the handle counts all its calls with one counter */
struct HostHandoff {
    unsigned int *d_value = nullptr, *d_done = nullptr;
    volatile unsigned int *h_value = nullptr, *h_done = nullptr;
    unsigned int seq = 0;

    HostHandoff() = default;
    HostHandoff(PFAC_context *c, pfac::HostSlot slot)
        : d_value(c->d_modeHint + slot.value), d_done(c->d_modeHint + slot.done), h_value(c->h_modeHint + slot.value), h_done(c->h_modeHint + slot.done)
    {
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
    unsigned long long value64() const { return __atomic_load_n(reinterpret_cast<const unsigned long long *>(const_cast<const unsigned int *>(h_value)), __ATOMIC_ACQUIRE); }
};

/* ------------------------------------------------------------------ the fold of a byte */

/* pfac::asciiFold on the device, for a caseless set (fold != 0) */
__device__ __forceinline__ unsigned char foldByte(unsigned char b, uint32_t fold) { return (unsigned char)(b + ((fold != 0 && (unsigned)(b - 'A') < 26u) ? 32 : 0)); }

/* ------------------------------------------------------------------ block prefix sums */

/* inclusive prefix sum over the 64 lanes: 32-bit values by DPP (waveInclusiveScan), 64-bit ones by shuffles */
template <class T>
__device__ __forceinline__ T waveInclusive(T v)
{
    if constexpr (sizeof(T) == 4) {
        return (T)waveInclusiveScan((uint32_t)v);
    } else {
        const unsigned int lane = threadIdx.x & 63u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const T up = __shfl_up(v, d);
            if ((int)lane >= d) v += up;
        }
        return v;
    }
}

/* exclusive prefix of `own` over the block's BLOCK threads, and the block's total (every thread calls it, every thread gets both);
 * waveSum: BLOCK / 64 entries of LDS, free again at the next call */
template <unsigned int BLOCK, class T>
__device__ __forceinline__ T blockExclusive(T own, T *waveSum, T &total)
{
    const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const T incl = waveInclusive(own);
    __syncthreads();                                    /* waveSum may still be read from the previous call */
    if (lane == 63) waveSum[wave] = incl;
    __syncthreads();
    T before = 0;
    total = 0;
#pragma unroll
    for (unsigned int w = 0; w < BLOCK / 64; w++) {
        const T s = waveSum[w];
        before += w < wave ? s : (T)0;
        total += s;
    }
    return before + incl - own;
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
        if (hostTotal != nullptr) {
            __hip_atomic_store(hostTotal, carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __threadfence_system();
        }
    }
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
