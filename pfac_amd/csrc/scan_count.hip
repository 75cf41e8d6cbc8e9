/*
 * scan_count.hip -- occurrence counts per pattern (include/pfac_ext.h: PFACX_count*): which patterns occurred, and how often.
 *
 * Every pattern that occurs at a position is a prefix of the longest one there, so A[id], the number of occurrences of pattern id, is the longest
 * histogram L summed over the patterns that have id on their prefix chain (Automaton::prefixPattern).  The counts never cost the expanded list:
 *
 *   (hipMemsetAsync)       L and the word of the total, 4 (F + 1) + 8 bytes, queued in front of the scan
 *   (the compacted scan)   PFACX_countFromDevice only: the pairs in ANY order (the four ordering launches are not paid for) into the handle's pair scratch
 *   pfac_count_hist        L[id] += 1 for every pair, ids outside [1, F] ignored.  A block of 256 threads takes 1024 ids a trip, four consecutive ids per
 *                          lane: one 16-byte load where the lane's four lie inside the list, else four loads with bounds (the list starts at any
 *                          4-byte alignment: the quads are cut on the ADDRESS).  Runs of equal ids -- inside a lane's four and across the lanes of the
 *                          wave -- are collapsed before any atomic: the head of a run adds its length (256 Mi pairs of one id: one LDS atomic per wave
 *                          and trip).  The adds go to a histogram of the block in LDS: direct-indexed 32-bit counters while F + 1 <= kCountDirect,
 *                          else a tagged cache of kCountCacheSlots {id, count} slots -- a slot is claimed by the first id that hashes to it; an id that
 *                          finds its slot taken by another goes straight to L with a global atomic (300 000 ids spread thin: about what one atomic
 *                          per pair costs, and no worse).  A block flushes its non-zero counters, one global atomic each, and adds what it counted
 *                          (chainLen[id] or 1 per pair) to the total with one 64-bit atomic
 *   pfac_count_store       one thread per id: counts[id] = L[id], counts[0] = 0; PFACX_COUNT_ACCUMULATE: counts[id] += L[id], 64-bit, no atomic (one
 *                          thread per entry), entry 0 left alone.  Thread 0 hands the total to the host
 *   pfac_count_chain       all-occurrence form of a set with maxChain > 1: one thread per id with L[id] != 0 follows prefixPattern from id and adds L[id]
 *                          to every ancestor's counts[] (64-bit vector atomic).  It reads L, never counts: the launch boundary behind pfac_count_store is
 *                          all the ordering it needs.  At most F x maxChain steps whatever the input
 *   pfac_host_done         (PFACX_countFromDevice) the call's sequence number to mapped host memory (scan_passes.h: HostHandoff)
 * SCRATCH of these: 4 (F + 1) + 8 bytes, each part rounded up to 256 (DeviceScratch::count); the pair list is DeviceScratch::allPairs (8 bytes per input
 * byte, shared with PFACX_matchAll*), the table DeviceScratch::allTable (8 (F + 1) bytes, shared too).
 *
 * The non-zero counts (PFACX_countNonzeroFromDevice) are the usual flag / scan / emit compaction, a block per kNzBlock entries:
 *   pfac_count_flags       the non-zero entries of each block and the 64-bit sum of its entries
 *   pfac_block_scan<sum>   the first list entry of each block, the number of entries (scan_passes.h)
 *   pfac_count_emit        (i, counts[i]) in ascending order, nothing at or beyond capacity
 *   pfac_count_finish      one block adds up the block sums; the distinct count and the total to mapped host memory
 * SCRATCH with B = (numCounts + 255) / 256: 4 B + 4 (B + 1) + 8 B + 16 bytes, each part rounded up to 256.
 * Plain C++, vector stores and vector atomics only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_count.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"

namespace {

constexpr unsigned int kCountThreads = 256;
constexpr unsigned int kCountPer = 4;                                   /* consecutive ids per lane: one 16-byte load */
constexpr unsigned int kCountTrip = kCountThreads * kCountPer;          /* ids a block takes per trip */
constexpr unsigned int kCountLdsWords = 16384;                          /* 64 KiB of the CU's 160: two blocks per CU */
constexpr unsigned int kCountDirect = kCountLdsWords;                   /* F + 1 <= this: a counter per id (pfac_amd/api.py: PFACX_COUNT_LDS_DIRECT) */
constexpr unsigned int kCountCacheLog2 = 13;
constexpr unsigned int kCountCacheSlots = 1u << kCountCacheLog2;        /* else: tags in the first half of the words, counts in the second */
static_assert(2 * kCountCacheSlots == kCountLdsWords, "the cache fills the words of the direct histogram");
constexpr unsigned int kNzBlock = 256;                                  /* entries per block of the non-zero compaction: one per thread */

struct HistArgs {
    const int *ids;                     /* the pairs' ids: `count` entries from any 4-byte aligned address */
    unsigned int count;
    unsigned int numIds;                /* F: ids outside [1, F] are ignored */
    const pfac::Int2 *table;            /* [F + 1] {prefixPattern, chainLen} by id, or null: every pair adds 1 to the total */
    unsigned int *hist;                 /* L[F + 1] */
    unsigned long long *total;          /* or null */
};

/* the four ids of quad q of the list as the ADDRESS cuts it (`shift` ints lie between the aligned 16 bytes that hold ids[0] and ids[0]); 0: no id */
__device__ __forceinline__ void loadQuad(const HistArgs &a, const int *aligned, unsigned int shift, size_t q, unsigned int v[kCountPer])
{
    const size_t j = q * kCountPer, end = (size_t)shift + a.count;
    if (j >= shift && j + kCountPer <= end) {
        const pfacmod::u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const pfacmod::u32x4 *>(aligned + j));
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
#pragma unroll
        for (unsigned int k = 0; k < kCountPer; k++) v[k] = j + k >= shift && j + k < end ? (unsigned int)aligned[j + k] : 0u;
    }
#pragma unroll
    for (unsigned int k = 0; k < kCountPer; k++) v[k] = v[k] - 1u < a.numIds ? v[k] : 0u;
}

template <bool DIRECT>
__global__ __launch_bounds__(kCountThreads) void pfac_count_hist(HistArgs a)
{
    __shared__ unsigned int lds[kCountLdsWords];
    __shared__ unsigned long long waveSum[kCountThreads / 64];
    const unsigned int t = threadIdx.x, lane = t & 63u;
    const unsigned int used = DIRECT ? a.numIds + 1u : kCountLdsWords;
    for (unsigned int i = t; i < used; i += kCountThreads) lds[i] = 0;
    __syncthreads();

    const unsigned int shift = (unsigned int)((reinterpret_cast<uintptr_t>(a.ids) & 15u) >> 2);
    const int *aligned = a.ids - shift;
    const size_t quads = ((size_t)shift + a.count + kCountPer - 1) / kCountPer;
    unsigned long long own = 0;
    /* the same trips for every thread of a block: the ballots and shuffles below are the whole wave's */
    for (size_t q0 = (size_t)blockIdx.x * kCountThreads; q0 < quads; q0 += (size_t)gridDim.x * kCountThreads) {
        unsigned int v[kCountPer] = {0, 0, 0, 0};
        if (q0 + t < quads) loadQuad(a, aligned, shift, q0 + t, v);
        /* element e = 4 lane + k of the wave's 256 heads a run iff it differs from element e - 1 */
        const unsigned int prev = (unsigned int)__shfl_up((int)v[kCountPer - 1], 1);
        bool head[kCountPer];
        head[0] = lane == 0 || v[0] != prev;
        unsigned long long any = __ballot(head[0]);
#pragma unroll
        for (unsigned int k = 1; k < kCountPer; k++) {
            head[k] = v[k] != v[k - 1];
            any |= __ballot(head[k]);
        }
        /* the first head behind this lane's four: the first lane above with a head, and that lane's first */
        const unsigned long long above = lane == 63u ? 0ull : any & (~0ull << (lane + 1u));
        const unsigned int nextLane = above ? (unsigned int)__ffsll((long long)above) - 1u : 0u;
        const unsigned int first = head[0] ? 0u : head[1] ? 1u : head[2] ? 2u : 3u;       /* (a lane without a head is never asked) */
        const unsigned int firstThere = (unsigned int)__shfl((int)first, (int)nextLane);
        unsigned int next = above ? nextLane * kCountPer + firstThere : 64u * kCountPer;
#pragma unroll
        for (int k = kCountPer - 1; k >= 0; k--) {
            if (!head[k]) continue;
            const unsigned int e = lane * kCountPer + (unsigned int)k, run = next - e, id = v[k];
            next = e;
            if (id == 0) continue;
            if (a.total != nullptr) {
                const int c = a.table != nullptr ? a.table[id].y : 1;
                own += (unsigned long long)run * (unsigned int)(c > 0 ? c : 1);
            }
            if constexpr (DIRECT) {
                atomicAdd(&lds[id], run);
            } else {
                const unsigned int slot = (id * 0x9E3779B1u) >> (32 - kCountCacheLog2);
                const unsigned int owner = atomicCAS(&lds[slot], 0u, id);
                if (owner == 0u || owner == id) atomicAdd(&lds[kCountCacheSlots + slot], run);
                else atomicAdd(&a.hist[id], run);
            }
        }
    }
    __syncthreads();
    if constexpr (DIRECT) {
        for (unsigned int i = t; i < used; i += kCountThreads) {
            const unsigned int c = lds[i];
            if (c != 0) atomicAdd(&a.hist[i], c);
        }
    } else {
        for (unsigned int s = t; s < kCountCacheSlots; s += kCountThreads) {
            const unsigned int id = lds[s], c = lds[kCountCacheSlots + s];
            if (c != 0 && id - 1u < a.numIds) atomicAdd(&a.hist[id], c);
        }
    }
    if (a.total != nullptr) {
        unsigned long long sum = 0;
        (void)blockExclusive<kCountThreads>(own, waveSum, sum);
        if (t == 0 && sum != 0) atomicAdd(a.total, sum);
    }
}

struct StoreArgs {
    const unsigned int *hist;           /* L[F + 1] */
    unsigned int numIds;
    unsigned int accumulate;
    const pfac::Int2 *table;            /* pfac_count_chain */
    unsigned long long *counts;         /* the caller's: entries [0, F] */
    const unsigned long long *total;    /* or null */
};

__global__ __launch_bounds__(kCountThreads) void pfac_count_store(StoreArgs a, unsigned long long *hostTotal)
{
    const unsigned int stride = gridDim.x * kCountThreads;
    for (unsigned int id = blockIdx.x * kCountThreads + threadIdx.x; id <= a.numIds; id += stride) {
        if (a.accumulate) {
            if (id != 0 && a.hist[id] != 0) a.counts[id] += a.hist[id];
        } else {
            a.counts[id] = id != 0 ? a.hist[id] : 0u;
        }
    }
    if (a.total != nullptr && blockIdx.x == 0 && threadIdx.x == 0) storeToHost(hostTotal, *a.total);
}

__global__ __launch_bounds__(kCountThreads) void pfac_count_chain(StoreArgs a)
{
    const unsigned int stride = gridDim.x * kCountThreads;
    for (unsigned int id = blockIdx.x * kCountThreads + threadIdx.x + 1u; id <= a.numIds; id += stride) {
        const unsigned long long own = a.hist[id];
        if (own == 0) continue;
        bool head = true;                                           /* id itself has its count from pfac_count_store: the members behind it */
        forEachChainMember(a.table, a.numIds, (int)id, [&](int q) {
            if (!head) atomicAdd(&a.counts[q], own);
            head = false;
            return true;
        });
    }
}

/* ------------------------------------------------------------------ the non-zero counts */

struct NonzeroArgs {
    const unsigned long long *counts;
    unsigned int n;
    unsigned int blocks;
    unsigned int *blockCount, *blockBase;       /* [blocks] non-zero entries of the block; [blocks + 1] in front of the block, [blocks] = of all */
    unsigned long long *blockSum;               /* [blocks] */
    unsigned long long *value;                  /* [2]: the distinct count, the sum */
    int *ids;
    unsigned long long *outCounts;
    size_t capacity;
};

__global__ __launch_bounds__(kNzBlock) void pfac_count_flags(NonzeroArgs a)
{
    __shared__ unsigned long long waveSum[kNzBlock / 64];
    __shared__ unsigned int waveCount[kNzBlock / 64];
    const unsigned int i = blockIdx.x * kNzBlock + threadIdx.x;
    const unsigned long long c = i < a.n ? a.counts[i] : 0ull;
    unsigned long long sum = 0;
    unsigned int nonzero = 0;
    (void)blockExclusive<kNzBlock>(c, waveSum, sum);
    (void)blockExclusive<kNzBlock>(c != 0 ? 1u : 0u, waveCount, nonzero);
    if (threadIdx.x == 0) {
        a.blockSum[blockIdx.x] = sum;
        a.blockCount[blockIdx.x] = nonzero;
    }
}

__global__ __launch_bounds__(kNzBlock) void pfac_count_emit(NonzeroArgs a)
{
    __shared__ unsigned int waveCount[kNzBlock / 64];
    const unsigned int i = blockIdx.x * kNzBlock + threadIdx.x;
    const unsigned long long c = i < a.n ? a.counts[i] : 0ull;
    unsigned int nonzero = 0;
    const size_t o = (size_t)a.blockBase[blockIdx.x] + blockExclusive<kNzBlock>(c != 0 ? 1u : 0u, waveCount, nonzero);
    if (c != 0 && o < a.capacity) {
        a.ids[o] = (int)i;
        a.outCounts[o] = c;
    }
}

__global__ __launch_bounds__(1024) void pfac_count_finish(NonzeroArgs a, unsigned long long *hostValue)
{
    __shared__ unsigned long long waveSum[16];
    unsigned long long own = 0, sum = 0;
    for (unsigned int b = threadIdx.x; b < a.blocks; b += 1024u) own += a.blockSum[b];
    (void)blockExclusive<1024>(own, waveSum, sum);
    if (threadIdx.x == 0) {
        const unsigned long long distinct = a.blockBase[a.blocks];
        a.value[0] = distinct;
        a.value[1] = sum;
        storeToHost(hostValue, distinct, sum);
    }
}

} // namespace

extern "C" {

PFAC_status_t PFACX_countPairs(PFAC_handle_t handle, char *d_scan, size_t size, int hashed, const int *d_ids, size_t numPairs, const void *d_table,
                               unsigned int flags, unsigned long long *d_counts, size_t *h_total)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!d_counts || (d_scan && (size == 0 || size > (size_t)0x7fffffff)) || (!d_scan && (numPairs > (size_t)0x7fffffff || (numPairs && !d_ids))))
        return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = handle;
    if (c->fa.numPatterns < 0) return PFAC_STATUS_INTERNAL_ERROR;
    const unsigned int F = (unsigned int)c->fa.numPatterns;
    const bool accumulate = (flags & PFACX_COUNT_ACCUMULATE) != 0;

    HistArgs h{};
    size_t bytes = 0;
    const PFAC_status_t carved = carveScratch(c->scratch.count, [&](ScratchCarver &k) {
        h.hist = k.take<unsigned int>((size_t)F + 1);
        h.total = k.take<unsigned long long>(1);
    }, &bytes);
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    if (hipMemsetAsync(h.hist, 0, bytes, 0) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;        /* L and the total: in front of the scan */

    size_t count = numPairs;
    if (d_scan) {
        /* the compacted scan, pairs in any order, into the pair scratch of the all-match calls: the ids, then as many positions */
        pfac::DeviceBuffer<int> &pairs = c->scratch.allPairs;
        const PFAC_status_t grown = pairs.reserve(2 * size);
        if (grown != PFAC_STATUS_SUCCESS) return grown;
        const PFAC_status_t st = compactedScan(handle, d_scan, size, hashed, pairs.get(), pairs.get() + pairs.count() / 2, false, &count);
        if (st != PFAC_STATUS_SUCCESS) return st;
        d_ids = pairs.get();
    }
    h.ids = d_ids;
    h.count = (unsigned int)count;
    h.numIds = F;
    h.table = static_cast<const pfac::Int2 *>(d_table);
    if (!h_total) h.total = nullptr;
    const HostHandoff total = h_total ? HostHandoff(c, pfac::kHostCount) : HostHandoff();

    if (count > 0) {
        const size_t trips = (count + 2 * kCountPer + kCountTrip - 1) / kCountTrip;             /* (+ the quad the alignment may add) */
        const unsigned int grid = (unsigned int)(trips < gridCap(c, 2) ? trips : gridCap(c, 2));
        if (F + 1 <= kCountDirect) hipLaunchKernelGGL(pfac_count_hist<true>, dim3(grid), dim3(kCountThreads), 0, 0, h);
        else hipLaunchKernelGGL(pfac_count_hist<false>, dim3(grid), dim3(kCountThreads), 0, 0, h);
    }
    StoreArgs s{};
    s.hist = h.hist;
    s.numIds = F;
    s.accumulate = accumulate ? 1u : 0u;
    s.table = h.table;
    s.counts = d_counts;
    s.total = h.total;
    if (count > 0 || !accumulate || h_total) {
        const unsigned int grid = count > 0 || !accumulate ? gridFor(c, (size_t)F + 1) : 1u;
        if (count == 0 && accumulate) s.numIds = 0;                                            /* nothing to add: the launch only hands the total over */
        hipLaunchKernelGGL(pfac_count_store, dim3(grid), dim3(kCountThreads), 0, 0, s, reinterpret_cast<unsigned long long *>(total.d_value));
        s.numIds = F;
    }
    if (count > 0 && s.table != nullptr) hipLaunchKernelGGL(pfac_count_chain, dim3(gridFor(c, F)), dim3(kCountThreads), 0, 0, s);
    if (!h_total) return hipGetLastError() == hipSuccess ? PFAC_STATUS_SUCCESS : PFAC_STATUS_INTERNAL_ERROR;
    unsigned long long added = 0;
    if (!total.finish(&added, h.total)) return PFAC_STATUS_INTERNAL_ERROR;
    *h_total = (size_t)added;
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_countNonzero(PFAC_handle_t handle, const unsigned long long *d_counts, size_t numCounts, int *d_ids,
                                 unsigned long long *d_outCounts, size_t capacity, size_t *h_numDistinct, unsigned long long *h_total)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!d_counts || !h_numDistinct || !h_total || numCounts == 0 || numCounts > (size_t)0x7fffffff || (capacity && (!d_ids || !d_outCounts)))
        return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = handle;
    NonzeroArgs a{};
    a.counts = d_counts;
    a.n = (unsigned int)numCounts;
    const size_t blocks = (numCounts + kNzBlock - 1) / kNzBlock;
    a.blocks = (unsigned int)blocks;
    a.ids = d_ids;
    a.outCounts = d_outCounts;
    a.capacity = capacity;
    const PFAC_status_t carved = carveScratch(c->scratch.count, [&](ScratchCarver &k) {
        a.blockCount = k.take<unsigned int>(blocks);
        a.blockBase = k.take<unsigned int>(blocks + 1);
        a.blockSum = k.take<unsigned long long>(blocks);
        a.value = k.take<unsigned long long>(2);
    });
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    const HostHandoff list(c, pfac::kHostNonzero);
    hipLaunchKernelGGL(pfac_count_flags, dim3(a.blocks), dim3(kNzBlock), 0, 0, a);
    blockScan<OpSum>({{a.blockCount}, {a.blockBase}}, a.blocks, nullptr, nullptr);
    if (capacity) hipLaunchKernelGGL(pfac_count_emit, dim3(a.blocks), dim3(kNzBlock), 0, 0, a);
    hipLaunchKernelGGL(pfac_count_finish, dim3(1), dim3(1024), 0, 0, a, reinterpret_cast<unsigned long long *>(list.d_value));
    unsigned long long v[2] = {0, 0};
    if (!list.finish(v, a.value, a.value + 1)) return PFAC_STATUS_INTERNAL_ERROR;
    if (v[0] > numCounts) return PFAC_STATUS_INTERNAL_ERROR;
    *h_numDistinct = (size_t)v[0];
    *h_total = v[1];
    return v[0] > capacity ? PFACX_STATUS_OUTPUT_TRUNCATED : PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
