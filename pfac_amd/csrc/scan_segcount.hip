/*
 * scan_segcount.hip -- per-segment occurrence counts in CSR form (include/pfac_ext.h: PFACX_countBatch*): how often each pattern occurs
 * in each segment of a batch.
 *
 * Pattern id occurs at a position of segment k iff it lies on the prefix chain (Automaton::prefixPattern) of the segment's LONGEST pair there, so
 * the count list follows from the ordered compacted batch scan (the pairs and the first pair of each segment, in handle scratch) and the
 * {prefixPattern, chainLen} table of the all-match calls.  Nothing here is sized by segments x patterns:
 *
 *   pfac_segcount_pass<false, ALL>  a block takes whole segments, k = blockIdx.x, + gridDim.x, ...  It keeps in LDS a direct-indexed table
 *                            counter[kSegWindow] of 32-bit counters, a bitmap of kSegWindow bits and a list of kSegTouched touched slots; ids
 *                            [w kSegWindow, (w + 1) kSegWindow) are WINDOW w.  For a window the block walks the segment's pairs, kSegBlockPairs a
 *                            trip, one per thread; a thread takes its pair's id or, with ALL, every id on its prefix chain (at most chainLen steps,
 *                            ended by the table's bounds whatever the table says).  An id in the window adds 1 to its counter with an LDS atomic;
 *                            whoever sees the counter go from 0 appends the slot to the touched list (a list that overflows only counts on: the
 *                            sweep below then covers the whole window).  An id BEHIND the window lowers nextWindow (LDS atomic minimum): the block
 *                            goes on with the next window any pair of the segment has an id in, so a segment costs the windows it touches, not
 *                            numIds / kSegWindow; an id in FRONT of the window was counted when that window was walked.  Then: the touched (or all
 *                            non-zero) slots set their bit in the bitmap; the bitmap's words are swept in order, one per thread -- popcounts under
 *                            a block prefix give the number of entries -- and cleared on the way, with the counters under their bits.  The
 *                            segment's number of entries goes to segFirst[k], 64-bit; what a thread has added to counters is summed over the
 *                            block at the end of the kernel and added to *sum, 64-bit, with one vector atomic per block
 *   pfac_array_scan          the exclusive 64-bit scan of the entry counts in place (scan_passes.h): segFirst[numSegments + 1], the length of the
 *                            list to the host
 *   pfac_segcount_pass<true, ALL>   the same walk for every segment that has an entry below `capacity` (all others leave at once): the popcount
 *                            prefix is the write position, ascending id order within the segment without a sort; (window base + bit, counter),
 *                            nothing at or beyond capacity
 *   (hipMemcpyAsync)         segFirst to the caller's array
 *   pfac_segcount_finish     *sum to the host; pfac_host_done behind it (scan_passes.h: HostHandoff)
 * Pass 2 recomputes what pass 1 found instead of staging it: a staged list would be as long as the count list, which has no bound the caller has not
 * set.  Whatever path a segment takes -- touched list, overflow sweep, truncation, no pair at all -- counter[], the bitmap, the touched count and
 * nextWindow are as the kernel's prologue left them when the segment ends.
 * ALL == false (PFACX_COUNT_LONGEST, or a set in which no pattern is a prefix of another) never reads the table.  With ALL the table reads repeat
 * per window like the LDS work: a pair's whole chain is read from the global table in every window its segment touches -- {prefixPattern, chainLen}
 * of every member, a dependent load a step --, also where the member lies in another window and is then dropped.  For a set of 100 000
 * patterns whose prefixes have ids in other windows than the patterns themselves that is the main work of a pass.
 * A SEGMENT IS ONE BLOCK'S WORK: its pairs are walked once per window it touches by 256 threads.  Counts over one huge buffer are what
 * PFACX_countFromDevice is for.
 * SCRATCH: 8 (numSegments + 1) + 8 bytes rounded up to 256 (DeviceScratch::segCount).  LDS of a block: 4 kSegWindow + kSegWindow / 8 + 2 kSegTouched
 * + 56 bytes = 35.05 KiB: four blocks, sixteen waves, on a compute unit's 160 KiB.
 * Plain C++, vector stores, LDS atomics and one 64-bit vector atomic per block only; the caller's offsets are not read here (scan_batch.hip has
 * clamped them into the first pairs, which are clamped to the pair list again where they are read).
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_segcount.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"

namespace {

constexpr unsigned int kSegBlockPairs = 256;                            /* pairs a block takes from a segment in one go: one per thread (pfac_amd/api.py: PFACX_SEGCOUNT_BLOCK_PAIRS) */
constexpr unsigned int kSegWindowLog2 = 13;
constexpr unsigned int kSegWindow = 1u << kSegWindowLog2;               /* ids per window: 32 KiB of counters, four blocks per compute unit (PFACX_SEGCOUNT_WINDOW) */
constexpr unsigned int kSegTouched = 1024;                              /* entries of the touched list (PFACX_SEGCOUNT_TOUCHED) */
constexpr unsigned int kSegWords = kSegWindow / 32;                     /* words of the bitmap */
constexpr unsigned int kNoWindow = 0xFFFFFFFFu;
static_assert(kSegWords == kSegBlockPairs, "the sweep gives every thread one word of the bitmap");
static_assert(kSegWindow <= 65536, "the touched list holds 16-bit slots");

struct SegCountArgs {
    const int *pairIds;                 /* the ordered longest pairs' ids */
    unsigned int count;
    const int *segFirstPairs;           /* [numSegments + 1], clamped where read; null: one segment of all pairs */
    unsigned int numSegments;
    const pfac::Int2 *table;            /* [numIds + 1] {prefixPattern, chainLen} by id; read with ALL only */
    unsigned int numIds;
    unsigned long long *segFirst;       /* [numSegments + 1]: pass 1 writes the entry counts, the scan turns them into the first entry of each segment */
    unsigned long long *sum;            /* the sum of all counts (zeroed in front of pass 1) */
    int *ids;
    unsigned int *counts;
    unsigned long long capacity;
};

/* the first pair of segment k among the `count` pairs */
__device__ __forceinline__ unsigned int firstPairOf(const SegCountArgs &a, unsigned int k)
{
    const int f = a.segFirstPairs[k];
    return f < 0 ? 0u : ((unsigned int)f < a.count ? (unsigned int)f : a.count);
}

template <bool EMIT, bool ALL>
__global__ __launch_bounds__(kSegBlockPairs) void pfac_segcount_pass(SegCountArgs a)
{
    __shared__ unsigned int counter[kSegWindow];
    __shared__ unsigned int bits[kSegWords];
    __shared__ unsigned short touched[kSegTouched];
    __shared__ unsigned int waveSum[kSegBlockPairs / 64];
    __shared__ unsigned long long waveSum64[kSegBlockPairs / 64];
    __shared__ unsigned int numTouched, nextWindow;
    const unsigned int t = threadIdx.x;
    for (unsigned int i = t; i < kSegWindow; i += kSegBlockPairs) counter[i] = 0;
    bits[t] = 0;
    if (t == 0) {
        numTouched = 0;
        nextWindow = kNoWindow;
    }
    __syncthreads();

    unsigned long long added = 0;                                                   /* what this thread has added to counters (pass 1 hands the block's sum on) */
    for (unsigned int k = blockIdx.x; k < a.numSegments; k += gridDim.x) {          /* (numSegments < 2^31: k + gridDim.x does not wrap) */
        unsigned long long base = 0;
        if constexpr (EMIT) {
            base = a.segFirst[k];
            if (a.segFirst[k + 1] == base || base >= a.capacity) continue;          /* no entry here, or none of them fits: the whole block leaves */
        }
        unsigned int first = 0, last = a.count;
        if (a.segFirstPairs != nullptr) {
            first = firstPairOf(a, k);
            last = firstPairOf(a, k + 1);
            if (last < first) last = first;                                         /* hostile offsets: an empty segment */
        }
        unsigned int entries = 0;                                                   /* of this segment so far: the same in every thread */
        unsigned int window = first < last ? 0u : kNoWindow;
        while (window != kNoWindow) {
            const unsigned int w0 = window << kSegWindowLog2;
            for (unsigned int i = first + t; i < last; i += kSegBlockPairs) {
                int q = a.pairIds[i];
                if (q < 1 || (unsigned int)q > a.numIds) continue;                  /* ignored, never used as an index */
                int steps = 1;                                                      /* the patterns on the chain, q included: the walk ends there whatever the table says */
                if constexpr (ALL) {
                    const int len = a.table[q].y;
                    steps = len > 1 ? len : 1;
                }
                for (int s = 0; s < steps && q >= 1 && (unsigned int)q <= a.numIds; s++) {
                    const unsigned int r = (unsigned int)q - w0;                    /* (wraps for an id in front of the window: counted there) */
                    if ((unsigned int)q >= w0) {
                        if (r >= kSegWindow) {
                            atomicMin(&nextWindow, (unsigned int)q >> kSegWindowLog2);
                        } else {
                            if (atomicAdd(&counter[r], 1u) == 0u) {
                                const unsigned int slot = atomicAdd(&numTouched, 1u);
                                if (slot < kSegTouched) touched[slot] = (unsigned short)r;
                            }
                            added++;
                        }
                    }
                    if constexpr (ALL) q = a.table[q].x;
                }
            }
            __syncthreads();
            const unsigned int n = numTouched, next = nextWindow;
            if (n != 0) {                                                           /* the same in every thread */
                if (n <= kSegTouched) {
                    for (unsigned int j = t; j < n; j += kSegBlockPairs) {
                        const unsigned int r = touched[j];
                        atomicOr(&bits[r >> 5], 1u << (r & 31u));
                    }
                } else {                                                            /* more slots than the list holds: every counter of the window */
                    for (unsigned int r = t; r < kSegWindow; r += kSegBlockPairs)
                        if (counter[r] != 0) atomicOr(&bits[r >> 5], 1u << (r & 31u));
                }
                __syncthreads();
                unsigned int word = bits[t];
                bits[t] = 0;
                unsigned int total = 0;
                const unsigned int before = blockExclusive<kSegBlockPairs>((unsigned int)__popc(word), waveSum, total);
                unsigned long long o = base + entries + before;
                while (word != 0) {                                                 /* a set bit is a non-zero counter: emitted in id order, cleared */
                    const unsigned int r = t * 32u + (unsigned int)__ffs((int)word) - 1u;
                    word &= word - 1u;
                    if constexpr (EMIT) {
                        if (o < a.capacity) {
                            a.ids[o] = (int)(w0 + r);
                            a.counts[o] = counter[r];
                        }
                        o++;
                    }
                    counter[r] = 0;
                }
                entries += total;
            }
            __syncthreads();                                                        /* everyone has read the two words */
            if (t == 0) {
                numTouched = 0;
                nextWindow = kNoWindow;
            }
            __syncthreads();
            window = next;
        }
        if constexpr (!EMIT) {
            if (t == 0) a.segFirst[k] = entries;
        }
    }
    if constexpr (!EMIT) {
        unsigned long long total = 0;
        (void)blockExclusive<kSegBlockPairs>(added, waveSum64, total);
        if (t == 0 && total != 0) atomicAdd(a.sum, total);
    }
}

/* the sum of the counts to the call's second mapped host value */
__global__ void pfac_segcount_finish(const unsigned long long *sum, unsigned long long *hostSum)
{
    storeToHost(hostSum, *sum);
}

} // namespace

extern "C" {

PFAC_status_t PFACX_segCountRun(PFAC_handle_t handle, const PFACX_segCountRun_t *run, size_t *h_numEntries, unsigned long long *h_total)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!run || !h_numEntries || !h_total || run->numSegments == 0 || run->numSegments >= (size_t)0x80000000u || run->count >= (size_t)0x80000000u ||
        run->numIds >= (size_t)0x7fffffff || (run->count && !run->d_pairIds) || !run->d_segFirst || (run->capacity && (!run->d_ids || !run->d_counts)))
        return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = handle;
    SegCountArgs a{};
    a.pairIds = run->d_pairIds;
    a.count = (unsigned int)run->count;
    a.segFirstPairs = run->d_segFirstPairs;
    a.numSegments = (unsigned int)run->numSegments;
    a.table = static_cast<const pfac::Int2 *>(run->d_table);
    a.numIds = (unsigned int)run->numIds;
    a.ids = run->d_ids;
    a.counts = run->d_counts;
    a.capacity = run->capacity;
    /* one region: segFirst[numSegments + 1], then the sum */
    const PFAC_status_t carved = carveScratch(c->scratch.segCount, [&](ScratchCarver &k) { a.segFirst = k.take<unsigned long long>(run->numSegments + 1, sizeof(unsigned long long)); });
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    a.sum = a.segFirst + a.numSegments + 1;
    if (hipMemsetAsync(a.sum, 0, sizeof(unsigned long long), nullptr) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
    const unsigned int grid = a.numSegments < gridCap(c, 4) ? a.numSegments : gridCap(c, 4);
    const HostHandoff list(c, pfac::kHostSegCount);
    const bool all = run->d_table != nullptr;
    const auto count = all ? pfac_segcount_pass<false, true> : pfac_segcount_pass<false, false>;
    const auto emit = all ? pfac_segcount_pass<true, true> : pfac_segcount_pass<true, false>;
    hipLaunchKernelGGL(count, dim3(grid), dim3(kSegBlockPairs), 0, 0, a);
    hipLaunchKernelGGL(pfac_array_scan<unsigned long long>, dim3(1), dim3(1024), 0, 0, a.segFirst, a.numSegments, a.segFirst + a.numSegments,
                       reinterpret_cast<unsigned long long *>(list.d_value));
    if (run->capacity) hipLaunchKernelGGL(emit, dim3(grid), dim3(kSegBlockPairs), 0, 0, a);
    if (hipMemcpyAsync(run->d_segFirst, a.segFirst, (run->numSegments + 1) * sizeof(unsigned long long), hipMemcpyDeviceToDevice, nullptr) != hipSuccess)
        return PFAC_STATUS_INTERNAL_ERROR;
    if (list.mapped())
        hipLaunchKernelGGL(pfac_segcount_finish, dim3(1), dim3(1), 0, 0, a.sum, reinterpret_cast<unsigned long long *>(list.d_value) + 1);
    unsigned long long both[2] = {0, 0};
    if (!list.finish(both, a.segFirst + a.numSegments, a.sum)) return PFAC_STATUS_INTERNAL_ERROR;
    *h_numEntries = (size_t)both[0];
    *h_total = both[1];
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
