/*
 * scan_segcount.hip -- per-segment occurrence counts in CSR form (include/pfac_ext.h: PFACX_countBatch*): how often each pattern occurs
 * in each segment of a batch.
 *
 * Pattern id occurs at a position of segment k iff it lies on the prefix chain (Automaton::prefixPattern) of the segment's LONGEST pair there, so
 * the count list follows from the ordered compacted batch scan (the pairs and the first pair of each segment, in handle scratch) and the
 * {prefixPattern, chainLen} table of the all-match calls.  Nothing here is sized by segments x patterns:
 *
 *   pfac_segcount_pass<false, ALL>  segmentWindows of scan_passes.h -- a block takes whole segments and walks a segment's pairs once per WINDOW
 *                            of kSegWindow ids it touches; the touched list, nextWindow, the bitmap and its sweep are the frame's -- over
 *                            counter[kSegWindow], a direct-indexed LDS table of 32-bit counters.  What is this unit's: a thread takes its pair's id
 *                            or, with ALL, every id on its prefix chain (at most chainLen steps, ended by the table's bounds whatever the table
 *                            says).  An id in the window adds 1 to its counter with an LDS atomic; whoever sees the counter go from 0 touches the
 *                            slot; an id BEHIND the window is handed to the frame (beyond); an id in FRONT of it was counted when that window was
 *                            walked.  Every touched slot is an entry, and its counter is cleared under its bit in the sweep, behind its emit
 *                            (RESET_IN_SWEEP: every touched window is swept to its end in both passes).  The segment's number of entries goes to
 *                            segFirst[k], 64-bit; what a thread has added to counters is summed over the block at the end of the kernel and added to
 *                            *sum, 64-bit, with one vector atomic per block
 *   pfac_array_scan          the exclusive 64-bit scan of the entry counts in place (scan_passes.h): segFirst[numSegments + 1], the length of the
 *                            list to the host
 *   pfac_segcount_pass<true, ALL>   the same walk for every segment that has an entry below `capacity` (all others leave at once): the popcount
 *                            prefix is the write position, ascending id order within the segment without a sort; (window base + bit, counter),
 *                            nothing at or beyond capacity
 *   (hipMemcpyAsync)         segFirst to the caller's array
 *   pfac_segcount_finish     *sum to the host; pfac_host_done behind it (scan_passes.h: HostHandoff)
 * Pass 2 recomputes what pass 1 found instead of staging it: a staged list would be as long as the count list, which has no bound the caller has not
 * set.  The launches are segmentWindowPasses (scan_passes.h), with pfac_segcount_finish behind them.
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

struct SegCountArgs {
    SegmentFrame f;                     /* the pairs' count, the segments' first pairs, segFirst, the capacity (scan_passes.h) */
    const int *pairIds;                 /* the ordered longest pairs' ids */
    const pfac::Int2 *table;            /* [numIds + 1] {prefixPattern, chainLen} by id; read with ALL only */
    unsigned int numIds;
    unsigned long long *sum;            /* the sum of all counts (zeroed in front of pass 1) */
    int *ids;
    unsigned int *counts;
};

/* the frame of scan_passes.h (segmentWindows) over counter[]: a slot is an id's counter, every touched one an entry, cleared in the sweep behind
 * its emit */
template <bool EMIT, bool ALL>
__global__ __launch_bounds__(kSegBlockPairs) void pfac_segcount_pass(SegCountArgs a)
{
    __shared__ unsigned int counter[kSegWindow];
    __shared__ unsigned long long waveSum64[kSegBlockPairs / 64];
    unsigned long long added = 0;                                                   /* what this thread has added to counters (pass 1 hands the block's sum on) */
    segmentWindows<EMIT, kSegWindowLog2, kSegTouched, kSegBlockPairs, true>(
        a.f, counter, [](unsigned int) {},
        [&](unsigned int i, unsigned int w0, auto touch, auto beyond) {
            /* the patterns on the pair's chain, without ALL -- no table: it is not read -- the pair alone; an id outside [1, numIds] is ignored,
             * never used as an index (scan_passes.h: forEachChainMember) */
            const pfac::Int2 *table = nullptr;
            if constexpr (ALL) table = a.table;
            forEachChainMember(table, a.numIds, a.pairIds[i], [&](int q) {
                const unsigned int r = (unsigned int)q - w0;                        /* (wraps for an id in front of the window: counted there) */
                if ((unsigned int)q >= w0) {
                    if (r >= kSegWindow) {
                        beyond((unsigned int)q >> kSegWindowLog2);
                    } else {
                        if (atomicAdd(&counter[r], 1u) == 0u) touch(r);
                        added++;
                    }
                }
                return true;
            });
        },
        [](unsigned int, unsigned int) { return true; },
        [&](unsigned long long o, unsigned int, unsigned int id, unsigned int count) {
            a.ids[o] = (int)id;
            a.counts[o] = count;
        });
    if constexpr (!EMIT) {
        unsigned long long total = 0;
        (void)blockExclusive<kSegBlockPairs>(added, waveSum64, total);
        if (threadIdx.x == 0 && total != 0) atomicAdd(a.sum, total);
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
    a.f.count = (unsigned int)run->count;
    a.f.segFirstPairs = run->d_segFirstPairs;
    a.f.numSegments = (unsigned int)run->numSegments;
    a.f.capacity = run->capacity;
    a.pairIds = run->d_pairIds;
    a.table = static_cast<const pfac::Int2 *>(run->d_table);
    a.numIds = (unsigned int)run->numIds;
    a.ids = run->d_ids;
    a.counts = run->d_counts;
    /* one region: segFirst[numSegments + 1], then the sum */
    const PFAC_status_t carved = carveSegFirst(c->scratch.segCount, a.f, sizeof(unsigned long long));
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    a.sum = a.f.segFirst + a.f.numSegments + 1;
    if (hipMemsetAsync(a.sum, 0, sizeof(unsigned long long), nullptr) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
    const HostHandoff list(c, pfac::kHostSegCount);
    const bool all = run->d_table != nullptr;
    const auto count = all ? pfac_segcount_pass<false, true> : pfac_segcount_pass<false, false>;
    const auto emit = all ? pfac_segcount_pass<true, true> : pfac_segcount_pass<true, false>;
    if (!segmentWindowPasses(c, a, count, emit, kSegBlockPairs, list, run->d_segFirst)) return PFAC_STATUS_INTERNAL_ERROR;
    if (list.mapped())
        hipLaunchKernelGGL(pfac_segcount_finish, dim3(1), dim3(1), 0, 0, a.sum, reinterpret_cast<unsigned long long *>(list.d_value) + 1);
    unsigned long long both[2] = {0, 0};
    if (!list.finish(both, a.f.segFirst + a.f.numSegments, a.sum)) return PFAC_STATUS_INTERNAL_ERROR;
    *h_numEntries = (size_t)both[0];
    *h_total = both[1];
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
