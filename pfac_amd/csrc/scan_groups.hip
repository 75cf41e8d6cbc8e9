/*
 * scan_groups.hip -- pattern groups (include/pfac_ext.h: PFACX_groups*): each segment of a batch sees only the patterns whose 64-bit
 * group mask meets the segment's.
 *
 * Every pattern that starts at p is a prefix of the longest one L that starts there, so the occurrences at p are L's prefix chain (scan_all.hip), and
 * the enabled ones are the members q with patMasks[q] & segMasks[segment] != 0.  The passes work on an ordered list of LONGEST pairs with the first
 * pair of each segment -- the handle's pair scratch behind the ordered compacted batch scan, or a list of the caller's -- and never read the input:
 *   (hipMemsetAsync)     segGroups zeroed, where it is given
 *   pfac_groups_bounds   with a segment array: bounds[k] = the first pair of segment k, every entry clamped to [0, count] where it is read and raised
 *                        to the largest entry in front of it (a block of 1024 threads per 8192 entries; it folds what lies in front of them itself,
 *                        like pfac_block_scan).  The passes below read only this array: ascending, inside the pair list, whatever the caller gave
 *   pfac_groups_count    a thread per pair, blocks of kGroupsBlock, cut by offsetBlocks.  The pair's segment, its mask once, then the chain from the
 *                        longest pattern down through {prefix, chain length}, patMasks[q] ANDed with the mask.  The value of a pair is 0 / 1 (the
 *                        first enabled member) or 0 .. chainLen (ALL); the hit bits are ORed over the WHOLE chain in both modes.  Block totals
 *                        through expandCount (scan_passes.h); the lanes of a wave that share a segment combine their hit bits by shuffles (both halves of
 *                        the 64 bits), the last lane of each run adds them to segGroups[segment] with one 64-bit atomicOr
 *   pfac_array_scan      exclusive scan of the block totals (one block; 64-bit), the length of the list to mapped host memory
 *   pfac_groups_write    only with capacity > 0 or segFirst given: expandWrite, the chain again, (id, pos) into the slots below `capacity` by the frame, and
 *                        segFirst (see below)
 *   pfac_host_done       the call's sequence number to mapped host memory (scan_passes.h: HostHandoff)
 * THE PAIR'S SEGMENT.  Pairs are ordered by segment: pair i lies in segment u(i) - 1, u(i) = the number of bounds <= i (0: in front of the first
 * bound, numSegments + 1: behind the last; both: no segment).  A block searches the bounds ONCE for its first and its last pair, the whole wave at a
 * time (waveLowerBound); a lane then searches only between the two, log2(1 + the segments its block's pairs span) steps.  Without a segment array
 * there is nothing to search.
 * WHO WRITES segFirst[k], k in [0, numSegments].  An entry with bounds[k] = i < count belongs to the thread of pair i in pfac_groups_write: it
 * writes the list offset in front of its pair to every such k, from u(i) - 1 downwards -- one entry where the segment in front of it has pairs, a
 * run of them behind empty segments.  The entries with bounds[k] == count -- the segments behind the last pair, and entry numSegments -- get the
 * length of the list from a grid-stride loop of the same launch.  Every entry has exactly one writer.
 * THE FRAME.  The walk along the chain (forEachChainMember), both passes, the capacity-checked store and the launches (expandPasses) are the expansion
 * frame of scan_passes.h, shared with scan_all.hip and scan_words.hip; this unit's own are the pair's segment, the test of a member (walkChain),
 * the hit bits and segFirst (the hook of the write pass).
 * BOUNDS: an id is checked against [1, numIds] before it indexes anything; a walk ends after chainLen steps and at an id outside [1, numIds]
 * whatever the table says (both in forEachChainMember); a segment index is below numSegments where it indexes segMasks or segGroups; positions are copied, never used.
 * SCRATCH: 8 (blocks + 1) bytes rounded up to 256, then 4 (numSegments + 1) bytes rounded up to 256 with a segment array (DeviceScratch::groups).
 * Plain C++, vector stores and 64-bit vector atomics only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_groups.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"

namespace {

constexpr unsigned int kGroupsBlock = 256;                              /* pairs a block takes in one go (pfac_amd/api.py: PFACX_GROUPS_BLOCK) */
constexpr unsigned int kBoundsPer = 8;                                  /* bounds per thread of pfac_groups_bounds */
constexpr unsigned int kBoundsBlock = 1024 * kBoundsPer;
constexpr unsigned int kNoSegment = 0xFFFFFFFFu;

struct GroupsArgs {
    ExpandFrame f;                      /* the pairs, the chain table, PFACX_GROUPS_ALL, the block cut, the caller's arrays (scan_passes.h) */
    const unsigned int *bounds;         /* [numSegments + 1] ascending, inside [0, count] (pfac_groups_bounds); null: one segment of all pairs */
    unsigned int numSegments;
    const unsigned long long *segMasks; /* [numSegments], or null: all bits */
    const unsigned long long *patMasks; /* [numIds + 1] by id */
    unsigned long long *segFirst;       /* [numSegments + 1], or null */
    unsigned long long *segGroups;      /* [numSegments], or null (zeroed in front of the count pass) */
};

/* bounds[k] = the largest of the clamped entries [0, k] of segFirstPairs, k < n = numSegments + 1 */
__global__ __launch_bounds__(1024) void pfac_groups_bounds(const int *segFirstPairs, unsigned int n, unsigned int count, unsigned int *bounds)
{
    __shared__ unsigned int waveOwn[16], waveFront[16];
    const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned int base = blockIdx.x * kBoundsBlock, i0 = base + threadIdx.x * kBoundsPer;
    unsigned int front = 0;                                             /* what lies in front of the block's entries: coalesced, from L2 */
    for (unsigned int q = threadIdx.x; q < base; q += 1024u) front = OpMax()(front, clampFirstPair(segFirstPairs[q], count));
    unsigned int x[kBoundsPer], own = 0;
#pragma unroll
    for (unsigned int k = 0; k < kBoundsPer; k++) {
        x[k] = i0 + k < n ? clampFirstPair(segFirstPairs[i0 + k], count) : 0u;
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

/* where the bounds of a block's pairs lie: u(i) of every pair i of the block is inside [lo, hi] */
struct BlockSegs { unsigned int lo, hi; };

/* ... found once per block, by every wave alike (all 64 lanes call it): u of the block's first and of its last pair */
__device__ __forceinline__ BlockSegs blockSegs(const GroupsArgs &a)
{
    BlockSegs b{1u, 1u};                                                /* no segment array: u(i) = 1, segment 0 */
    if (a.bounds == nullptr) return b;
    const size_t first = (size_t)blockIdx.x * a.f.per;
    const size_t end = a.f.count - first < a.f.per ? a.f.count : first + a.f.per;
    const unsigned int iLo = (unsigned int)first, iHi = (unsigned int)(end - 1);
    b.lo = waveLowerBound(0u, a.numSegments + 1u, [&](unsigned int k) { return a.bounds[k] > iLo; });
    b.hi = waveLowerBound(b.lo, a.numSegments + 1u, [&](unsigned int k) { return a.bounds[k] > iHi; });
    return b;
}

/* u(i) of pair i of the block: the first k of [b.lo, b.hi) with bounds[k] > i, else b.hi; a lane by itself */
__device__ __forceinline__ unsigned int boundsUpTo(const GroupsArgs &a, const BlockSegs &b, unsigned int i)
{
    unsigned int lo = b.lo, hi = b.hi;
    while (lo < hi) {
        const unsigned int mid = lo + ((hi - lo) >> 1);
        if (a.bounds[mid] > i) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

/* the segment of a pair with u bounds at or in front of it */
__device__ __forceinline__ unsigned int segmentOf(const GroupsArgs &a, unsigned int u) { return u >= 1u && u <= a.numSegments ? u - 1u : kNoSegment; }

/* The enabled members of the chain of pattern id under the segment mask, longest first (scan_passes.h: forEachChainMember): emit(q) for each that
 * is reported (list mode: the first alone); returns their number.  HITS: the whole chain is walked and `hits` takes mask & segment mask of every
 * member, reported or not */
template <bool HITS, class Emit>
__device__ __forceinline__ unsigned int walkChain(const GroupsArgs &a, int id, unsigned long long segMask, unsigned long long &hits, Emit emit)
{
    if (segMask == 0ull) return 0u;
    unsigned int found = 0;
    forEachChainMember(a.f.table, a.f.numIds, id, [&](int q) {
        const unsigned long long m = a.patMasks[q] & segMask;
        if (m == 0ull) return true;
        if (HITS) hits |= m;
        if (a.f.all || found == 0u) {
            emit(q);
            found++;
        }
        return HITS || a.f.all != 0u;
    });
    return found;
}

/* The hit bits of the lanes that share a segment, ORed, to segGroups[segment]: one atomic per run of lanes.  Called where the lanes of a wave that
 * are active are its first ones (a thread per pair, in order) and their segments ascend: a shuffle reads a lower lane, which is active too */
__device__ __forceinline__ void addSegmentHits(unsigned long long *segGroups, unsigned int seg, unsigned long long hits)
{
    const unsigned int lane = threadIdx.x & 63u;
    const unsigned long long active = __ballot(1);
    const unsigned int before = __shfl_up(seg, 1);
    const unsigned long long heads = __ballot(lane == 0 || before != seg);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long h = __shfl_up(hits, d);        /* 64 bits: both halves */
        const unsigned int s = __shfl_up(seg, d);
        if ((int)lane >= d && s == seg) hits |= h;
    }
    /* the last lane of a run: the one in front of a head, and the last active one */
    const unsigned long long tails = heads >> 1 | 1ull << (63 - __clzll((long long)active));
    if ((tails >> lane & 1ull) && seg != kNoSegment && hits != 0ull) atomicOr(&segGroups[seg], hits);
}

__global__ __launch_bounds__(kGroupsBlock) void pfac_groups_count(GroupsArgs a)
{
    const BlockSegs b = blockSegs(a);
    expandCount<kGroupsBlock>(a.f, [&](size_t k) -> unsigned long long {
        const unsigned int seg = segmentOf(a, a.bounds != nullptr ? boundsUpTo(a, b, (unsigned int)k) : 1u);
        unsigned long long hits = 0;
        unsigned int found = 0;
        if (seg != kNoSegment)
            found = walkChain<true>(a, a.f.pairIds[k], a.segMasks != nullptr ? a.segMasks[seg] : ~0ull, hits, [](int) {});
        if (a.segGroups != nullptr) addSegmentHits(a.segGroups, seg, hits);
        return found;
    });
}

__global__ __launch_bounds__(kGroupsBlock) void pfac_groups_write(GroupsArgs a)
{
    const BlockSegs b = blockSegs(a);
    const unsigned int count = (unsigned int)a.f.count;
    /* the entries of segFirst that no pair owns: bounds[k] == count */
    if (a.segFirst != nullptr) {
        const unsigned int tail = a.bounds != nullptr ? waveLowerBound(0u, a.numSegments + 1u, [&](unsigned int k) { return a.bounds[k] >= count; }) : 1u;
        const unsigned long long total = a.f.blockBase[gridDim.x];
        for (size_t k = (size_t)tail + (size_t)blockIdx.x * kGroupsBlock + threadIdx.x; k <= a.numSegments; k += (size_t)gridDim.x * kGroupsBlock)
            a.segFirst[k] = total;
    }
    unsigned int u = 1u;                                        /* of the pair a thread has just valued: left to its store */
    unsigned long long segMask = 0;
    unsigned long long unused = 0;
    expandWrite<kGroupsBlock>(
        a.f,
        [&](size_t k) -> unsigned long long {
            u = a.bounds != nullptr ? boundsUpTo(a, b, (unsigned int)k) : 1u;
            const unsigned int seg = segmentOf(a, u);
            segMask = seg == kNoSegment ? 0ull : (a.segMasks != nullptr ? a.segMasks[seg] : ~0ull);
            return walkChain<false>(a, a.f.pairIds[k], segMask, unused, [](int) {});
        },
        [&](size_t k, auto emit) { (void)walkChain<false>(a, a.f.pairIds[k], segMask, unused, emit); },
        [&](size_t k, unsigned long long before) {
            if (a.segFirst == nullptr) return;                  /* every segment that starts at this pair */
            if (a.bounds == nullptr) {
                if (k == 0) a.segFirst[0] = before;
            } else {
                for (unsigned int j = u; j > 0u && a.bounds[j - 1u] == (unsigned int)k; j--) a.segFirst[j - 1u] = before;
            }
        });
}

} // namespace

extern "C" {

PFAC_status_t PFACX_groupsRun(PFAC_handle_t handle, const PFACX_groupsRun_t *run, size_t *h_total)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!run || !h_total || run->numSegments == 0 || run->numSegments >= (size_t)0x80000000u || run->count >= (size_t)0x80000000u ||
        run->numIds >= (size_t)0x7fffffff || !run->d_patternMasks || (run->count && (!run->d_pairIds || !run->d_pairPos)) ||
        (run->capacity && (!run->d_ids || !run->d_pos)) || (!run->d_segFirstPairs && run->numSegments != 1))
        return PFAC_STATUS_INVALID_PARAMETER;
    *h_total = 0;
    if (run->count == 0) {                                      /* no pair: nothing to launch */
        if (run->d_segFirst && hipMemsetAsync(run->d_segFirst, 0, (run->numSegments + 1) * sizeof(size_t), nullptr) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
        if (run->d_segGroups && hipMemsetAsync(run->d_segGroups, 0, run->numSegments * sizeof(unsigned long long), nullptr) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
        return hipStreamSynchronize(nullptr) == hipSuccess ? PFAC_STATUS_SUCCESS : PFAC_STATUS_INTERNAL_ERROR;
    }
    PFAC_context *c = handle;
    GroupsArgs a{};
    a.f = ExpandFrame{run->d_pairIds, run->d_pairPos, run->count, static_cast<const pfac::Int2 *>(run->d_table), (unsigned int)run->numIds,
                      run->all ? 1u : 0u, 0, nullptr, run->d_ids, run->d_pos, run->capacity};
    a.numSegments = (unsigned int)run->numSegments;
    a.segMasks = run->d_segMasks;
    a.patMasks = run->d_patternMasks;
    static_assert(sizeof(size_t) == sizeof(unsigned long long), "segFirst is written as 64-bit words");
    a.segFirst = reinterpret_cast<unsigned long long *>(run->d_segFirst);
    a.segGroups = run->d_segGroups;
    unsigned int *bounds = nullptr;
    return expandPasses(
        c, c->scratch.groups, pfac::kHostGroups, a, pfac_groups_count, pfac_groups_write, kGroupsBlock, a.f.capacity || a.segFirst, h_total,
        [&](ScratchCarver &k) {
            if (run->d_segFirstPairs) a.bounds = bounds = k.take<unsigned int>(run->numSegments + 1);
        },
        false,
        [&]() {                                                 /* in front of the passes: segGroups zeroed, the bounds */
            if (a.segGroups && hipMemsetAsync(a.segGroups, 0, run->numSegments * sizeof(unsigned long long), nullptr) != hipSuccess) return false;
            if (bounds)
                hipLaunchKernelGGL(pfac_groups_bounds, dim3((a.numSegments + 1u + kBoundsBlock - 1u) / kBoundsBlock), dim3(1024), 0, 0,
                                   run->d_segFirstPairs, a.numSegments + 1u, (unsigned int)a.f.count, bounds);
            return true;
        });
}

} /* extern "C" */
