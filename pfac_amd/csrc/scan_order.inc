/*
 * scan_order.inc -- compacted output: the four ordering kernels and PairOrder (included by scan_module.hip inside its unnamed namespace)
 */
/* ------------------------------------------------- compacted output: the pairs in position order */

/* The scan leaves (position, id) pairs in the order its walks finished.  Positions are DISTINCT keys below n, so they
 * are ordered with a counting pass over position bins and a rank inside each bin -- four short launches over the pairs
 * (~0.6 M for the bench stream, ~35 us together) instead of a general radix sort (rocPRIM Onesweep: a histogram and four
 * digit passes with decoupled look-back, 0.12 ms for the same pairs).  The number of pairs is read from the device
 * counter: the launches are queued behind the scan without the host knowing it.
 *   pfac_order_count    pairs per bin (bin = position >> shift, at most 2^16 bins).  64 consecutive pairs of the list
 *                       come from four flushes of scanning waves, i.e. from a handful of bins: one atomic per distinct
 *                       bin and wave, not per pair (the part sustains ~25 atomics per ns)
 *   pfac_order_offsets  exclusive prefix sum of the counters: block k sums everything in front of its 1024 counters
 *                       itself (at most 252 KiB, coalesced, from L2) -- no pass between blocks; lists the bins with
 *                       more than 64 pairs
 *   pfac_order_scatter  pair -> its bin's range of the scratch arrays (any order inside the bin); the lanes of a wave
 *                       that share a bin share one atomic, all of a wave's atomics are one instruction
 *   pfac_order_rank     one thread per pair: final place = bin start + number of smaller positions in the bin; then
 *                       the bins with more than 64 pairs, one block per listed bin: the bin's positions as a bitmap
 *                       in LDS, rank = set bits below
 * More pairs than the scratch arrays hold: every launch leaves at once, the host grows the scratch and queues them again.
 *
 * Round 5: the launches clean up behind themselves -- the scatter pass leaves the bin counters zero; the pairs' and the crowded bins'
 * counters exist twice, calls alternate between them and the rank pass zeroes the pair the NEXT call will use (a last-block-out counter
 * instead: 2048 blocks asking one device counter, the rank pass 8.5 -> 29 us) -- and the count pass writes the number of pairs to a word of mapped host memory: a call whose
 * predecessor used the same layout needs no memset in front of its scan and no device-to-host copy behind it (PairOrder, reduceScan).
 * (The four passes as the phases of ONE launch, three grid barriers between agent-scope fences: 0.125 ms behind the scan instead of
 * 0.072 -- every barrier is a write-back and an invalidate of the XCDs' whole L2s -- measured and dropped.)
 */
constexpr unsigned kOrderMaxBinsLog2 = 16;
constexpr unsigned kOrderMinShift = 6;           /* a bin of 64 positions holds at most 64 pairs */
constexpr unsigned kOrderMaxShift = 15;          /* int input_size < 2^31 */
constexpr unsigned kOrderBlockBins = 1024;       /* counters per block of pfac_order_offsets */
constexpr unsigned kOrderCrowded = 64;

struct OrderArgs {
    const unsigned int *posIn;     /* the scan's pairs, any order */
    const int *idIn;
    unsigned int *count;           /* device counter of the pairs (behind crowdedCount: one memset clears all counters of a call) */
    unsigned int capacity;         /* pairs posTmp / idTmp hold */
    unsigned int shift;
    unsigned int bins;
    unsigned int *counts;          /* bins rounded up to whole blocks (zeros), then the crowded bins' counter and the pairs' counter */
    unsigned int *cursor;          /* same length: start -> (after the scatter) end of each bin */
    unsigned int *crowdedCount;
    unsigned int *crowded;         /* bins */
    unsigned int *posTmp;
    int *idTmp;
    unsigned int *posOut;
    int *idOut;
    unsigned int *nextCounters;    /* the crowded bins' and the pairs' counter of the handle's next call (two words): the rank pass leaves them zero */
    unsigned int *hostCount;       /* mapped host memory: the number of pairs, for the host (or null) */
    unsigned int paddedBins;       /* counters the scatter pass leaves zero */
};

__device__ __forceinline__ void orderCountPhase(const OrderArgs &o, unsigned int count)
{
    const unsigned int lane = threadIdx.x & 63u;
    for (unsigned int first = blockIdx.x * 256u + (threadIdx.x & ~63u); first < count; first += gridDim.x * 256u) {
        const bool has = first + lane < count;
        const unsigned int b = has ? o.posIn[first + lane] >> o.shift : 0xFFFFFFFFu;
        unsigned long long todo = __ballot(has);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const unsigned int b0 = (unsigned int)__builtin_amdgcn_readlane((int)b, leader);
            const unsigned long long same = __ballot(b == b0);
            if ((int)lane == leader) atomicAdd(&o.counts[b0], (unsigned int)__popcll(same));
            todo &= ~same;
        }
    }
}

/* the cursors of the 1024 bins of block `blk` (every thread of the block calls it) */
__device__ __forceinline__ void orderOffsetsPhase(const OrderArgs &o, unsigned int blk, unsigned int *waveSum)
{
    const unsigned int t = threadIdx.x;
    const unsigned int firstQuad = blk * (kOrderBlockBins / 4);
    const u32x4 *all = reinterpret_cast<const u32x4 *>(o.counts);
    unsigned int front = 0;
    unsigned int q = t;
    for (; q + 7u * 256u < firstQuad; q += 8u * 256u) {                 /* eight loads in flight: the last block reads 252 KiB */
        u32x4 v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = all[q + k * 256u];
#pragma unroll
        for (int k = 0; k < 8; k++) front += v[k].x + v[k].y + v[k].z + v[k].w;
    }
    for (; q < firstQuad; q += 256u) {
        const u32x4 v = all[q];
        front += v.x + v.y + v.z + v.w;
    }
    const u32x4 c = all[firstQuad + t];
    unsigned int base = 0, ignored = 0;
    (void)blockExclusive<256>(front, waveSum, base);
    unsigned int run = base + blockExclusive<256>(c.x + c.y + c.z + c.w, waveSum, ignored);
    const unsigned int bin = (firstQuad + t) * 4;
    if (c.x > kOrderCrowded) o.crowded[atomicAdd(o.crowdedCount, 1u)] = bin;
    if (c.y > kOrderCrowded) o.crowded[atomicAdd(o.crowdedCount, 1u)] = bin + 1;
    if (c.z > kOrderCrowded) o.crowded[atomicAdd(o.crowdedCount, 1u)] = bin + 2;
    if (c.w > kOrderCrowded) o.crowded[atomicAdd(o.crowdedCount, 1u)] = bin + 3;
    u32x4 s;
    s.x = run; run += c.x;
    s.y = run; run += c.y;
    s.z = run; run += c.z;
    s.w = run;
    reinterpret_cast<u32x4 *>(o.cursor)[firstQuad + t] = s;
}

__device__ __forceinline__ void orderScatterPhase(const OrderArgs &o, unsigned int count)
{
    const unsigned int lane = threadIdx.x & 63u;
    for (unsigned int first = blockIdx.x * 256u + (threadIdx.x & ~63u); first < count; first += gridDim.x * 256u) {
        const bool has = first + lane < count;
        const unsigned int p = has ? o.posIn[first + lane] : 0xFFFFFFFFu;
        const int id = has ? o.idIn[first + lane] : 0;
        const unsigned int b = has ? p >> o.shift : 0xFFFFFFFFu;
        /* the lanes that share a bin: the first of them takes the bin's cursor forward for all */
        unsigned int myLeader = lane, myRank = 0, groupSize = 0;
        unsigned long long todo = __ballot(has);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const unsigned int b0 = (unsigned int)__builtin_amdgcn_readlane((int)b, leader);
            const unsigned long long same = __ballot(b == b0);
            if (b == b0) {
                myLeader = (unsigned int)leader;
                myRank = (unsigned int)__popcll(same & ((1ull << lane) - 1ull));
                groupSize = (unsigned int)__popcll(same);
            }
            todo &= ~same;
        }
        unsigned int base = 0;
        if (has && lane == myLeader) base = atomicAdd(&o.cursor[b], groupSize);
        base = (unsigned int)__shfl((int)base, (int)myLeader);
        if (has) { o.posTmp[base + myRank] = p; o.idTmp[base + myRank] = id; }
    }
}

/* bits / below: 2^(kOrderMaxShift - 5) words each: the positions of one crowded bin, set bits in front of each word */
__device__ __forceinline__ void orderRankPhase(const OrderArgs &o, unsigned int count, unsigned int *bits, unsigned int *below, unsigned int *waveSum)
{
    const unsigned int listed = *o.crowdedCount;
    for (unsigned int i = blockIdx.x * 256u + threadIdx.x; i < count; i += gridDim.x * 256u) {
        const unsigned int p = o.posTmp[i];
        const int id = o.idTmp[i];
        const unsigned int b = p >> o.shift;
        const unsigned int end = o.cursor[b], start = b ? o.cursor[b - 1] : 0u;
        if (end - start > kOrderCrowded) continue;                       /* placed below */
        unsigned int rank = 0;
        for (unsigned int j = start; j < end; j++) rank += o.posTmp[j] < p ? 1u : 0u;
        o.posOut[start + rank] = p;
        o.idOut[start + rank] = id;
    }
    /* bins with more than 64 pairs, one block per listed bin (the same trip count for every thread of the block) */
    const unsigned int t = threadIdx.x;
    const unsigned int words = 1u << (o.shift - 5), mask = (1u << o.shift) - 1u;
    for (unsigned int k = blockIdx.x; k < listed; k += gridDim.x) {
        const unsigned int b = o.crowded[k];
        const unsigned int end = o.cursor[b], start = b ? o.cursor[b - 1] : 0u, c = end - start;
        for (unsigned int w = t; w < words; w += 256u) bits[w] = 0;
        __syncthreads();
        for (unsigned int e = t; e < c; e += 256u) {
            const unsigned int p = o.posTmp[start + e] & mask;
            atomicOr(&bits[p >> 5], 1u << (p & 31u));
        }
        __syncthreads();
        /* exclusive prefix of the words' population counts: `per` consecutive words per thread */
        const unsigned int per = words > 256u ? words / 256u : 1u;
        unsigned int own = 0;
        for (unsigned int j = 0; j < per; j++) {
            const unsigned int w = t * per + j;
            if (w < words) own += (unsigned int)__popc(bits[w]);
        }
        unsigned int ignored = 0;
        unsigned int run = blockExclusive<256>(own, waveSum, ignored);
        for (unsigned int j = 0; j < per; j++) {
            const unsigned int w = t * per + j;
            if (w < words) { below[w] = run; run += (unsigned int)__popc(bits[w]); }
        }
        __syncthreads();
        for (unsigned int e = t; e < c; e += 256u) {
            const unsigned int pos = o.posTmp[start + e], p = pos & mask;
            const unsigned int rank = below[p >> 5] + (unsigned int)__popc(bits[p >> 5] & ((1u << (p & 31u)) - 1u));
            o.posOut[start + rank] = pos;
            o.idOut[start + rank] = o.idTmp[start + e];
        }
        __syncthreads();
    }
}


__global__ __launch_bounds__(256) void pfac_order_count(OrderArgs o)
{
    const unsigned int count = *o.count;                   /* final: the scan is over */
    if (blockIdx.x == 0 && threadIdx.x == 0 && o.hostCount != nullptr) {
        __hip_atomic_store(o.hostCount, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __threadfence_system();
    }
    if (count > o.capacity) return;
    orderCountPhase(o, count);
}

__global__ __launch_bounds__(256) void pfac_order_offsets(OrderArgs o)
{
    __shared__ unsigned int waveSum[4];
    if (*o.count > o.capacity) return;
    orderOffsetsPhase(o, blockIdx.x, waveSum);
}

__global__ __launch_bounds__(256) void pfac_order_scatter(OrderArgs o)
{
    const unsigned int count = *o.count;
    if (count > o.capacity) return;
    orderScatterPhase(o, count);
    for (unsigned int i = blockIdx.x * 256u + threadIdx.x; i < o.paddedBins / 4u; i += gridDim.x * 256u)      /* the next call's counters */
        reinterpret_cast<u32x4 *>(o.counts)[i] = u32x4{0, 0, 0, 0};
}

__global__ __launch_bounds__(256) void pfac_order_rank(OrderArgs o)
{
    __shared__ unsigned int bits[1u << (kOrderMaxShift - 5)];
    __shared__ unsigned int below[1u << (kOrderMaxShift - 5)];
    __shared__ unsigned int waveSum[4];
    const unsigned int count = *o.count;
    if (count > o.capacity) return;
    orderRankPhase(o, count, bits, below, waveSum);
    if (blockIdx.x == 0 && threadIdx.x == 0) { o.nextCounters[0] = 0; o.nextCounters[1] = 0; }     /* nobody uses them before the next call's scan */
}


/* grow-only device scratch of the compacted-output path, owned by the handle (the caller holds its lock) */
PFAC_status_t reduceScratch(PFAC_context *mc, size_t need, char **base)
{
    if (mc->scratch.reduce.count() < need) {
        mc->orderCleanBase = nullptr;                      /* a new allocation: nobody has left its counters zero */
        const PFAC_status_t st = mc->scratch.reduce.reserve(need + need / 2);
        if (st != PFAC_STATUS_SUCCESS) return st;
    }
    *base = mc->scratch.reduce.get();
    return PFAC_STATUS_SUCCESS;
}

/* The ordering of a compacted-output call over n input bytes: the handle's scratch cut into the arrays of OrderArgs
 * (room for at least `pairs` pairs; all the scratch there is), then clearCounters() in front of the scan and order()
 * behind it, both asynchronous on the null stream. */
struct PairOrder {
    OrderArgs o{};
    size_t counterBytes = 0;

    /* parity: which of the two {crowded bins, pairs} counter pairs this call uses (PFAC_context::orderParity) */
    PFAC_status_t plan(PFAC_context *mc, size_t n, size_t pairs, int *d_ids, int *d_pos, unsigned int parity)
    {
        unsigned int log2n = 1;
        while (log2n < 32 && (n - 1) >> log2n) log2n++;
        o.shift = log2n > kOrderMaxBinsLog2 + kOrderMinShift ? log2n - kOrderMaxBinsLog2 : kOrderMinShift;
        if (o.shift > kOrderMaxShift) return PFAC_STATUS_INTERNAL_ERROR;
        o.bins = (unsigned int)(((n - 1) >> o.shift) + 1);
        const size_t padded = ((size_t)o.bins + kOrderBlockBins - 1) / kOrderBlockBins * kOrderBlockBins;
        counterBytes = (padded * sizeof(unsigned int) + 4 * sizeof(unsigned int) + 255) / 256 * 256;
        const size_t cursorBytes = padded * sizeof(unsigned int);
        const size_t listBytes = ((size_t)o.bins * sizeof(unsigned int) + 255) / 256 * 256;
        const size_t fixed = counterBytes + cursorBytes + listBytes;
        const size_t arrayBytes = (pairs * sizeof(int) + 255) / 256 * 256;
        char *base = nullptr;
        const PFAC_status_t st = reduceScratch(mc, fixed + 2 * arrayBytes, &base);
        if (st != PFAC_STATUS_SUCCESS) return st;
        const size_t perArray = (mc->scratch.reduce.count() - fixed) / 2 / 256 * 256;
        o.capacity = perArray / sizeof(int) > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned int)(perArray / sizeof(int));
        o.counts = reinterpret_cast<unsigned int *>(base);
        o.crowdedCount = o.counts + padded + 2 * (parity & 1u);
        o.count = o.crowdedCount + 1;
        o.nextCounters = o.counts + padded + 2 * ((parity & 1u) ^ 1u);
        o.paddedBins = (unsigned int)padded;
        o.hostCount = mc->d_modeHint ? mc->d_modeHint + pfac::kHostPairs.value : nullptr;
        o.cursor = reinterpret_cast<unsigned int *>(base + counterBytes);
        o.crowded = reinterpret_cast<unsigned int *>(base + counterBytes + cursorBytes);
        o.posTmp = reinterpret_cast<unsigned int *>(base + fixed);
        o.idTmp = reinterpret_cast<int *>(base + fixed + perArray);
        o.posIn = o.posOut = reinterpret_cast<unsigned int *>(d_pos);
        o.idIn = o.idOut = d_ids;
        return PFAC_STATUS_SUCCESS;
    }
    hipError_t clearCounters() const { return hipMemsetAsync(o.counts, 0, counterBytes, 0); }
    hipError_t order(const PFAC_context *c) const
    {
        const unsigned int grid = gridFor(c, o.capacity);
        hipLaunchKernelGGL(pfac_order_count, dim3(grid), dim3(256), 0, 0, o);
        hipLaunchKernelGGL(pfac_order_offsets, dim3((o.bins + kOrderBlockBins - 1) / kOrderBlockBins), dim3(256), 0, 0, o);
        hipLaunchKernelGGL(pfac_order_scatter, dim3(grid), dim3(256), 0, 0, o);
        hipLaunchKernelGGL(pfac_order_rank, dim3(grid), dim3(256), 0, 0, o);
        return hipGetLastError();
    }
};

