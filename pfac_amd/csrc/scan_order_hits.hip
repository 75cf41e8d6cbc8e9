/*
 * scan_order_hits.hip -- hit lists in start order (include/pfac_ext.h: PFACX_orderHits*): a stable key sort of a list of up to four
 * int columns on the device, by (start) or by (start, id), both signed.
 *
 * The ordering passes of the compacted-output path (scan_order.inc) rank DISTINCT positions inside position bins; a hit list holds equal starts
 * and carries up to four columns, so this unit is a general least-significant-digit radix sort over (key, index) pairs of 8 bytes, 8 bits a pass.
 * The 64-bit key of entry k is (uint32)start[k] ^ 0x80000000 in the high word and, with PFACX_ORDER_TIES_BY_ID, (uint32)ids[k] ^ 0x80000000 in the
 * low word (else 0): unsigned order of the keys is the requested signed order.  A pair holds the 32-bit word of the key that the running passes
 * sort on and the incoming index of the entry.
 *
 *   hipMemsetAsync            the five probe words
 *   pfac_order_probe          grid-stride: the OR of all keys, the OR of all complemented keys (the AND, complemented: both start from zero) and
 *                             the number of descents, key[k] < key[k - 1]; a wave reduces, its first lane adds three atomics
 *   pfac_order_finish         the bits in which two keys differ (OR & ~AND) and the descents to the host (HostHandoff, kHostOrder)
 * No descent: the list is ordered, nothing is written but the identity into d_perm (pfac_order_iota), and no scratch beyond the probe words is taken.
 * Otherwise, for each of the eight digits whose bits differ, least significant first (a digit all keys agree on moves nothing):
 *   pfac_order_count<MODE>    block b owns tilesPer CONTIGUOUS tiles of kOrderTile entries and writes its 256 digit counts to counts[digit][b]
 *   pfac_block_scan<sum>      (scan_passes.h) the exclusive prefix of that table: digit-major, so offsets[d][b] is where block b's first key with
 *                             digit d goes -- behind every smaller digit and behind digit d of the blocks in front of it
 *   pfac_order_scatter<MODE>  the same blocks over the same tiles, in order.  A wave takes a contiguous quarter of the tile in eight rounds of 64.
 *                             Per key eight ballots give the lanes of the round with the same digit; the rank inside the round is the popcount of
 *                             that mask below the lane, and the lowest peer adds the mask's popcount to the wave's row of LDS counters, whose old
 *                             value is the rank of the round inside the wave.  Behind a barrier thread d prefixes digit d across the four rows in
 *                             wave order, on top of the block's running base of digit d; behind another every lane stores its pair at row[wave][d]
 *                             + its rank.  Tile order, wave order, round order and lane order are all the incoming order: the pass is stable.
 * MODE says where a pass reads: FRESH -- the first pass: key from the caller's column, index k, no pack launch --, PAIR -- the pair buffer --, SWITCH
 * -- the first pass over the start word behind passes over the id word: index from the pair buffer, key from start[index].  Passes alternate
 * between two pair buffers.  Behind the last pass:
 *   pfac_order_gather         per given column: temp[k] = column[index of pair k], then one device copy of temp over the column
 *   pfac_order_gather         once more without a column: d_perm[k] = index of pair k
 * Nothing of the caller's is written before the last pass has finished.
 *
 * NO BLOCK WAITS ON ANOTHER: no look-back, no flags, no grid barrier; the order between phases is the order of the launches, so a wrong count can
 * misplace a pair but cannot hang.
 * BOUNDS.  Column values are keys and nothing else.  Every index that reaches a load or a store is made here: an entry index k < n, a pair's index
 * (written by FRESH as k, copied from then on; clamped to n - 1 where it is used all the same), a scatter slot (checked against n), a counter
 * index digit < 256 and block < blocks.  A thread loads only below min(n, the end of its block's tiles).
 * SCRATCH of a call over n hits that needs a pass, with tiles = (n + 2047) / 2048, blocks <= min(tiles, 8 per compute unit):
 * 40 (probe) + 8 n + 8 n (pairs) + 4 n (column temp) + 4 x 256 x blocks (counts) + 4 x (256 x blocks + 1) (offsets), each part rounded up to 256;
 * a call that finds its list ordered takes the probe words alone.  LDS: 5 KiB.  No scratch memory, plain C++, vector stores and ordinary atomics.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_order_hits.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "pfac_ext.h"
#include "scan_passes.h"

namespace {

constexpr unsigned int kOrderThreads = 256;
constexpr unsigned int kOrderWaves = kOrderThreads / 64;
constexpr unsigned int kOrderRounds = 8;                                     /* rounds of 64 entries a wave takes of a tile */
constexpr unsigned int kOrderTile = kOrderThreads * kOrderRounds;            /* 2048 entries */
constexpr unsigned int kOrderWaveSpan = kOrderTile / kOrderWaves;            /* 512: the contiguous part of a tile one wave owns */
constexpr unsigned int kOrderBias = 0x80000000u;                             /* signed order as unsigned order */
static_assert(kOrderTile == PFACX_ORDER_TILE && kOrderThreads == PFACX_ORDER_THREADS, "pfac_module.h tells the tests where tiles, waves and rounds end");
static_assert(kOrderThreads == 256, "a thread per digit prefixes the rows");

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));                  /* a pair: x = the key word, y = the incoming index */

enum OrderMode { kFresh = 0, kPair = 1, kSwitch = 2 };

struct OrderArgs {
    const int *start, *ids;             /* the caller's key columns: read as keys, never as indices (ids: null without the ties flag) */
    unsigned int n;
    const int *col;                     /* FRESH, SWITCH: the column this pass takes its key word from */
    const u32x2 *in;                    /* PAIR, SWITCH */
    u32x2 *out;
    unsigned int shift;                 /* the digit: bits [shift, shift + 8) of the key word */
    unsigned int tilesPer, blocks;      /* tiles per block; the blocks of the count and scatter launches */
    unsigned int *counts;               /* [256][blocks] */
    unsigned int *offsets;              /* [256][blocks] + 1: their exclusive prefix */
    unsigned long long *probe;          /* OR, complemented AND, descents; then the two values of the hand-off */
};

__device__ __forceinline__ unsigned long long orderKey64(const OrderArgs &a, unsigned int k)
{
    const unsigned int lo = a.ids != nullptr ? (unsigned int)a.ids[k] ^ kOrderBias : 0u;
    return (unsigned long long)((unsigned int)a.start[k] ^ kOrderBias) << 32 | lo;
}

struct OpOr {
    template <class T> __device__ __forceinline__ T operator()(T x, T y) const { return x | y; }
};

__global__ __launch_bounds__(kOrderThreads) void pfac_order_probe(OrderArgs a)
{
    unsigned long long any = 0, none = 0, descents = 0;
    for (unsigned int k = blockIdx.x * kOrderThreads + threadIdx.x; k < a.n; k += gridDim.x * kOrderThreads) {
        const unsigned long long key = orderKey64(a, k);
        any |= key;
        none |= ~key;
        if (k != 0 && key < orderKey64(a, k - 1u)) descents++;
    }
    any = waveReduce(any, OpOr());
    none = waveReduce(none, OpOr());
    descents = waveReduce(descents, OpSum());
    if ((threadIdx.x & 63u) == 0) {
        atomicOr(&a.probe[0], any);
        atomicOr(&a.probe[1], none);
        if (descents != 0) atomicAdd(&a.probe[2], descents);
    }
}

__global__ void pfac_order_finish(unsigned long long *probe, unsigned long long *hostValue)
{
    const unsigned long long differ = probe[0] & probe[1], descents = probe[2];
    probe[3] = differ;
    probe[4] = descents;
    storeToHost(hostValue, differ, descents);
}

/* entry k of a pass: the key word the pass sorts on, and the incoming index */
template <int MODE>
__device__ __forceinline__ u32x2 orderLoad(const OrderArgs &a, unsigned int k)
{
    if constexpr (MODE == kFresh) {
        return u32x2{(unsigned int)a.col[k] ^ kOrderBias, k};
    } else if constexpr (MODE == kPair) {
        return a.in[k];
    } else {
        unsigned int idx = a.in[k].y;
        idx = idx < a.n ? idx : a.n - 1u;
        return u32x2{(unsigned int)a.col[idx] ^ kOrderBias, idx};
    }
}

/* the lanes of the wave that hold digit d, among those with `valid` (0 for a lane without) */
__device__ __forceinline__ unsigned long long digitPeers(unsigned int d, bool valid)
{
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (unsigned int b = 0; b < 8; b++) {
        const unsigned long long set = __ballot((d >> b) & 1u);
        peers &= ((d >> b) & 1u) ? set : ~set;
    }
    return valid ? peers : 0ull;
}

/* the block's entries [first, end): tilesPer whole tiles, cut at n */
__device__ __forceinline__ void orderRange(const OrderArgs &a, unsigned int &first, unsigned int &end)
{
    const unsigned long long lo = (unsigned long long)blockIdx.x * a.tilesPer * kOrderTile, hi = lo + (unsigned long long)a.tilesPer * kOrderTile;
    first = lo < a.n ? (unsigned int)lo : a.n;
    end = hi < a.n ? (unsigned int)hi : a.n;
}

template <int MODE>
__global__ __launch_bounds__(kOrderThreads) void pfac_order_count(OrderArgs a)
{
    __shared__ unsigned int rows[kOrderWaves][256];
    const unsigned int t = threadIdx.x, lane = t & 63u, wave = t >> 6;
#pragma unroll
    for (unsigned int w = 0; w < kOrderWaves; w++) rows[w][t] = 0;
    __syncthreads();
    unsigned int first, end;
    orderRange(a, first, end);
    volatile unsigned int *row = rows[wave];
    for (unsigned int k0 = first + wave * 64u; k0 < end; k0 += kOrderThreads) {            /* the same trips for every lane of a wave */
        const unsigned int k = k0 + lane;
        const bool valid = k < end;
        const unsigned int d = valid ? (orderLoad<MODE>(a, k).x >> a.shift) & 255u : 0u;
        const unsigned long long peers = digitPeers(d, valid);
        if (valid && (peers & ((1ull << lane) - 1ull)) == 0) row[d] = row[d] + (unsigned int)__popcll(peers);   /* the lowest peer; digits differ between peers groups */
    }
    __syncthreads();
    unsigned int total = 0;
#pragma unroll
    for (unsigned int w = 0; w < kOrderWaves; w++) total += rows[w][t];
    a.counts[(size_t)t * a.blocks + blockIdx.x] = total;
}

template <int MODE>
__global__ __launch_bounds__(kOrderThreads) void pfac_order_scatter(OrderArgs a)
{
    __shared__ unsigned int rows[kOrderWaves][256];
    __shared__ unsigned int digitBase[256];
    const unsigned int t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    unsigned int first, end;
    orderRange(a, first, end);
    digitBase[t] = a.offsets[(size_t)t * a.blocks + blockIdx.x];
    volatile unsigned int *row = rows[wave];
    for (unsigned int tile = first; tile < end; tile += kOrderTile) {                       /* the same trips for every thread of the block */
#pragma unroll
        for (unsigned int w = 0; w < kOrderWaves; w++) rows[w][t] = 0;
        __syncthreads();
        u32x2 pair[kOrderRounds];
        unsigned int rank[kOrderRounds];
#pragma unroll
        for (unsigned int r = 0; r < kOrderRounds; r++) {
            const unsigned int k = tile + wave * kOrderWaveSpan + r * 64u + lane;
            const bool valid = k < end;
            pair[r] = valid ? orderLoad<MODE>(a, k) : u32x2{0u, 0u};
            const unsigned int d = (pair[r].x >> a.shift) & 255u;
            const unsigned long long peers = digitPeers(d, valid);
            const unsigned int below = (unsigned int)__popcll(peers & ((1ull << lane) - 1ull));
            const unsigned int before = row[d];                                             /* of this digit in the wave's earlier rounds */
            __builtin_amdgcn_wave_barrier();
            if (valid && below == 0) row[d] = before + (unsigned int)__popcll(peers);
            __builtin_amdgcn_wave_barrier();
            rank[r] = before + below;
        }
        __syncthreads();
        {
            unsigned int run = digitBase[t];                                                /* thread t: digit t across the rows, in wave order */
#pragma unroll
            for (unsigned int w = 0; w < kOrderWaves; w++) {
                const unsigned int c = rows[w][t];
                rows[w][t] = run;
                run += c;
            }
            digitBase[t] = run;
        }
        __syncthreads();
#pragma unroll
        for (unsigned int r = 0; r < kOrderRounds; r++) {
            const unsigned int k = tile + wave * kOrderWaveSpan + r * 64u + lane;
            const unsigned int d = (pair[r].x >> a.shift) & 255u;
            const unsigned int at = row[d] + rank[r];
            if (k < end && at < a.n) a.out[at] = pair[r];
        }
        __syncthreads();                                                                    /* the rows are zeroed by the next trip */
    }
}

__global__ __launch_bounds__(kOrderThreads) void pfac_order_iota(int *perm, unsigned int n)
{
    for (unsigned int k = blockIdx.x * kOrderThreads + threadIdx.x; k < n; k += gridDim.x * kOrderThreads) perm[k] = (int)k;
}

/* temp[k] = col[index of pair k]; col == null: the index itself (d_perm) */
__global__ __launch_bounds__(kOrderThreads) void pfac_order_gather(const u32x2 *pairs, const int *col, int *out, unsigned int n)
{
    for (unsigned int k = blockIdx.x * kOrderThreads + threadIdx.x; k < n; k += gridDim.x * kOrderThreads) {
        unsigned int idx = pairs[k].y;
        idx = idx < n ? idx : n - 1u;
        out[k] = col != nullptr ? col[idx] : (int)idx;
    }
}

template <int MODE>
void orderPass(const OrderArgs &a)
{
    hipLaunchKernelGGL(pfac_order_count<MODE>, dim3(a.blocks), dim3(kOrderThreads), 0, 0, a);
    blockScan<OpSum>({{a.counts}, {a.offsets}}, 256u * a.blocks, nullptr, nullptr);
    hipLaunchKernelGGL(pfac_order_scatter<MODE>, dim3(a.blocks), dim3(kOrderThreads), 0, 0, a);
}

} // namespace

extern "C" {

PFAC_status_t PFACX_orderRun(PFAC_handle_t handle, const PFACX_orderRun_t *run, int *h_wasOrdered)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!run || !h_wasOrdered || !run->d_start || run->numHits == 0 || run->numHits > (size_t)0x7fffffff || (run->flags & ~PFACX_ORDER_TIES_BY_ID) ||
        ((run->flags & PFACX_ORDER_TIES_BY_ID) && !run->d_ids))
        return PFAC_STATUS_INVALID_PARAMETER;
    PFAC_context *c = handle;
    const bool ties = (run->flags & PFACX_ORDER_TIES_BY_ID) != 0;

    OrderArgs a{};
    a.start = run->d_start;
    a.ids = ties ? run->d_ids : nullptr;
    a.n = (unsigned int)run->numHits;
    const unsigned int tiles = (a.n + kOrderTile - 1u) / kOrderTile;
    const unsigned int grid = gridFor(c, (size_t)tiles * 256);                 /* min(tiles, eight per compute unit) */
    a.tilesPer = (tiles + grid - 1u) / grid;
    a.blocks = (tiles + a.tilesPer - 1u) / a.tilesPer;
    const size_t table = (size_t)256 * a.blocks;

    /* the probe, in the probe words alone */
    PFAC_status_t carved = carveScratch(c->scratch.order, [&](ScratchCarver &k) { a.probe = k.take<unsigned long long>(5); });
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    if (hipMemsetAsync(a.probe, 0, 5 * sizeof(unsigned long long), nullptr) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
    hipLaunchKernelGGL(pfac_order_probe, dim3(gridFor(c, a.n)), dim3(kOrderThreads), 0, 0, a);
    unsigned long long probed[2] = {0, 0};
    {
        const HostHandoff values(c, pfac::kHostOrder);
        hipLaunchKernelGGL(pfac_order_finish, dim3(1), dim3(1), 0, 0, a.probe, reinterpret_cast<unsigned long long *>(values.d_value));
        if (!values.finish(probed, a.probe + 3, a.probe + 4)) return PFAC_STATUS_INTERNAL_ERROR;
    }
    const unsigned long long differ = probed[0];
    if (probed[1] == 0) {                                                      /* no descent: ordered as it stands */
        if (run->d_perm) {
            hipLaunchKernelGGL(pfac_order_iota, dim3(gridFor(c, a.n)), dim3(kOrderThreads), 0, 0, run->d_perm, a.n);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
        }
        *h_wasOrdered = 1;
        return PFAC_STATUS_SUCCESS;
    }
    if (probed[1] >= a.n || differ == 0) return PFAC_STATUS_INTERNAL_ERROR;    /* a descent needs two keys that differ */

    u32x2 *buffer[2] = {nullptr, nullptr};
    int *temp = nullptr;
    carved = carveScratch(c->scratch.order, [&](ScratchCarver &k) {           /* (a buffer that grows loses the probe words: they are read) */
        a.probe = k.take<unsigned long long>(5);
        buffer[0] = k.take<u32x2>(a.n);
        buffer[1] = k.take<u32x2>(a.n);
        temp = k.take<int>(a.n);
        a.counts = k.take<unsigned int>(table);
        a.offsets = k.take<unsigned int>(table + 1);
    });
    if (carved != PFAC_STATUS_SUCCESS) return carved;

    int have = -1;                                                             /* the buffer that holds the pairs; none yet */
    unsigned int word = 0;                                                     /* the key word they hold: 0 the id word, 1 the start word */
    for (unsigned int digit = 0; digit < 8; digit++) {
        if (((differ >> (8u * digit)) & 0xFFull) == 0) continue;               /* all keys agree here */
        const unsigned int w = digit / 4u;
        a.shift = 8u * (digit & 3u);
        a.col = w ? run->d_start : run->d_ids;
        a.in = have < 0 ? nullptr : buffer[have];
        a.out = buffer[have < 0 ? 0 : 1 - have];
        if (have < 0) orderPass<kFresh>(a);
        else if (w != word) orderPass<kSwitch>(a);
        else orderPass<kPair>(a);
        have = have < 0 ? 0 : 1 - have;
        word = w;
    }
    if (have < 0) return PFAC_STATUS_INTERNAL_ERROR;

    const unsigned int g = gridFor(c, a.n);
    for (int *col : {run->d_start, run->d_ids, run->d_end, run->d_aux}) {
        if (!col) continue;
        hipLaunchKernelGGL(pfac_order_gather, dim3(g), dim3(kOrderThreads), 0, 0, buffer[have], col, temp, a.n);
        if (hipMemcpyAsync(col, temp, (size_t)a.n * sizeof(int), hipMemcpyDeviceToDevice, nullptr) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
    }
    if (run->d_perm) hipLaunchKernelGGL(pfac_order_gather, dim3(g), dim3(kOrderThreads), 0, 0, buffer[have], nullptr, run->d_perm, a.n);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) return PFAC_STATUS_INTERNAL_ERROR;
    *h_wasOrdered = 0;
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
