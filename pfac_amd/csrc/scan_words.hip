/*
 * scan_words.hip -- whole-word and delimiter-bounded matches (include/pfac_ext.h: PFACX_matchWords* / PFACX_wordsPairsFromDevice): the
 * occurrences whose neighbours in the input are not in a byte class W.
 *
 * Every pattern that starts at p is a prefix of the longest one L that starts there, so the occurrences at p are L's prefix chain (scan_all.hip).  They
 * share the byte in front of them, in[p - 1]; each has its own byte behind it, in[p + len].  The passes work on an ordered list of LONGEST pairs -- the
 * handle's pair scratch behind PFACX_allReduce, or a list of the caller's -- and look at the input again, at most 1 + chainLen bytes per pair:
 *   pfac_words_count     a thread per pair: in[p - 1] once, then the chain from the longest pattern down, in[p + len(q)] for each member q.  The value
 *                        of a pair is 0 / 1 in list mode (the walk stops at the first bounded member) and 0 .. chainLen in ALL mode; the block's total
 *                        goes to blockBase[block] (scan_passes.h: expandCount)
 *   pfac_array_scan      exclusive scan of the block totals (one block; 64-bit), the length of the list to mapped host memory
 *   pfac_words_write     the block's pairs again (expandWrite): each thread walks its chain once more and hands every bounded member to the frame, which
 *                        writes (id, p) into consecutive slots; slots >= capacity are skipped (the caller learns the full length)
 *   pfac_host_done       the call's sequence number to mapped host memory (scan_passes.h: HostHandoff)
 * The walk along the chain (forEachChainMember), both passes, the capacity-checked store and the launches (expandPasses) are the expansion frame of
 * scan_passes.h, shared with scan_all.hip and scan_groups.hip; this unit's own is the test of a member (walkPair).
 * The class is 256 bits; a block keeps its eight words in LDS (a kernel-argument array indexed by a lane's byte would go to scratch).  Every index
 * into the input is checked against [0, n) before the load; an id outside [1, F] is a pair that counts nothing, a chain member that does not lie
 * inside the input is not kept, and a walk ends after chainLen steps whatever the table says: a caller's list cannot make a pass read or write outside
 * the buffers.  SCRATCH: 8 (blocks + 1) bytes rounded up to 256 (DeviceScratch::words), blocks = one per 256 pairs, eight per compute unit at most.
 * Plain C++ and vector stores only.
 */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "scan_words.hip is written for gfx950 (CDNA4): wave64"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfac_context.h"
#include "scan_passes.h"

namespace {

constexpr unsigned int kWordsBlock = 256;

struct WordsArgs {
    ExpandFrame f;                      /* the pairs, the chain table, PFACX_WORDS_ALL, the block cut, the caller's arrays (scan_passes.h) */
    const unsigned char *in;            /* the caller's bytes: never the folded copy */
    unsigned int n;
    const int *patternLen;              /* [numIds + 1] by id */
    unsigned int cls[8];                /* W: byte b is in it iff bit b & 31 of cls[b >> 5] is set */
};

/* W into the block's LDS: constant indices into the argument, one thread */
__device__ __forceinline__ void stageClass(const WordsArgs &a, unsigned int *cls)
{
    if (threadIdx.x == 0) {
#pragma unroll
        for (unsigned int k = 0; k < 8; k++) cls[k] = a.cls[k];
    }
    __syncthreads();
}

/* is in[i] a byte of W?  false outside the input: the ends of the buffer bound like a byte that is not in W */
__device__ __forceinline__ bool inClassAt(const WordsArgs &a, const unsigned int *cls, unsigned int i)
{
    if (i >= a.n) return false;
    const unsigned int b = a.in[i];
    return (cls[b >> 5] >> (b & 31u)) & 1u;
}

/* The bounded members of pair k's chain, longest first (scan_passes.h: forEachChainMember): emit(q) for each of them; returns their number
 * (list mode: 0 or 1) */
template <class Emit>
__device__ __forceinline__ unsigned int walkPair(const WordsArgs &a, const unsigned int *cls, size_t k, Emit emit)
{
    const int id = a.f.pairIds[k], p = a.f.pairPos[k];
    if (p < 0 || (unsigned int)p >= a.n) return 0u;
    if (p > 0 && inClassAt(a, cls, (unsigned int)p - 1u)) return 0u;
    const unsigned int room = a.n - (unsigned int)p;
    unsigned int found = 0;
    forEachChainMember(a.f.table, a.f.numIds, id, [&](int q) {
        const int len = a.patternLen[q];
        if (len <= 0 || (unsigned int)len > room || inClassAt(a, cls, (unsigned int)p + (unsigned int)len)) return true;
        emit(q);
        found++;
        return a.f.all != 0u;
    });
    return found;
}

__global__ __launch_bounds__(kWordsBlock) void pfac_words_count(WordsArgs a)
{
    __shared__ unsigned int cls[8];
    stageClass(a, cls);
    expandCount<kWordsBlock>(a.f, [&](size_t k) -> unsigned long long { return walkPair(a, cls, k, [](int) {}); });
}

__global__ __launch_bounds__(kWordsBlock) void pfac_words_write(WordsArgs a)
{
    __shared__ unsigned int cls[8];
    stageClass(a, cls);
    expandWrite<kWordsBlock>(
        a.f, [&](size_t k) -> unsigned long long { return walkPair(a, cls, k, [](int) {}); },
        [&](size_t k, auto emit) { (void)walkPair(a, cls, k, emit); });
}

} // namespace

extern "C" {

PFAC_status_t PFACX_wordsRun(PFAC_handle_t handle, const PFACX_wordsRun_t *run, size_t *h_total)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!run || !h_total || !run->d_input || run->size == 0 || run->size > (size_t)0x7fffffff || !run->d_patternLen || run->numIds > (size_t)0x7fffffff ||
        run->count > (size_t)0x7fffffff || (run->count && (!run->d_pairIds || !run->d_pairPos)) || (run->capacity && (!run->d_ids || !run->d_pos)))
        return PFAC_STATUS_INVALID_PARAMETER;
    *h_total = 0;
    if (run->count == 0) return PFAC_STATUS_SUCCESS;
    PFAC_context *c = handle;
    WordsArgs a{};
    a.in = reinterpret_cast<const unsigned char *>(run->d_input);
    a.n = (unsigned int)run->size;
    a.patternLen = run->d_patternLen;
    for (int k = 0; k < 8; k++) a.cls[k] = run->cls[k];
    a.f = ExpandFrame{run->d_pairIds, run->d_pairPos, run->count, static_cast<const pfac::Int2 *>(run->d_table), (unsigned int)run->numIds,
                      run->all ? 1u : 0u, 0, nullptr, run->d_ids, run->d_pos, run->capacity};
    return expandPasses(c, c->scratch.words, pfac::kHostWordList, a, pfac_words_count, pfac_words_write, kWordsBlock, a.f.capacity != 0, h_total);
}

} /* extern "C" */
