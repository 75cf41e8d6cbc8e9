/*
 * scan_words.hip -- whole-word and delimiter-bounded matches (include/pfac_ext.h: PFACX_matchWords* / PFACX_wordsPairsFromDevice): the
 * occurrences whose neighbours in the input are not in a byte class W.
 *
 * Every pattern that starts at p is a prefix of the longest one L that starts there, so the occurrences at p are L's prefix chain (scan_all.hip).  They
 * share the byte in front of them, in[p - 1]; each has its own byte behind it, in[p + len].  The passes work on an ordered list of LONGEST pairs -- the
 * handle's pair scratch behind PFACX_allReduce, or a list of the caller's -- and look at the input again, at most 1 + chainLen bytes per pair:
 *   pfac_words_count     a thread per pair: in[p - 1] once, then the chain from the longest pattern down, in[p + len(q)] for each member q.  The value
 *                        of a pair is 0 / 1 in list mode (the walk stops at the first bounded member) and 0 .. chainLen in ALL mode; the block's total
 *                        goes to blockBase[block] (scan_passes.h: offsetsBlockTotal)
 *   pfac_array_scan      exclusive scan of the block totals (one block; 64-bit), the length of the list to mapped host memory
 *   pfac_words_write     the block's pairs again (offsetsOfBlock): each thread walks its chain once more and writes (id, p) for every bounded member into
 *                        consecutive slots; slots >= capacity are skipped (the caller learns the full length)
 *   pfac_host_done       the call's sequence number to mapped host memory (scan_passes.h: HostHandoff)
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
    const unsigned char *in;            /* the caller's bytes: never the folded copy */
    unsigned int n;
    const int *pairIds;                 /* the ordered longest pairs */
    const int *pairPos;
    size_t count;
    const pfac::Int2 *table;            /* [numIds + 1] {prefixPattern, chainLen} by id, or null: every chain is the pair itself */
    const int *patternLen;              /* [numIds + 1] by id */
    unsigned int numIds;
    unsigned int all;                   /* PFACX_WORDS_ALL: every bounded member, else the longest one */
    unsigned int cls[8];                /* W: byte b is in it iff bit b & 31 of cls[b >> 5] is set */
    size_t per;                         /* pairs per block: a multiple of kWordsBlock */
    unsigned long long *blockBase;      /* [blocks + 1]: block totals -> their exclusive prefix; [blocks] = the length of the list */
    int *ids;                           /* the caller's arrays: capacity entries each */
    int *pos;
    size_t capacity;
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

/* The bounded members of pair k's chain, longest first: emit(q, j) for the j-th of them; returns their number (list mode: 0 or 1) */
template <class Emit>
__device__ __forceinline__ unsigned int walkPair(const WordsArgs &a, const unsigned int *cls, size_t k, Emit emit)
{
    const int id = a.pairIds[k], p = a.pairPos[k];
    if ((unsigned int)id - 1u >= a.numIds || p < 0 || (unsigned int)p >= a.n) return 0u;
    if (p > 0 && inClassAt(a, cls, (unsigned int)p - 1u)) return 0u;
    int steps = a.table != nullptr ? a.table[id].y : 1;
    if (steps < 1) steps = 1;                                   /* an id the trie does not hold stands for itself alone */
    const unsigned int room = a.n - (unsigned int)p;
    unsigned int found = 0;
    int q = id;
    for (int s = 0; s < steps && (unsigned int)q - 1u < a.numIds; s++) {
        const int len = a.patternLen[q];
        if (len > 0 && (unsigned int)len <= room && !inClassAt(a, cls, (unsigned int)p + (unsigned int)len)) {
            emit(q, found);
            found++;
            if (!a.all) break;
        }
        q = a.table != nullptr ? a.table[q].x : 0;
    }
    return found;
}

__global__ __launch_bounds__(kWordsBlock) void pfac_words_count(WordsArgs a)
{
    __shared__ unsigned int cls[8];
    stageClass(a, cls);
    offsetsBlockTotal<kWordsBlock>(a.count, a.per, a.blockBase, [&](size_t k) -> unsigned long long { return walkPair(a, cls, k, [](int, unsigned int) {}); });
}

__global__ __launch_bounds__(kWordsBlock) void pfac_words_write(WordsArgs a)
{
    __shared__ unsigned int cls[8];
    stageClass(a, cls);
    offsetsOfBlock<kWordsBlock>(
        a.count, a.per, a.blockBase, [&](size_t k) -> unsigned long long { return walkPair(a, cls, k, [](int, unsigned int) {}); },
        [&](size_t k, unsigned long long before) {
            if (before >= a.capacity) return;
            const int p = a.pairPos[k];
            (void)walkPair(a, cls, k, [&](int q, unsigned int j) {
                if (before + j < a.capacity) {
                    a.ids[before + j] = q;
                    a.pos[before + j] = p;
                }
            });
        });
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
    a.pairIds = run->d_pairIds;
    a.pairPos = run->d_pairPos;
    a.count = run->count;
    a.table = static_cast<const pfac::Int2 *>(run->d_table);
    a.patternLen = run->d_patternLen;
    a.numIds = (unsigned int)run->numIds;
    a.all = run->all ? 1u : 0u;
    for (int k = 0; k < 8; k++) a.cls[k] = run->cls[k];
    a.ids = run->d_ids;
    a.pos = run->d_pos;
    a.capacity = run->capacity;
    const unsigned int blocks = offsetBlocks(c, a.count, kWordsBlock, a.per);
    const PFAC_status_t carved = carveScratch(c->scratch.words, [&](ScratchCarver &k) { a.blockBase = k.take<unsigned long long>((size_t)blocks + 1); });
    if (carved != PFAC_STATUS_SUCCESS) return carved;
    const HostHandoff list(c, pfac::kHostWordList);
    hipLaunchKernelGGL(pfac_words_count, dim3(blocks), dim3(kWordsBlock), 0, 0, a);
    hipLaunchKernelGGL(pfac_array_scan<unsigned long long>, dim3(1), dim3(1024), 0, 0, a.blockBase, blocks, a.blockBase + blocks,
                       reinterpret_cast<unsigned long long *>(list.d_value));
    if (a.capacity) hipLaunchKernelGGL(pfac_words_write, dim3(blocks), dim3(kWordsBlock), 0, 0, a);
    unsigned long long total = 0;
    if (!list.finish(&total, a.blockBase + blocks)) return PFAC_STATUS_INTERNAL_ERROR;
    *h_total = (size_t)total;
    return PFAC_STATUS_SUCCESS;
}

} /* extern "C" */
