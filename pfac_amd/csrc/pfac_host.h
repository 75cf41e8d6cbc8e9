/*
 * pfac_host.h -- internal declarations of the host side of libpfac.so.
 */
#ifndef PFAC_HOST_H_
#define PFAC_HOST_H_

#include <algorithm>
#include <memory>
#include <new>
#include <optional>
#include <string>
#include <unordered_map>

#include "pfac_context.h"

namespace pfac {

/* pattern_compiler.cpp */
PFAC_status_t compilePatternFile(const char *filename, Automaton &fa, unsigned int flags = 0);
PFAC_status_t compilePatternBytes(std::vector<unsigned char> bytes, Automaton &fa, unsigned int flags = 0);   /* flags: PFACX_READ_* */
void buildInitialRow(const Automaton &fa, std::vector<int> &row);
void buildPrefixPatterns(Automaton &fa);                    /* fa.prefixPattern / chainLen / maxChain from the trie */
void buildFilter(const Automaton &fa, Filter &f);
void buildReduceFilter(const Automaton &fa, Filter &f);     /* gram1 + prefix4 alone (buildFilter calls it; a compiled set is loaded without them) */

/* tables.cpp */
PFAC_status_t buildDenseTable(const Automaton &fa, std::vector<int> &dense);
PFAC_status_t buildHashTable(const Automaton &fa, std::vector<Int2> &rowPtr,
                             std::vector<Int2> &valPtr);

PFAC_status_t buildChainedHashTable(const Automaton &fa, std::vector<ChainSlot> &slots, int &jumpLog2, bool narrow = false);

/* cpu_engine.cpp: PFAC_PLATFORM_CPU / PFAC_PLATFORM_CPU_OMP */
PFAC_status_t matchOnCpu(const PFAC_context *ctx, const unsigned char *in, size_t n, int *out,
                         bool useOpenMP);

} // namespace pfac

/* ---- internals of libpfac.so shared by pfac_api.cpp, host_pipeline.cpp, multi_gpu.cpp, compiled_set.cpp ---- */
#include <hip/hip_runtime_api.h>
namespace pfac_internal {

/* positions per piece of the pipelined PFAC_matchFromHost: 32 Mi positions = 32 MiB up, 128 MiB down */
constexpr size_t kHostPiece = size_t(32) << 20;

/* pfac_api.cpp */
void freeTables(PFAC_context *c);
void freeHostStage(PFAC_context *c);                  /* the staging buffers of the host calls with their streams and events */
void freeResources(PFAC_context *c);
PFAC_status_t bindTable(PFAC_context *c);
/* the end of every reader of a pattern set (the caller holds both locks; c->fa is compiled and checked): the set is ready, its tables are
 * built and uploaded -- or the handle is left empty */
PFAC_status_t bindCompiledSet(PFAC_context *c);
void correctTextureMode(PFAC_context *c);
PFAC_status_t prepareCpuPlatformLocked(PFAC_context *c);                                        /* the caller holds c->lock */
/* ... has called the above; any number of threads.  *generation (may be null): c->setGeneration, read in the section that reads the tables */
PFAC_status_t matchHostOnCpuPlatformPrepared(PFAC_context *c, const char *in, size_t n, int *out, unsigned long long *generation = nullptr);
/* the longest match at positions [0, owned) of `readable` >= owned host bytes (the rest read-ahead only) as (id, position + posShift) pairs in position
 * order; ids/pos hold `readable` entries at least; any platform: the CPU matcher into ids, compacted in place, or the pipelined path of the GPU
 * platform (LIB_NOT_EXIST without a device or a module).  The caller holds c->lock */
PFAC_status_t hostLongestPairsLocked(PFAC_context *c, char *in, size_t owned, size_t readable, int posShift, int *ids, int *pos, int *count);
/* ... of a whole buffer, for a caller without the lock: held for the whole call on the GPU platform, on the CPU platforms only while the tables are
 * prepared -- several threads match there side by side.  *generation (may be null): the setGeneration of the set that was scanned, read while the scan holds it still */
PFAC_status_t hostLongestPairs(PFAC_context *c, char *in, size_t size, int *ids, int *pos, int *count, unsigned long long *generation);
/* The compiled set (c->fa) held still for a scope: tablesInUse shared, which whoever replaces the set holds exclusively.  status(): SUCCESS iff a set
 * is loaded and -- where a generation is given -- it is still the one with that number, else PATTERNS_NOT_READY.  Never held across a scan: the CPU
 * platforms' first match takes tablesInUse exclusively (ensureHostRefTable) */
class SetPin {
public:
    explicit SetPin(PFAC_context *c) : held_(c->tablesInUse), ok_(c->isPatternsReady) {}
    SetPin(PFAC_context *c, unsigned long long generation) : held_(c->tablesInUse), ok_(c->isPatternsReady && c->setGeneration == generation) {}
    PFAC_status_t status() const { return ok_ ? PFAC_STATUS_SUCCESS : PFAC_STATUS_PATTERNS_NOT_READY; }
private:
    std::shared_lock<std::shared_mutex> held_;
    bool ok_;
};
/* the two steps of a host form whose post-pass reads c->fa: the longest pairs of the buffer, then the pin on the set they came from */
struct PinnedPairs {
    PinnedPairs(PFAC_context *c, char *in, size_t size, int *ids, int *pos) : status(hostLongestPairs(c, in, size, ids, pos, &count, &generation))
    { if (status == PFAC_STATUS_SUCCESS) status = pin.emplace(c, generation).status(); }
    static constexpr bool needsModule = false;        /* scanForm: the GPU platform answers LIB_NOT_EXIST from inside the scan */
    int count = 0;
    unsigned long long generation = 0;
    PFAC_status_t status;                     /* (declared behind what its initialiser writes) */
    std::optional<SetPin> pin;
};
/* what most calls that need a pattern set check first, before they hold a lock: the handle, a loaded set, no null among the pointers they require */
inline PFAC_status_t checkSetAndPointers(PFAC_context *c, std::initializer_list<const void *> required)
{
    if (!c) return PFAC_STATUS_INVALID_HANDLE;
    if (SetPin(c).status() != PFAC_STATUS_SUCCESS) return PFAC_STATUS_PATTERNS_NOT_READY;
    for (const void *p : required)
        if (!p) return PFAC_STATUS_INVALID_PARAMETER;
    return PFAC_STATUS_SUCCESS;
}
/* positions, counts and lengths are ints on the device and in the callers' arrays */
constexpr size_t kMaxInt = 0x7fffffff;
/* what the rules, count-batch and groups calls refuse: a size or a number of segments from here on */
constexpr size_t kTwoGiB = size_t(1) << 31;
/* nothing to launch with: LIB_NOT_EXIST of every device form, and of a host form on the GPU platform */
inline bool lacksModule(const PFAC_context *c) { return !c->hasDevice || !c->module; }
inline bool hostLacksModule(const PFAC_context *c) { return c->platform == PFAC_PLATFORM_GPU && lacksModule(c); }
/* the status of a call whose full list has `total` entries */
inline PFAC_status_t truncatedIf(unsigned long long total, size_t capacity) { return total > capacity ? PFACX_STATUS_OUTPUT_TRUNCATED : PFAC_STATUS_SUCCESS; }
/* The cuts of PFACX_split* on the host (split_api.cpp, locate_api.cpp).  ByteClass (pfac_context.h): a caller's class, {'\n'} for a null h_class;
 * inClass: byte b is in the class; isCut: position c of [1, n - 1] is a cut, given a = (in[c - 1] is in the class) and b = (in[c] is) -- the four
 * flag combinations of the header in one place */
using pfac::ByteClass;
inline bool inClass(const unsigned int *cls, unsigned char b) { return (cls[b >> 5] >> (b & 31u)) & 1u; }
inline bool isCut(unsigned int flags, bool a, bool b)
{
    return (flags & PFACX_SPLIT_RUNS) ? ((flags & PFACX_SPLIT_BEFORE) ? b && !a : a && !b) : ((flags & PFACX_SPLIT_BEFORE) ? b : a);
}
/* the pair temporaries of a host form in one allocation: numIds ids, then numPos positions; not initialised: a page nothing writes costs nothing */
struct HostPairs {
    HostPairs(size_t numIds, size_t numPos) : mem(new (std::nothrow) int[numIds + numPos + 1]), ids(mem.get()), pos(mem ? mem.get() + numIds : nullptr) {}
    explicit operator bool() const { return mem != nullptr; }
    std::unique_ptr<int[]> mem;
    int *const ids, *const pos;
};
/* f(q) for the patterns that occur where pattern id is the longest -- id, then its chain of prefix patterns (Automaton::prefixPattern): at most
 * chainLen[id] of them (one for an id that is not in the trie), none for an id outside [1, numPatterns]; ends at such an id, or where f returns false */
template <class F>
inline void forEachChainMember(const pfac::Automaton &fa, int id, F f)
{
    if (id < 1 || id > fa.numPatterns) return;
    const int steps = fa.chainLen[(size_t)id] > 1 ? fa.chainLen[(size_t)id] : 1;
    for (int k = 0, q = id; k < steps && q >= 1 && q <= fa.numPatterns && f(q); k++) q = fa.prefixPattern[(size_t)q];
}
/* the length of pattern id, 0 for an id the set does not have */
inline size_t patternLenOf(const pfac::Automaton &fa, int id) { return id > 0 && (size_t)id < fa.patternLen.size() ? (size_t)fa.patternLen[(size_t)id] : 0; }
/* What a caller opens on a handle and closes again: the common head of PFACX_stream_s, PFACX_flows_s, PFACX_rules_s, PFACX_groups_s and
 * PFACX_flowRules_s, and what PFAC_context::objects holds.  A kind's destructor is the one place that gives its device memory back, deviceBytes()
 * what PFACX_getInfo counts of it (deviceTableBytes); a kind with several device buffers (a rule set, a flow-rule set) lists them ONCE, in a
 * forEachDeviceBuffer(self, f) of its own from which both follow, as DeviceTables::forEach does.  One is only ever built by adoptNew */
struct HandleObject {
    PFAC_context *handle = nullptr;           /* the handle that holds it; null while it is being set up */
    unsigned long long generation = 0;        /* PFAC_context::setGeneration when it was opened (a stream, a flow set: or last reset as a whole) */
    virtual ~HandleObject() = default;
    virtual size_t deviceBytes() const = 0;
};
/* host vectors into their device buffers, (buffer, vector) pair by pair, up to the first that fails: the caller releases what went up */
inline PFAC_status_t uploadAll() { return PFAC_STATUS_SUCCESS; }
template <class T, class... Rest>
inline PFAC_status_t uploadAll(pfac::DeviceBuffer<T> &to, const std::vector<T> &from, Rest &...rest)
{
    const PFAC_status_t st = to.upload(from.data(), from.size());
    return st != PFAC_STATUS_SUCCESS ? st : uploadAll(rest...);
}
/* What every PFACX_...Open ends with, behind its argument checks (*out is null): a new T that the handle holds, stamped with the set's generation.
 * Under c->lock: PATTERNS_NOT_READY without a set, then setUp(T &) -- it may read c->fa, refuse with a status or throw bad_alloc.  Whatever
 * fails, the object is gone and *out stays null */
template <class T, class SetUp>
PFAC_status_t adoptNew(PFAC_context *c, T **out, SetUp setUp)
{
    std::unique_ptr<T> obj(new (std::nothrow) T());
    if (!obj) return PFAC_STATUS_ALLOC_FAILED;
    std::lock_guard<std::mutex> guard(c->lock);
    if (!c->isPatternsReady) return PFAC_STATUS_PATTERNS_NOT_READY;
    try {
        const PFAC_status_t st = setUp(*obj);
        if (st != PFAC_STATUS_SUCCESS) return st;
        c->objects.push_back(obj.get());
    } catch (const std::bad_alloc &) { return PFAC_STATUS_ALLOC_FAILED; }
    obj->handle = c;
    obj->generation = c->setGeneration;
    *out = obj.release();
    return PFAC_STATUS_SUCCESS;
}
/* pfac_api.cpp: every PFACX_...Close -- INVALID_HANDLE for null, for an object no handle holds, for one its handle does not hold (any more);
 * the object is destroyed, its device memory with it, while the handle's lock is held */
PFAC_status_t closeObject(HandleObject *obj);
/* what the calls on such an object check first (the caller holds c->lock: the set cannot change between this check and the end of the call):
 * the stream, flows, rules and groups calls alike */
inline PFAC_status_t checkSetGeneration(const PFAC_context *c, unsigned long long generation)
{
    if (generation != c->setGeneration) return PFAC_STATUS_INVALID_PARAMETER;     /* another pattern set since: PFACX_streamReset / PFACX_flowsReset; a rule set or a group table is opened anew */
    if (!c->isPatternsReady) return PFAC_STATUS_PATTERNS_NOT_READY;
    return PFAC_STATUS_SUCCESS;
}
inline size_t up256(size_t n) { return (n + 255) & ~size_t(255); }
/* do [a, a + na) and [b, b + nb) share a byte? */
inline bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return na != 0 && nb != 0 && x < y + nb && y < x + na;
}
/* host_pipeline.cpp: the caller holds c->lock */
PFAC_status_t prepareHostPath(PFAC_context *c, size_t maxBytes);
PFAC_status_t matchDeviceLocked(PFAC_context *c, char *d_inputString, size_t size, int *d_matched_result);
PFAC_status_t matchHostOnGpu(PFAC_context *c, char *h_inputString, size_t owned, size_t readable, int *h_matched_result);
PFAC_status_t matchHostReduceOnGpu(PFAC_context *c, char *h_inputString, size_t size, size_t readable, size_t posBase, int *h_matched_result, int *h_pos, int *h_num_matched);
/* caseless sets (PFACX_READ_NOCASE), the fold where input enters the library; the caller holds c->lock.  foldDeviceInput: the caller's
 * device bytes into the handle's fold scratch, *d_use = what the scan reads (d_in itself for a case-sensitive handle: no launch, no
 * scratch).  foldStaged: a staging piece in place, on the default stream behind its upload (nothing for a case-sensitive handle) */
PFAC_status_t foldDeviceInput(PFAC_context *c, char *d_in, size_t size, char **d_use);
PFAC_status_t foldStaged(PFAC_context *c, char *d_piece, size_t size);
/* the locked prologue of a device call that scans: the texture mode resolved, the input folded, the perf mode as the `hashed` argument of the module's
 * entry points (the caller holds c->lock and has checked hasDevice and module) */
struct DeviceScan { char *d_scan; int hashed; };
inline PFAC_status_t beginDeviceScan(PFAC_context *c, char *d_input, size_t size, DeviceScan *s)
{
    correctTextureMode(c);
    s->hashed = c->perfMode == PFAC_TIME_DRIVEN ? 0 : 1;
    return foldDeviceInput(c, d_input, size, &s->d_scan);
}
/* the compacted-output scan of the handle's perf mode over n device bytes, its pairs in position order or -- the ordering launches not paid for --
 * in any (the caller holds c->lock).  The one place on the host side that sets c->reduceUnordered (the module's: scan_passes.h compactedScan); the
 * handle's own setting is put back */
inline PFAC_status_t reduceOnDevice(PFAC_context *c, char *d_in, size_t n, int *d_ids, int *d_pos, bool ordered, int *h_count)
{
    PFAC_reduce_kernel_protoType fn = c->perfMode == PFAC_TIME_DRIVEN ? c->reduce_kernel_ptr : c->reduce_inplace_kernel_ptr;
    const bool wasUnordered = c->reduceUnordered;
    c->reduceUnordered = !ordered;
    const PFAC_status_t st = fn(c, reinterpret_cast<int *>(d_in), (int)n, d_ids, d_pos, h_count, nullptr, nullptr);
    c->reduceUnordered = wasUnordered;
    return st;
}
/* the ordered longest pairs of a device buffer with c->lock held, as PinnedPairs has those of a host buffer with the set pinned */
struct DevicePairs {
    DevicePairs(PFAC_context *c, char *d_input, size_t size, int *d_ids, int *d_pos) : guard(c->lock)
    {
        DeviceScan scan;                                                   /* a caseless set: the scan reads the folded copy, a post-pass the caller's bytes */
        status = beginDeviceScan(c, d_input, size, &scan);
        if (status == PFAC_STATUS_SUCCESS) status = reduceOnDevice(c, scan.d_scan, size, d_ids, d_pos, true, &count);
    }
    static constexpr bool needsModule = true;
    std::lock_guard<std::mutex> guard;
    int count = 0;
    PFAC_status_t status = PFAC_STATUS_SUCCESS;
};
/* The frame of a scan form with a post-pass over its pairs (PFACX_matchLocated*, PFACX_matchCaptured*), Pairs = DevicePairs: the device form, or
 * PinnedPairs: the host form.  The checks of PFAC_matchFromDeviceReduce in its order -- the handle, a loaded set, the pointers and `restOk` (what
 * the call checks of its own outputs and flags), size == 0, for the device form the module, size > kMaxInt --, then the pairs into ids / pos and
 * their number to *h_num_matched; post(kept) over the first kept = min(count, capacity) > 0 of them while Pairs holds the lock or the pin, its
 * status returned where it fails; OUTPUT_TRUNCATED where count > capacity */
template <class Pairs, class Post>
inline PFAC_status_t scanForm(PFAC_context *c, char *input, size_t size, int *ids, int *pos, bool restOk, size_t capacity, int *h_num_matched,
                              Post post)
{
    if (!c) return PFAC_STATUS_INVALID_HANDLE;
    if (!c->isPatternsReady) return PFAC_STATUS_PATTERNS_NOT_READY;
    if (!input || !ids || !pos || !h_num_matched || !restOk) return PFAC_STATUS_INVALID_PARAMETER;
    if (size == 0) { *h_num_matched = 0; return PFAC_STATUS_SUCCESS; }
    if (Pairs::needsModule && lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    if (size > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    const Pairs pairs(c, input, size, ids, pos);
    if (pairs.status != PFAC_STATUS_SUCCESS) return pairs.status;
    if (pairs.count < 0 || (size_t)pairs.count > size) return PFAC_STATUS_INTERNAL_ERROR;
    *h_num_matched = pairs.count;
    const size_t kept = (size_t)pairs.count < capacity ? (size_t)pairs.count : capacity;
    const PFAC_status_t st = kept ? post(kept) : PFAC_STATUS_SUCCESS;
    return st != PFAC_STATUS_SUCCESS ? st : truncatedIf((unsigned long long)pairs.count, capacity);
}
/* the non-zero results of the first `owned` entries of a full result vector as (id, position + posShift) pairs; ids may be the vector
 * itself (pair z comes from an entry at or behind z).  Returns the number of pairs */
inline int compactPairs(const int *results, size_t owned, int posShift, int *ids, int *pos)
{
    int z = 0;
    for (size_t i = 0; i < owned; i++) {
        const int m = results[i];
        if (m > 0) { ids[z] = m; pos[z] = (int)i + posShift; z++; }
    }
    return z;
}
/* stream_api.cpp: what the stream and the flows calls share (the caller holds c->lock).  streamSplitOf: how a piece of `size` bytes splits the work of a
 * stream that carries `carried` bytes -- of the pending and the piece's positions the first seam + owned are final, `seam` of them carried.
 * hostPiece: one host-fed piece (or, size == 0 and flush: the stream's end) of a stream whose carry is carry[0, carried): the seam
 * [carry | head of the piece], in room of its own, and the piece's final positions through hostLongestPairsLocked; the pairs go to ids / pos
 * (room: size + M - 1), their number to *count, the stream's next carry to `next`.  Nothing of the stream changes: the caller moves it on when its
 * whole call has succeeded */
struct StreamSplit { size_t seam, owned; };
StreamSplit streamSplitOf(size_t carried, size_t size, size_t M);
PFAC_status_t hostPiece(PFAC_context *c, const unsigned char *carry, size_t carried, char *piece, size_t size, bool flush, int *ids, int *pos,
                        std::vector<unsigned char> &next, int *count);
/* batch_api.cpp: offsets[0] == 0, offsets[n] == size, never decreasing */
bool batchOffsetsValid(const size_t *offsets, size_t numSegments, size_t size);
/* batch_api.cpp: the batch calls (PFACX_matchBatch*) behind their argument checks; the caller holds c->lock */
PFAC_status_t ensurePatternLen(PFAC_context *c);            /* the device copy of fa.patternLen the batch fix-ups read */
PFAC_status_t matchBatchDeviceLocked(PFAC_context *c, char *d_input, size_t size, const size_t *d_offsets, size_t numSegments, int *d_matched_result);
/* batch_api.cpp: the ordered longest pairs of a batch on the device; the caller holds c->lock.
 * batchReduceLocked: behind beginDeviceScan, over the bytes the scan reads.  The compacted scan WITH its ordering launches into d_ids / d_pos
 * (`size` entries each) and, with offsets, the batch fix-up behind it (scan_batch.hip): no pair runs from one segment into the next, the first
 * pair of each segment to d_segFirstPairs[numSegments + 1]; the fix-up's pattern lengths are uploaded here.  d_offsets null: one segment, no
 * fix-up, nothing written to d_segFirstPairs.
 * scratchBatchPairs: the same from the caller's input into the handle's pair scratch -- DeviceScratch::allPairs, one allocation of 2 size
 * entries, the ids in its first half and the positions in its second; DeviceScratch::allSegFirst with offsets only -- behind beginDeviceScan:
 * what every call that works on "the pairs of each segment" starts with */
PFAC_status_t batchReduceLocked(PFAC_context *c, char *d_scan, size_t size, const size_t *d_offsets, size_t numSegments, int *d_ids, int *d_pos,
                                int *d_segFirstPairs, int *h_count);
struct BatchPairs {
    int *ids, *pos;                           /* `count` pairs in position order */
    size_t count;
    const int *segFirstPairs;                 /* [numSegments + 1]; null without offsets */
    char *d_scan;                             /* the bytes that were scanned: the input, or its fold for a caseless set */
};
PFAC_status_t scratchBatchPairs(PFAC_context *c, char *d_input, size_t size, const size_t *d_offsets, size_t numSegments, BatchPairs *out);
/* nothing to do on the device: d_segFirst[numSegments + 1] and d_segGroups[numSegments] zeroed, each where given */
PFAC_status_t zeroSegmentArrays(size_t *d_segFirst, unsigned long long *d_segGroups, size_t numSegments);
/* batch_api.cpp: the two steps of a batch host form whose post-pass reads c->fa -- PinnedPairs segment by segment.  The constructor takes the
 * longest pairs of every segment of a validated batch (h_offsets null: one segment, the whole buffer): the ids of segment k at ids[offsets[k],
 * offsets[k] + numPairs[k]).  keepPositions: pos[] holds each pair's position IN ITS SEGMENT at the index of its id; else pos is room the scan
 * needs and holds nothing.  The caller holds c->lock through `guard`, size > 0: the GPU platform runs the pipelined batch path under it and
 * leaves it held; the CPU platforms unlock it and match segment by segment (hostLongestPairs takes the lock while it prepares the tables:
 * several threads match side by side).  Then pin(generation): the set held still for the post-pass, PATTERNS_NOT_READY if it is not that
 * generation's any more -- generations only count up, so a set that is the caller's now was the caller's during every scan */
class HostBatchPairs {
public:
    HostBatchPairs(PFAC_context *c, char *h_input, size_t size, const size_t *h_offsets, size_t numSegments, bool keepPositions,
                   std::unique_lock<std::mutex> &guard);
    HostBatchPairs(const HostBatchPairs &) = delete;
    PFAC_status_t pin(unsigned long long generation) { return pin_.emplace(c_, generation).status(); }
    PFAC_status_t status = PFAC_STATUS_SUCCESS;
    const size_t *offsets;                    /* h_offsets, or {0, size} */
    int *ids = nullptr, *pos = nullptr;
    std::vector<int> numPairs;
private:
    PFAC_status_t scan(char *h_input, size_t size, size_t numSegments, bool keepPositions, std::unique_lock<std::mutex> &guard);
    PFAC_context *c_;
    size_t whole_[2];
    std::optional<HostPairs> pairs_;
    std::optional<SetPin> pin_;
};
/* The id a pattern line is reported under (rule sets, group tables): the id itself where it is in the trie; for the lower id of duplicate lines
 * the id that has its bytes; 0 for a pattern the set does not report at all.  The map from bytes to id is built by the first id that is not in
 * the trie */
class ReportedIds {
public:
    explicit ReportedIds(const pfac::Automaton &fa) : fa_(fa) {}
    int of(int id)                            /* id of [1, fa.numPatterns] */
    {
        if (fa_.chainLen[(size_t)id] > 0) return id;
        if (map_.empty())
            for (int q = 1; q <= fa_.numPatterns; q++)
                if (fa_.chainLen[(size_t)q] > 0) map_.emplace(bytesOf(q), q);
        const auto it = map_.find(bytesOf(id));
        return it == map_.end() ? 0 : it->second;
    }
private:
    std::string bytesOf(int id) const { return std::string(reinterpret_cast<const char *>(fa_.file.data()) + fa_.patternOff[(size_t)id], (size_t)fa_.patternLen[(size_t)id]); }
    const pfac::Automaton &fa_;
    std::unordered_map<std::string, int> map_;
};
/* A rule set inverted by pattern (rules_api.cpp: invertRules), what a PFACX_rules_s and a PFACX_flowRules_s each hold one of: memberOff[F + 2],
 * member[] = rule << 5 | bit, ascending rule within a pattern; need[rule], the bits of the positive members.  A conditioned set (PFACX_rulesOpenEx)
 * has memberCond, a window {lo, hi} per membership indexed like member[] (2 j, 2 j + 1; pfac_context.h: kCondEnd); empty: a plain set, every
 * occurrence sets its bit.  A set with chains (PFACX_rulesOpenSeq with a PFACX_RULE_RELATIVE member) has the links of rule r at seqLink[kSeqLinkWords
 * seqOff[r], kSeqLinkWords seqOff[r + 1]), chain by chain in rule order; empty: no rule has a chain */
struct RuleTables {
    size_t numRules = 0, numIds = 0;          /* numIds: F of the pattern set it was opened on */
    std::vector<int> memberOff, seqOff;
    std::vector<unsigned int> member, need, memberCond, seqLink;
    bool conditioned() const { return !memberCond.empty(); }
    bool sequenced() const { return !seqOff.empty(); }
};
/* rules_api.cpp: the plain rules of PFACX_rulesOpen, validated and inverted exactly as that call does it (the caller holds c->lock, fa is the
 * handle's set, the pointers are not null) -- what a flow-rule set (flowrules_api.cpp) is opened over: bit b of a rule is its b-th resolved id in
 * ascending order.  INVALID_PARAMETER: whatever PFACX_rulesOpen refuses, the limits on numRules included */
PFAC_status_t invertPlainRules(const pfac::Automaton &fa, const int *h_ruleOff, const int *h_rulePatterns, size_t numRules, RuleTables *out);
/* The rule masks the pairs ids[0, numPairs) of one segment (or piece) set: every membership j of every pattern q on pair i's prefix chain that
 * accept(i, j, q) lets through ORs its bit into mask[rule]; `touched` returns as the rules whose mask left 0, in the order they were met.  mask[]
 * is all 0 on entry, and whoever decides the touched rules clears what was set */
template <class Accept>
inline void touchedRuleMasks(const pfac::Automaton &fa, const RuleTables &t, const int *ids, size_t numPairs, std::vector<unsigned int> &mask,
                             std::vector<unsigned int> &touched, Accept accept)
{
    touched.clear();
    for (size_t i = 0; i < numPairs; i++)
        forEachChainMember(fa, ids[i], [&](int q) {           /* (the caller's pin: fa.numPatterns == t.numIds) */
            for (int j = t.memberOff[(size_t)q]; j < t.memberOff[(size_t)q + 1]; j++) {
                if (!accept(i, (size_t)j, q)) continue;
                const unsigned int m = t.member[(size_t)j], r = m >> 5;
                if (mask[r] == 0) touched.push_back(r);
                mask[r] |= 1u << (m & 31u);
            }
            return true;
        });
}
/* The host frame of "a sorted list of entries per segment, in CSR form" (the rules, flow-rules and count-batch host forms; segmentWindowPasses
 * of scan_passes.h on the device).  Segment by segment: segFirst[k] (where given) is the running total, fill(k, keys) puts the segment's keys
 * into the cleared `keys`, they are sorted ascending, then store(k, key, at, fits) for every key -- `at` its place in the whole list, fits == at <
 * capacity: only then may the entry be written, else it is only counted.  segFirst[numSegments] closes the list.  Returns the full length */
template <class Key, class Fill, class Store>
inline size_t sortedSegmentLists(size_t numSegments, size_t capacity, size_t *segFirst, Fill fill, Store store)
{
    std::vector<Key> keys;
    size_t total = 0;
    for (size_t k = 0; k < numSegments; k++) {
        if (segFirst) segFirst[k] = total;
        keys.clear();
        fill(k, keys);
        std::sort(keys.begin(), keys.end());
        for (const Key key : keys) {
            store(k, key, total, total < capacity);
            total++;
        }
    }
    if (segFirst) segFirst[numSegments] = total;
    return total;
}
/* ... the store of the forms whose entry is (segment or piece, rule) */
inline auto storeSegmentAndRule(int *seg, int *rule) { return [=](size_t k, unsigned int r, size_t at, bool fits) { if (fits) { seg[at] = (int)k; rule[at] = (int)r; } }; }
/* all_api.cpp: the device copy of {fa.prefixPattern, fa.chainLen} by id (scratch.allTable) that the all-match expansion and the count calls read;
 * the caller holds c->lock */
PFAC_status_t ensureAllTable(PFAC_context *c);
/* host_pipeline.cpp: PFACX_matchBatchFromHost on the GPU platform (h_offsets validated); the caller holds c->lock */
PFAC_status_t matchBatchHostOnGpu(PFAC_context *c, char *h_input, size_t size, const size_t *h_offsets, size_t numSegments, int *h_matched_result);

} // namespace pfac_internal

#endif
