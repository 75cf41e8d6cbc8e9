/*
 * verify_calls.h -- the host frame of the six VERIFY families (case_api.cpp, sig_api.cpp, approx_api.cpp, gapsig_api.cpp, edit_api.cpp,
 * clsig_api.cpp with its batch forms).  Each loads a derived pattern set into the handle -- anchors, pieces, folded lines --, takes the ordered
 * LONGEST pairs of a scan, walks every pair's prefix chain through a per-id class table and verifies every candidate against the caller's bytes.
 * What is here once:
 *   StringSet, adoptOverStrings   the open tail: the derived strings interned as "text, one line each", loaded through the reader of every
 *                                 pattern set, and the new object adopted only where the handle really holds them, id by id
 *   checkVerifyArgs               what the three match calls check first
 *   ensureDeviceTables            the first device call of an object: its tables up, or none of them
 *   fillRunFrame, finishRun       around a family's PFACX_*Run: the chain table, the tables, the common head of the run (pfac_module.h:
 *                                 PFACX_verifyRun_t); the module's call, the length of the list, the status
 *   verifyFromDevice, verifyFromHost, verifyPairsFromDevice
 *                                 the three forms.  A family hands in VerifyCall (the arguments every form has) and its part as callables:
 *                                 run(pairIds, pairPos, count) under the handle's lock, onHost(pairIds, pairPos, count) -> the length of the list,
 *                                 and where it has them extra checks in front of the lock (`pre`) and what an empty pair list leaves to do (`onEmpty`)
 * THE ORDER OF THE CHECKS is the calls' contract (tests/test_verify_frame_host.py walks it): the object, the arguments, the family's own, a device
 * form's capacity or a pairs form's overlap test, the module, then under the lock the generation and the empty exits.
 */
#ifndef PFAC_VERIFY_CALLS_H
#define PFAC_VERIFY_CALLS_H

#include <cstring>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "pfac_host.h"

namespace pfac_internal {

/* distinct strings in order of first appearance: ids from 1, the text the pattern reader takes with one line each */
struct StringSet {
    std::vector<std::string> strings;                 /* by id - 1 */
    std::string text;
    int idOf(const std::string &s)
    {
        const auto placed = seen.emplace(s, (int)strings.size() + 1);
        if (placed.second) {
            strings.push_back(s);
            text += s;
            text += '\n';
        }
        return placed.first->second;
    }
    size_t size() const { return strings.size(); }

private:
    std::map<std::string, int> seen;
};

/* The open tail: the strings through the reader of every pattern set -- the set is replaced, the handle case-sensitive --, then a new T whose
 * setUp(T &) runs only where the handle holds exactly these strings, id by id: another thread may have replaced the set since */
template <class T, class SetUp>
PFAC_status_t adoptOverStrings(PFAC_context *handle, const StringSet &set, T **out, SetUp setUp)
{
    const PFAC_status_t st = PFACX_readPatternFromMemory(handle, set.text.data(), set.text.size());
    if (st != PFAC_STATUS_SUCCESS) return st;
    return adoptNew(handle, out, [&](T &obj) -> PFAC_status_t {
        const pfac::Automaton &fa = handle->fa;
        if (handle->caseInsensitive || (size_t)fa.numPatterns != set.size()) return PFAC_STATUS_INVALID_PARAMETER;
        for (size_t q = 1; q <= set.size(); q++) {
            const std::string &s = set.strings[q - 1];
            if ((size_t)fa.patternLen[q] != s.size() || fa.chainLen[q] < 1 || std::memcmp(fa.file.data() + fa.patternOff[q], s.data(), s.size()) != 0)
                return PFAC_STATUS_INVALID_PARAMETER;
        }
        return setUp(obj);
    });
}

/* the arguments every form of every family has.  ownOk: the family's own test of its arguments (the flags of PFACX_case*), refused with the rest */
struct VerifyCall {
    const char *input;
    size_t size;
    int *ids, *pos;
    size_t capacity;
    size_t *h_num_matched;
    bool ownOk = true;
};

/* what the three match calls check first (the generation and the pattern set: under the lock) */
inline PFAC_status_t checkVerifyArgs(const HandleObject *obj, const VerifyCall &call)
{
    if (!obj || !obj->handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!call.input || !call.h_num_matched || !call.ownOk || call.size > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    return PFAC_STATUS_SUCCESS;
}

/* the first device call of an object: its tables (Obj::uploadTables) -- all of them or none, so the FIRST buffer of forEachDeviceBuffer (the
 * class offsets: never empty) says whether they are up; the caller holds the handle's lock */
template <class Obj>
PFAC_status_t ensureDeviceTables(Obj *obj)
{
    bool first = true, up = false;
    Obj::forEachDeviceBuffer(*obj, [&](const auto &b) {
        if (first) up = static_cast<bool>(b);
        first = false;
    });
    if (up) return PFAC_STATUS_SUCCESS;
    const PFAC_status_t st = obj->uploadTables();
    if (st != PFAC_STATUS_SUCCESS) Obj::forEachDeviceBuffer(*obj, [](auto &b) { b.release(); });
    return st;
}

/* In front of a family's PFACX_*Run, behind the argument checks, under c->lock: the chain table and the object's tables on the device, and the
 * head of the run over `count` ordered longest pairs.  obj->numIds and obj->d_blob / obj->blob are every family's */
template <class Obj>
PFAC_status_t fillRunFrame(Obj *obj, const VerifyCall &call, const int *d_pairIds, const int *d_pairPos, size_t count, PFACX_verifyRun_t *v)
{
    PFAC_context *c = obj->handle;
    PFAC_status_t st = c->fa.maxChain > 1 ? ensureAllTable(c) : PFAC_STATUS_SUCCESS;
    if (st == PFAC_STATUS_SUCCESS) st = ensureDeviceTables(obj);
    if (st != PFAC_STATUS_SUCCESS) return st;
    v->d_input = call.input;
    v->size = call.size;
    v->d_pairIds = d_pairIds;
    v->d_pairPos = d_pairPos;
    v->count = count;
    v->d_table = c->fa.maxChain > 1 ? c->scratch.allTable.get() : nullptr;
    v->numIds = obj->numIds;
    v->d_blob = obj->d_blob.get();
    v->blobWords = obj->blob.size();
    v->d_ids = call.ids;
    v->d_pos = call.pos;
    v->capacity = call.capacity;
    return PFAC_STATUS_SUCCESS;
}

/* ... and behind it: the module's passes, the full length of the list to the caller, TRUNCATED where it did not fit */
template <class Run>
PFAC_status_t finishRun(PFAC_context *c, PFAC_status_t (*runPtr)(PFAC_handle_t, const Run *, size_t *), const Run &run, const VerifyCall &call)
{
    size_t total = 0;
    const PFAC_status_t st = runPtr(c, &run, &total);
    if (st != PFAC_STATUS_SUCCESS) return st;
    *call.h_num_matched = total;
    return truncatedIf(total, call.capacity);
}

/* the callable of a family that has nothing to check or to do at one of the frame's hooks */
struct NothingMore {
    PFAC_status_t operator()() const { return PFAC_STATUS_SUCCESS; }
};

/* The device form: the unchanged compacted-output scan with its ordered pairs in handle scratch (PFACX_allReduce), then run(pairIds, pairPos,
 * count) over them.  The caller's arrays take the scan's unordered list first, so they are needed whatever the capacity, with size entries */
template <class Obj, class Run, class Pre = NothingMore, class Empty = NothingMore>
PFAC_status_t verifyFromDevice(Obj *obj, const VerifyCall &call, Run run, Pre pre = Pre(), Empty onEmpty = Empty())
{
    PFAC_status_t st = checkVerifyArgs(obj, call);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (!call.ids || !call.pos) return PFAC_STATUS_INVALID_PARAMETER;
    if ((st = pre()) != PFAC_STATUS_SUCCESS) return st;
    PFAC_context *c = obj->handle;
    if (call.size && call.capacity < call.size) return PFAC_STATUS_INVALID_PARAMETER;
    if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(c->lock);
    st = checkSetGeneration(c, obj->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (call.size == 0) { *call.h_num_matched = 0; return PFAC_STATUS_SUCCESS; }
    DeviceScan scan;                                                       /* a caseless handle: the scan reads the folded copy, the passes the caller's bytes */
    st = beginDeviceScan(c, const_cast<char *>(call.input), call.size, &scan);
    if (st != PFAC_STATUS_SUCCESS) return st;
    /* the caller's arrays take the scan's unordered list, the ordered pairs go to the handle's pair scratch: the passes never filter in place */
    int count = 0;
    st = c->all_reduce_ptr(c, reinterpret_cast<int *>(scan.d_scan), (int)call.size, call.ids, call.pos, &count, scan.hashed);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (count < 0 || (size_t)count > call.size) return PFAC_STATUS_INTERNAL_ERROR;
    const int *pairIds = c->scratch.allPairs.get();
    const int *pairPos = pairIds + c->scratch.allPairs.count() / 2;        /* one allocation: the ids, then as many positions */
    if (count == 0) { *call.h_num_matched = 0; return onEmpty(); }
    return run(pairIds, pairPos, (size_t)count);
}

/* The host form: the longest pairs from hostLongestPairs into a temporary of its own, the set pinned, then total = onHost(pairIds, pairPos,
 * count) -- a loop over c->fa and the object's host tables that writes no slot at or beyond the capacity */
template <class Obj, class OnHost, class Pre = NothingMore>
PFAC_status_t verifyFromHost(Obj *obj, const VerifyCall &call, OnHost onHost, Pre pre = Pre())
{
    PFAC_status_t st = checkVerifyArgs(obj, call);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (call.capacity && (!call.ids || !call.pos)) return PFAC_STATUS_INVALID_PARAMETER;
    if ((st = pre()) != PFAC_STATUS_SUCCESS) return st;
    PFAC_context *c = obj->handle;
    {
        std::lock_guard<std::mutex> guard(c->lock);
        st = checkSetGeneration(c, obj->generation);
        if (st != PFAC_STATUS_SUCCESS) return st;
    }
    if (call.size == 0) { *call.h_num_matched = 0; return PFAC_STATUS_SUCCESS; }
    if (hostLacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    const HostPairs pairs(call.size, call.size);
    if (!pairs) return PFAC_STATUS_ALLOC_FAILED;
    const PinnedPairs scan(c, const_cast<char *>(call.input), call.size, pairs.ids, pairs.pos);
    if (scan.status != PFAC_STATUS_SUCCESS) return scan.status;
    if (scan.generation != obj->generation) return PFAC_STATUS_INVALID_PARAMETER;    /* another thread has replaced the set meanwhile: as after the call */
    const size_t total = onHost(pairs.ids, pairs.pos, (size_t)(scan.count > 0 ? scan.count : 0));
    *call.h_num_matched = total;
    return truncatedIf(total, call.capacity);
}

/* The pairs form: run over a list of the caller's.  outputs: every array the passes write capacity entries of (null: not asked for) -- none
 * may share a byte with the pair arrays */
template <class Obj, class Run, class Pre = NothingMore, class Empty = NothingMore>
PFAC_status_t verifyPairsFromDevice(Obj *obj, const VerifyCall &call, const int *d_pairIds, const int *d_pairPos, size_t numPairs,
                                    std::initializer_list<const int *> outputs, Run run, Pre pre = Pre(), Empty onEmpty = Empty())
{
    PFAC_status_t st = checkVerifyArgs(obj, call);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (numPairs > kMaxInt || call.capacity > SIZE_MAX / sizeof(int) || (numPairs && (!d_pairIds || !d_pairPos)) || (call.capacity && (!call.ids || !call.pos)))
        return PFAC_STATUS_INVALID_PARAMETER;
    if ((st = pre()) != PFAC_STATUS_SUCCESS) return st;
    if (call.capacity && numPairs) {
        const size_t in = numPairs * sizeof(int), out = call.capacity * sizeof(int);
        for (const int *array : outputs)
            if (array && (overlap(array, out, d_pairIds, in) || overlap(array, out, d_pairPos, in))) return PFAC_STATUS_INVALID_PARAMETER;
    }
    PFAC_context *c = obj->handle;
    if (lacksModule(c)) return PFAC_STATUS_LIB_NOT_EXIST;
    std::lock_guard<std::mutex> guard(c->lock);
    st = checkSetGeneration(c, obj->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (call.size == 0) { *call.h_num_matched = 0; return PFAC_STATUS_SUCCESS; }
    if (numPairs == 0) { *call.h_num_matched = 0; return onEmpty(); }
    return run(d_pairIds, d_pairPos, numPairs);
}

} // namespace pfac_internal

#endif
