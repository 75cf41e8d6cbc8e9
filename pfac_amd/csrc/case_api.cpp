/*
 * case_api.cpp -- PFACX_caseOpen / PFACX_caseClose / PFACX_caseMatchFromDevice / ...FromHost / PFACX_casePairsFromDevice (include/pfac_ext.h):
 * per-pattern case sensitivity over a caseless set.
 *
 * The handle's set is the folded one: lines with the same folded bytes are one automaton id q, the highest of their ids.  PFACX_caseOpen runs the
 * caller's UNFOLDED text through the compiler's line splitter (pfac::compilePatternBytes without PFACX_READ_NOCASE), checks line by line that its
 * fold is the handle's set, and resolves the lines of each q into VARIANTS: the caseless lines of the class are one pattern, the sensitive ones
 * one per distinct byte string, each reported under the highest of its line ids; a class's variants are stored by id descending, in CSR form by q
 * (buildVariants).  Every pattern of the folded set that occurs at p is a prefix of the longest one there, so all three forms work on the caseless
 * LONGEST pairs and walk each pair's prefix chain (Automaton::prefixPattern), member by member through its variants: a caseless variant holds, a
 * sensitive one where the caller's bytes equal its own.  The device form runs the unchanged compacted-output path with its ordered pairs in
 * handle scratch (PFACX_allReduce) and the passes of scan_case.hip (PFACX_caseRun) behind it, which read the CALLER's bytes; the pairs form runs
 * those passes over a list of the caller's.  The host form takes the longest pairs from hostLongestPairs into a temporary of its own and walks
 * the chains here (caseOnHost).
 * The order of the checks, the scan, the pair temporaries and the generation re-check of the three forms are the frame of verify_calls.h; this
 * file's own is the variant tables, the check of the folded lines in PFACX_caseOpen, the run's arguments (caseRunLocked) and the host loop.
 */
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "pfac_host.h"
#include "verify_calls.h"

struct PFACX_case_s : pfac_internal::HandleObject {
    size_t numIds = 0;                        /* F of the pattern set it was opened on */
    /* by automaton id q: the variants of its class at vars[varOff[q] & ~kTrivial, varOff[q + 1] & ~kTrivial), {line id, dword index of the
     * original bytes in blob; -1: caseless}, by line id descending; kTrivial on varOff[q]: one caseless variant, which is then q itself */
    std::vector<unsigned int> varOff;         /* [F + 2] */
    std::vector<pfac::Int2> vars;
    std::vector<unsigned int> blob;           /* the bytes of the sensitive variants, each padded to whole dwords */
    int maxPerPosition = 1;                   /* the longest ALL list of one position */
    /* the same on the device, uploaded by the first device call: state of the object (deviceTableBytes), freed by PFACX_caseClose */
    pfac::DeviceBuffer<unsigned int> d_varOff, d_blob;
    pfac::DeviceBuffer<pfac::Int2> d_vars;

    template <class Self, class F> static void forEachDeviceBuffer(Self &self, F f) { f(self.d_varOff); f(self.d_vars); f(self.d_blob); }
    PFAC_status_t uploadTables() { return pfac_internal::uploadAll(d_varOff, varOff, d_vars, vars, d_blob, blob); }
    ~PFACX_case_s() override { forEachDeviceBuffer(*this, [](auto &b) { b.release(); }); }
    size_t deviceBytes() const override { size_t n = 0; forEachDeviceBuffer(*this, [&n](const auto &b) { n += b.bytes(); }); return n; }
};

using namespace pfac_internal;

namespace {

constexpr unsigned int kTrivial = 0x80000000u;

/* The tables of `cs` from the unfolded lines of `text` (split by the compiler: `lines`) and the caller's flags; fa is the handle's folded set, and
 * the caller has checked that the fold of line i is fa's pattern i */
void buildVariants(const pfac::Automaton &fa, const pfac::Automaton &lines, const unsigned char *sensitive, PFACX_case_s *cs)
{
    const size_t F = (size_t)fa.numPatterns;
    ReportedIds reported(fa);
    /* the lines of each class, highest id first; then per class: one caseless variant (its highest caseless id), one per distinct sensitive text */
    std::vector<std::vector<int>> members(F + 1);
    for (size_t id = F; id >= 1; id--) {
        const int q = reported.of((int)id);
        if (q) members[(size_t)q].push_back((int)id);
    }
    cs->numIds = F;
    cs->varOff.assign(F + 2, 0u);
    cs->vars.clear();
    cs->blob.clear();
    std::vector<int> perClass(F + 1, 0);
    for (size_t q = 1; q <= F; q++) {
        cs->varOff[q] = (unsigned int)cs->vars.size();
        bool caselessSeen = false;
        std::map<std::string, bool> exactSeen;
        for (const int id : members[q]) {
            const char *bytes = reinterpret_cast<const char *>(lines.file.data()) + lines.patternOff[(size_t)id];
            const size_t len = (size_t)lines.patternLen[(size_t)id];
            if (!sensitive[id]) {
                if (!caselessSeen) cs->vars.push_back(pfac::Int2{id, -1});
                caselessSeen = true;
                continue;
            }
            if (!exactSeen.emplace(std::string(bytes, len), true).second) continue;       /* an exact duplicate of a higher id */
            cs->vars.push_back(pfac::Int2{id, (int)cs->blob.size()});
            const size_t at = cs->blob.size();
            cs->blob.resize(at + (len + 3) / 4, 0u);
            std::memcpy(cs->blob.data() + at, bytes, len);
        }
        const size_t count = cs->vars.size() - cs->varOff[q];
        perClass[q] = (int)count;
        if (count == 1 && cs->vars.back().y < 0) cs->varOff[q] |= kTrivial;               /* (then its id is q: the highest id of the class) */
    }
    cs->varOff[F + 1] = (unsigned int)cs->vars.size();
    cs->varOff[0] = 0u;
    /* the longest ALL list of a position: over the chains, the sum of the members' variants -- a pattern's sum needs its prefix's, which is shorter */
    std::vector<int> byLen;
    for (size_t q = 1; q <= F; q++)
        if (fa.chainLen[q] > 0) byLen.push_back((int)q);
    std::sort(byLen.begin(), byLen.end(), [&](int x, int y) { return fa.patternLen[(size_t)x] < fa.patternLen[(size_t)y]; });
    std::vector<long long> sum(F + 1, 0);
    long long most = 1;
    for (const int q : byLen) {
        const int above = fa.prefixPattern[(size_t)q];
        sum[(size_t)q] = perClass[(size_t)q] + (above >= 1 && (size_t)above <= F ? sum[(size_t)above] : 0);
        most = std::max(most, sum[(size_t)q]);
    }
    cs->maxPerPosition = (int)std::min<long long>(most, 0x7fffffff);
}

/* the arguments of one call: the flags are this family's own test */
VerifyCall caseCall(const char *input, size_t size, unsigned int flags, int *ids, int *pos, size_t capacity, size_t *h_num_matched)
{
    return VerifyCall{input, size, ids, pos, capacity, h_num_matched, (flags & ~PFACX_CASE_ALL) == 0u};
}

/* the passes over `count` ordered longest pairs, behind the argument checks; the caller holds c->lock */
PFAC_status_t caseRunLocked(PFACX_case_s *cs, const VerifyCall &call, unsigned int flags, const int *d_pairIds, const int *d_pairPos, size_t count)
{
    PFAC_context *c = cs->handle;
    PFACX_caseRun_t run{};
    PFAC_status_t st = ensurePatternLen(c);
    if (st == PFAC_STATUS_SUCCESS) st = fillRunFrame(cs, call, d_pairIds, d_pairPos, count, &run.v);
    if (st != PFAC_STATUS_SUCCESS) return st;
    run.d_patternLen = c->scratch.patternLen.get();
    run.d_varOff = cs->d_varOff.get();
    run.d_vars = cs->d_vars.get();
    run.numVars = cs->vars.size();
    run.all = (flags & PFACX_CASE_ALL) ? 1u : 0u;
    return finishRun(c, c->case_run_ptr, run, call);
}

/* The host loop: the variants that hold along the chains of `count` ordered longest pairs into ids / pos (slots >= capacity are not written);
 * returns the full length of the list */
size_t caseOnHost(const pfac::Automaton &fa, const PFACX_case_s &cs, const unsigned char *in, size_t n, bool all, const int *pairIds,
                  const int *pairPos, size_t count, int *ids, int *pos, size_t capacity)
{
    size_t total = 0;
    const unsigned char *blob = reinterpret_cast<const unsigned char *>(cs.blob.data());
    for (size_t i = 0; i < count; i++) {
        const int p = pairPos[i];
        if (p < 0 || (size_t)p >= n) continue;
        forEachChainMember(fa, pairIds[i], [&](int q) {                       /* (the caller's pin: fa.numPatterns == cs.numIds) */
            const size_t len = (size_t)fa.patternLen[(size_t)q];
            if (len == 0 || (size_t)p + len > n) return true;
            const size_t first = cs.varOff[(size_t)q] & ~kTrivial, end = cs.varOff[(size_t)q + 1] & ~kTrivial;
            for (size_t v = first; v < end; v++) {
                const pfac::Int2 var = cs.vars[v];
                if (var.y >= 0 && std::memcmp(in + p, blob + 4 * (size_t)var.y, len) != 0) continue;
                if (total < capacity) { ids[total] = var.x; pos[total] = p; }
                total++;
                if (!all) return false;                                       /* list mode: the longest pattern, the highest id */
            }
            return true;
        });
    }
    return total;
}

} // namespace

extern "C" {

PFAC_status_t PFACX_caseOpen(PFAC_handle_t handle, const char *patterns, size_t size, unsigned int readFlags, const unsigned char *h_sensitive,
                             size_t numFlags, PFACX_case_t *cs, int *maxMatchesPerPosition)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!cs) return PFAC_STATUS_INVALID_PARAMETER;
    *cs = nullptr;
    if (!patterns || !h_sensitive) return PFAC_STATUS_INVALID_PARAMETER;
    /* the caller's text through the compiler's own splitter, unfolded: the lines by id, before the handle's lock is taken */
    pfac::Automaton lines;
    try {
        const unsigned char *text = reinterpret_cast<const unsigned char *>(patterns);
        const PFAC_status_t st = pfac::compilePatternBytes(std::vector<unsigned char>(text, text + size), lines,
                                                           readFlags & (PFACX_READ_STRICT | PFACX_READ_STRIP_CR));
        if (st != PFAC_STATUS_SUCCESS) return st;
    } catch (const std::bad_alloc &) { return PFAC_STATUS_ALLOC_FAILED; }
    const PFAC_status_t st = adoptNew(handle, cs, [&](PFACX_case_s &obj) -> PFAC_status_t {
        const pfac::Automaton &fa = handle->fa;
        if (!handle->caseInsensitive || lines.numPatterns != fa.numPatterns || numFlags < (size_t)fa.numPatterns + 1) return PFAC_STATUS_INVALID_PARAMETER;
        for (int id = 1; id <= fa.numPatterns; id++) {
            const size_t len = (size_t)fa.patternLen[(size_t)id];
            if ((size_t)lines.patternLen[(size_t)id] != len) return PFAC_STATUS_INVALID_PARAMETER;
            const unsigned char *mine = lines.file.data() + lines.patternOff[(size_t)id], *theirs = fa.file.data() + fa.patternOff[(size_t)id];
            for (size_t i = 0; i < len; i++)
                if (pfac::asciiFold(mine[i]) != theirs[i]) return PFAC_STATUS_INVALID_PARAMETER;
        }
        buildVariants(fa, lines, h_sensitive, &obj);
        return PFAC_STATUS_SUCCESS;
    });
    if (st == PFAC_STATUS_SUCCESS && maxMatchesPerPosition) *maxMatchesPerPosition = (*cs)->maxPerPosition;
    return st;
}

PFAC_status_t PFACX_caseClose(PFACX_case_t cs) { return closeObject(cs); }

PFAC_status_t PFACX_caseMatchFromDevice(PFACX_case_t cs, char *d_input, size_t size, unsigned int flags, int *d_ids, int *d_pos, size_t capacity,
                                        size_t *h_num_matched)
{
    const VerifyCall call = caseCall(d_input, size, flags, d_ids, d_pos, capacity, h_num_matched);
    return verifyFromDevice(cs, call, [&](const int *ids, const int *pos, size_t count) { return caseRunLocked(cs, call, flags, ids, pos, count); });
}

PFAC_status_t PFACX_caseMatchFromHost(PFACX_case_t cs, char *h_input, size_t size, unsigned int flags, int *h_ids, int *h_pos, size_t capacity,
                                      size_t *h_num_matched)
{
    const VerifyCall call = caseCall(h_input, size, flags, h_ids, h_pos, capacity, h_num_matched);
    return verifyFromHost(cs, call, [&](const int *ids, const int *pos, size_t count) {
        return caseOnHost(cs->handle->fa, *cs, reinterpret_cast<const unsigned char *>(h_input), size, (flags & PFACX_CASE_ALL) != 0, ids, pos, count,
                          h_ids, h_pos, capacity);
    });
}

PFAC_status_t PFACX_casePairsFromDevice(PFACX_case_t cs, const char *d_input, size_t size, unsigned int flags, const int *d_pairIds,
                                        const int *d_pairPos, size_t numPairs, int *d_ids, int *d_pos, size_t capacity, size_t *h_num_matched)
{
    const VerifyCall call = caseCall(d_input, size, flags, d_ids, d_pos, capacity, h_num_matched);
    return verifyPairsFromDevice(cs, call, d_pairIds, d_pairPos, numPairs, {d_ids, d_pos},
                                 [&](const int *ids, const int *pos, size_t count) { return caseRunLocked(cs, call, flags, ids, pos, count); });
}

} /* extern "C" */
