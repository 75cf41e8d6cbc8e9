/*
 * sig_api.cpp -- PFACX_sigOpen / PFACX_sigOpenText / PFACX_sigGetAnchors / PFACX_sigClose / PFACX_sigMatchFromDevice / ...FromHost /
 * PFACX_sigPairsFromDevice (include/pfac_ext.h): masked byte signatures with wildcards.
 *
 * A signature is a fixed-length string of (value, mask) bytes.  PFACX_sigOpen copies the caller's CSR arrays, canonicalises value &= mask, picks
 * one fully specified run of each signature as its ANCHOR (chooseAnchor: the longest run of bytes with mask 0xFF and a value other than '\n', the
 * leftmost of equal ones, cut to its first maxAnchorLen bytes), loads the distinct anchors into the handle through the reader every pattern set
 * goes through -- one line per anchor, in order of first appearance, so handle id q is the q-th distinct anchor -- and builds per handle id q the
 * signatures of its class (buildTables): {signature id, anchorOff, len, blobOff} by id descending, in CSR form by q, with a dword-aligned blob of
 * each signature's value dwords and mask dwords.  PFACX_sigOpenText is a parser in front of it (parseText).  Every anchor that occurs at p is a
 * prefix of the longest one there, so all three match forms work on the LONGEST pairs of the anchor set and walk each pair's prefix chain
 * (Automaton::prefixPattern), member by member through its class: a signature starts at p - anchorOff, must lie inside the input, and holds
 * where every masked byte does.  The device form runs the unchanged compacted-output path with its ordered pairs in handle scratch
 * (PFACX_allReduce) and the passes of scan_sig.hip (PFACX_sigRun) behind it; the pairs form runs those passes over a list of the caller's.  The
 * host form takes the longest pairs from hostLongestPairs into a temporary of its own and walks the chains here (sigOnHost).
 * The open tail (the anchors loaded and the handle checked to hold them), the order of the checks, the scan, the pair temporaries and the
 * generation re-check of the three forms are the frame of verify_calls.h; this file's own is the plan, the tables, the run's arguments
 * (sigRunLocked) and the host loop.
 */
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "pfac_host.h"
#include "verify_calls.h"

struct PFACX_sig_s : pfac_internal::HandleObject {
    size_t numIds = 0;                        /* F of the anchor set it loaded */
    size_t numSigs = 0;                       /* S */
    /* by signature id (entry 0 unused): the handle's pattern id of its anchor, the anchor's offset inside the signature, its length */
    std::vector<int> anchorId, anchorOff, anchorLen;
    /* by handle id q: the signatures of its class at sigs[sigOff[q], sigOff[q + 1]), by signature id descending */
    std::vector<unsigned int> sigOff;         /* [F + 2] */
    std::vector<pfac::SigEntry> sigs;         /* [S] */
    std::vector<unsigned int> blob;           /* per signature (len + 3) / 4 value dwords, then as many mask dwords; the bytes behind len: mask 0 */
    /* the same on the device, uploaded by the first device call: state of the object (deviceTableBytes), freed by PFACX_sigClose */
    pfac::DeviceBuffer<unsigned int> d_sigOff, d_blob;
    pfac::DeviceBuffer<pfac::SigEntry> d_sigs;

    template <class Self, class F> static void forEachDeviceBuffer(Self &self, F f) { f(self.d_sigOff); f(self.d_sigs); f(self.d_blob); }
    PFAC_status_t uploadTables() { return pfac_internal::uploadAll(d_sigOff, sigOff, d_sigs, sigs, d_blob, blob); }
    ~PFACX_sig_s() override { forEachDeviceBuffer(*this, [](auto &b) { b.release(); }); }
    size_t deviceBytes() const override { size_t n = 0; forEachDeviceBuffer(*this, [&n](const auto &b) { n += b.bytes(); }); return n; }
};

using namespace pfac_internal;

namespace {

constexpr size_t kMaxSigLen = 65535, kDefaultAnchorLen = 32;

/* the caller's signatures, copied and canonicalised, with the anchor of each and the anchor set as the reader's text */
struct SigPlan {
    std::vector<unsigned char> values, masks;         /* all signatures back to back */
    std::vector<size_t> off;                          /* [S + 1] into both */
    std::vector<int> anchorId, anchorOff, anchorLen;  /* by signature id */
    StringSet anchors;                                /* by handle id - 1: the distinct anchors, and the anchor set as the reader's text */
};

/* The anchor of one signature: the longest run of bytes with mask 0xFF and a value other than '\n' (the pattern reader splits lines there), the
 * leftmost of equal ones, cut to its first maxAnchorLen bytes.  false: the signature has no such byte */
bool chooseAnchor(const unsigned char *v, const unsigned char *m, size_t len, size_t maxAnchorLen, size_t *off, size_t *alen)
{
    size_t best = 0, bestAt = 0;
    for (size_t i = 0; i < len;) {
        if (m[i] != 0xFF || v[i] == '\n') { i++; continue; }
        size_t j = i;
        while (j < len && m[j] == 0xFF && v[j] != '\n') j++;
        if (j - i > best) { best = j - i; bestAt = i; }
        i = j;
    }
    *off = bestAt;
    *alen = std::min(best, maxAnchorLen);
    return best > 0;
}

/* The plan of S signatures in CSR form.  INVALID_PARAMETER with *badSig = the id of the signature: an offset that does not ascend (an empty
 * signature), a signature longer than 65 535 bytes, one without a fully specified byte other than '\n' */
PFAC_status_t planSignatures(const unsigned char *h_values, const unsigned char *h_masks, const size_t *h_sigOff, size_t numSigs, size_t maxAnchorLen,
                             SigPlan *plan, int *badSig)
{
    const size_t S = numSigs, cut = maxAnchorLen ? maxAnchorLen : kDefaultAnchorLen;
    plan->off.assign(S + 1, 0);
    plan->anchorId.assign(S + 1, 0);
    plan->anchorOff.assign(S + 1, 0);
    plan->anchorLen.assign(S + 1, 0);
    size_t blobWords = 0;
    for (size_t i = 1; i <= S; i++) {
        *badSig = (int)i;
        if (h_sigOff[i] <= h_sigOff[i - 1] || h_sigOff[i] - h_sigOff[i - 1] > kMaxSigLen) return PFAC_STATUS_INVALID_PARAMETER;
        const size_t len = h_sigOff[i] - h_sigOff[i - 1];
        plan->off[i] = plan->off[i - 1] + len;
        blobWords += 2 * ((len + 3) / 4);
    }
    *badSig = 0;
    if (blobWords > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;          /* the tables index the blob with ints */
    plan->values.resize(plan->off[S]);
    plan->masks.resize(plan->off[S]);
    for (size_t i = 1; i <= S; i++) {
        const size_t from = h_sigOff[i - 1], at = plan->off[i - 1], len = plan->off[i] - at;
        unsigned char *v = plan->values.data() + at, *m = plan->masks.data() + at;
        for (size_t k = 0; k < len; k++) {
            m[k] = h_masks[from + k];
            v[k] = (unsigned char)(h_values[from + k] & m[k]);
        }
        size_t aoff = 0, alen = 0;
        if (!chooseAnchor(v, m, len, cut, &aoff, &alen)) { *badSig = (int)i; return PFAC_STATUS_INVALID_PARAMETER; }
        plan->anchorId[i] = plan->anchors.idOf(std::string(reinterpret_cast<const char *>(v) + aoff, alen));
        plan->anchorOff[i] = (int)aoff;
        plan->anchorLen[i] = (int)alen;
    }
    return PFAC_STATUS_SUCCESS;
}

/* the tables of `sg` from the plan: the classes by handle id, each by signature id descending, and the blob */
void buildTables(const SigPlan &plan, PFACX_sig_s *sg)
{
    const size_t S = plan.off.size() - 1, F = plan.anchors.size();
    sg->numIds = F;
    sg->numSigs = S;
    sg->anchorId = plan.anchorId;
    sg->anchorOff = plan.anchorOff;
    sg->anchorLen = plan.anchorLen;
    sg->sigOff.assign(F + 2, 0u);
    for (size_t i = 1; i <= S; i++) sg->sigOff[(size_t)plan.anchorId[i] + 1]++;
    for (size_t q = 1; q <= F + 1; q++) sg->sigOff[q] += sg->sigOff[q - 1];      /* sigOff[q + 1] = the end of class q; sigOff[q]: its start */
    /* (sigOff[0] = sigOff[1] = 0: class 0 is empty) */
    std::vector<unsigned int> next(sg->sigOff.begin(), sg->sigOff.end());
    sg->sigs.assign(S, pfac::SigEntry{0, 0, 0, 0});
    sg->blob.clear();
    for (size_t i = S; i >= 1; i--) {                                              /* id descending within every class */
        const size_t at = plan.off[i - 1], len = plan.off[i] - at, words = (len + 3) / 4, blobAt = sg->blob.size();
        sg->blob.resize(blobAt + 2 * words, 0u);
        std::memcpy(sg->blob.data() + blobAt, plan.values.data() + at, len);
        std::memcpy(sg->blob.data() + blobAt + words, plan.masks.data() + at, len);
        sg->sigs[next[(size_t)plan.anchorId[i]]++] = pfac::SigEntry{(int)i, plan.anchorOff[i], (int)len, (int)blobAt};
    }
}

/* the hex text of PFACX_sigOpenText into CSR arrays; false with *badLine = the 1-based line that is refused */
bool parseText(const char *text, size_t size, std::vector<unsigned char> &values, std::vector<unsigned char> &masks, std::vector<size_t> &off,
               int *badLine)
{
    const auto nibble = [](char c) -> int {          /* 0 .. 15, 16: '?', -1: neither */
        if (c >= '0' && c <= '9') return c - '0';
        if (c >= 'a' && c <= 'f') return c - 'a' + 10;
        if (c >= 'A' && c <= 'F') return c - 'A' + 10;
        return c == '?' ? 16 : -1;
    };
    off.assign(1, 0);
    size_t line = 1;
    for (size_t i = 0; i < size; line++) {
        *badLine = (int)std::min(line, kMaxInt);
        const void *nl = std::memchr(text + i, '\n', size - i);
        if (!nl) return false;                                                 /* bytes behind the last '\n' */
        const size_t stop = (size_t)(static_cast<const char *>(nl) - text);
        size_t end = stop;
        if (end > i && text[end - 1] == '\r') end--;
        const size_t before = values.size();
        for (size_t j = i; j < end;) {
            if (text[j] == ' ' || text[j] == '\t') { j++; continue; }
            const int hi = nibble(text[j]), lo = j + 1 < end ? nibble(text[j + 1]) : -1;
            if (hi < 0 || lo < 0) return false;                                 /* another character, or a digit without its partner */
            values.push_back((unsigned char)((hi < 16 ? hi << 4 : 0) | (lo < 16 ? lo : 0)));
            masks.push_back((unsigned char)((hi < 16 ? 0xF0 : 0) | (lo < 16 ? 0x0F : 0)));
            j += 2;
        }
        if (values.size() == before) return false;                              /* an empty line */
        off.push_back(values.size());
        i = stop + 1;
    }
    *badLine = 0;
    return true;
}

/* the passes over `count` ordered longest pairs, behind the argument checks; the caller holds c->lock */
PFAC_status_t sigRunLocked(PFACX_sig_s *sg, const VerifyCall &call, const int *d_pairIds, const int *d_pairPos, size_t count)
{
    PFACX_sigRun_t run{};
    const PFAC_status_t st = fillRunFrame(sg, call, d_pairIds, d_pairPos, count, &run.v);
    if (st != PFAC_STATUS_SUCCESS) return st;
    run.d_sigOff = sg->d_sigOff.get();
    run.d_sigs = sg->d_sigs.get();
    run.numSigs = sg->sigs.size();
    return finishRun(sg->handle, sg->handle->sig_run_ptr, run, call);
}

/* The host loop: the signatures that hold along the chains of `count` ordered longest pairs into ids / pos (slots >= capacity are not written);
 * returns the full length of the list */
size_t sigOnHost(const pfac::Automaton &fa, const PFACX_sig_s &sg, const unsigned char *in, size_t n, const int *pairIds, const int *pairPos,
                 size_t count, int *ids, int *pos, size_t capacity)
{
    size_t total = 0;
    const unsigned char *blob = reinterpret_cast<const unsigned char *>(sg.blob.data());
    for (size_t i = 0; i < count; i++) {
        const int p = pairPos[i];
        if (p < 0 || (size_t)p >= n) continue;
        forEachChainMember(fa, pairIds[i], [&](int q) {                       /* (the caller's pin: fa.numPatterns == sg.numIds) */
            for (size_t v = sg.sigOff[(size_t)q]; v < sg.sigOff[(size_t)q + 1]; v++) {
                const pfac::SigEntry e = sg.sigs[v];
                if (e.anchorOff > p) continue;                                  /* it would start in front of the input */
                const size_t s = (size_t)(p - e.anchorOff), len = (size_t)e.len;
                if (len > n - s) continue;                                      /* ... or end behind it */
                const unsigned char *val = blob + 4 * (size_t)e.blobOff, *mask = val + 4 * ((len + 3) / 4);
                size_t k = 0;
                while (k < len && ((in[s + k] ^ val[k]) & mask[k]) == 0) k++;
                if (k < len) continue;
                if (total < capacity) { ids[total] = e.id; pos[total] = (int)s; }
                total++;
            }
            return true;
        });
    }
    return total;
}

} // namespace

extern "C" {

PFAC_status_t PFACX_sigOpen(PFAC_handle_t handle, const unsigned char *h_values, const unsigned char *h_masks, const size_t *h_sigOff, size_t numSigs,
                            size_t maxAnchorLen, PFACX_sig_t *sig, int *badSig)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!sig) return PFAC_STATUS_INVALID_PARAMETER;
    *sig = nullptr;
    int bad = 0;
    if (badSig) *badSig = 0;
    if (!h_values || !h_masks || !h_sigOff || numSigs == 0 || numSigs >= kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    SigPlan plan;
    try {
        const PFAC_status_t st = planSignatures(h_values, h_masks, h_sigOff, numSigs, maxAnchorLen, &plan, &bad);
        if (badSig) *badSig = bad;
        if (st != PFAC_STATUS_SUCCESS) return st;                             /* nothing of the handle has changed */
    } catch (const std::bad_alloc &) { return PFAC_STATUS_ALLOC_FAILED; }
    return adoptOverStrings(handle, plan.anchors, sig, [&](PFACX_sig_s &obj) -> PFAC_status_t {       /* (verify_calls.h: the tables hold only over the anchors) */
        buildTables(plan, &obj);
        return PFAC_STATUS_SUCCESS;
    });
}

PFAC_status_t PFACX_sigOpenText(PFAC_handle_t handle, const char *text, size_t size, size_t maxAnchorLen, PFACX_sig_t *sig, int *badLine)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!sig) return PFAC_STATUS_INVALID_PARAMETER;
    *sig = nullptr;
    int bad = 0;
    if (badLine) *badLine = 0;
    if (!text) return PFAC_STATUS_INVALID_PARAMETER;
    std::vector<unsigned char> values, masks;
    std::vector<size_t> off;
    try {
        const bool parsed = parseText(text, size, values, masks, off, &bad);
        if (badLine) *badLine = bad;
        if (!parsed || off.size() < 2) return PFAC_STATUS_INVALID_PARAMETER;  /* (no line at all: numSigs == 0) */
    } catch (const std::bad_alloc &) { return PFAC_STATUS_ALLOC_FAILED; }
    /* a line is a signature: the id the binary form refuses is the line */
    return PFACX_sigOpen(handle, values.data(), masks.data(), off.data(), off.size() - 1, maxAnchorLen, sig, badLine);
}

PFAC_status_t PFACX_sigClose(PFACX_sig_t sig) { return closeObject(sig); }

PFAC_status_t PFACX_sigGetAnchors(PFACX_sig_t sig, int *h_anchorId, int *h_anchorOff, int *h_anchorLen, size_t n)
{
    if (!sig || !sig->handle) return PFAC_STATUS_INVALID_HANDLE;
    PFAC_context *c = sig->handle;
    std::lock_guard<std::mutex> guard(c->lock);
    const PFAC_status_t st = checkSetGeneration(c, sig->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (n < sig->numSigs + 1) return PFAC_STATUS_INVALID_PARAMETER;
    const size_t bytes = (sig->numSigs + 1) * sizeof(int);
    if (h_anchorId) std::memcpy(h_anchorId, sig->anchorId.data(), bytes);
    if (h_anchorOff) std::memcpy(h_anchorOff, sig->anchorOff.data(), bytes);
    if (h_anchorLen) std::memcpy(h_anchorLen, sig->anchorLen.data(), bytes);
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_sigMatchFromDevice(PFACX_sig_t sig, char *d_input, size_t size, int *d_ids, int *d_pos, size_t capacity, size_t *h_num_matched)
{
    const VerifyCall call{d_input, size, d_ids, d_pos, capacity, h_num_matched};
    return verifyFromDevice(sig, call, [&](const int *ids, const int *pos, size_t count) { return sigRunLocked(sig, call, ids, pos, count); });
}

PFAC_status_t PFACX_sigMatchFromHost(PFACX_sig_t sig, char *h_input, size_t size, int *h_ids, int *h_pos, size_t capacity, size_t *h_num_matched)
{
    const VerifyCall call{h_input, size, h_ids, h_pos, capacity, h_num_matched};
    return verifyFromHost(sig, call, [&](const int *ids, const int *pos, size_t count) {
        return sigOnHost(sig->handle->fa, *sig, reinterpret_cast<const unsigned char *>(h_input), size, ids, pos, count, h_ids, h_pos, capacity);
    });
}

PFAC_status_t PFACX_sigPairsFromDevice(PFACX_sig_t sig, const char *d_input, size_t size, const int *d_pairIds, const int *d_pairPos, size_t numPairs,
                                       int *d_ids, int *d_pos, size_t capacity, size_t *h_num_matched)
{
    const VerifyCall call{d_input, size, d_ids, d_pos, capacity, h_num_matched};
    return verifyPairsFromDevice(sig, call, d_pairIds, d_pairPos, numPairs, {d_ids, d_pos},
                                 [&](const int *ids, const int *pos, size_t count) { return sigRunLocked(sig, call, ids, pos, count); });
}

} /* extern "C" */
