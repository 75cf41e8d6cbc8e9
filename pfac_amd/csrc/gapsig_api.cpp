/*
 * gapsig_api.cpp -- PFACX_gapsigOpen / PFACX_gapsigOpenText / PFACX_gapsigGetAnchors / PFACX_gapsigClose / PFACX_gapsigMatchFromDevice /
 * ...FromHost / PFACX_gapsigPairsFromDevice (include/pfac_ext.h): signatures with bounded gaps between parts.
 *
 * A signature is a sequence of parts, each a fixed-length string of (value, mask) bytes, with a gap of lo .. hi bytes between neighbours.
 * PFACX_gapsigOpen copies the caller's CSR arrays, canonicalises value &= mask, checks the limits (planSignatures: parts, slack, span), picks one
 * fully specified run inside one part of each signature as its ANCHOR (chooseAnchor: the longest run of bytes with mask 0xFF and a value other
 * than '\n', of equal ones the one in the lowest part, then the leftmost, cut to its first maxAnchorLen bytes), loads the distinct anchors into
 * the handle through the reader every pattern set goes through -- one line per anchor, in order of first appearance, so handle id q is the q-th
 * distinct anchor -- and builds per handle id q the signatures of its class (buildTables): {signature id, first part, parts | anchor part << 16,
 * anchorOff} by id descending, in CSR form by q, the parts {len, blobOff, lo, hi}, and a dword-aligned blob of each part's value dwords and mask
 * dwords.  PFACX_gapsigOpenText is a parser in front of it (parseText).  All three match forms work on the LONGEST pairs of the anchor set and
 * walk each pair's prefix chain, member by member through its class; per (anchor occurrence, signature) they run the search of scan_gapsig.hip
 * (its header says what it is and why an occurrence is listed once), here over a plain byte loop (searchOnHost).  The device form runs the
 * unchanged compacted-output path with its ordered pairs in handle scratch (PFACX_allReduce) and the passes of scan_gapsig.hip (PFACX_gapsigRun)
 * behind it; the pairs form runs those passes over a list of the caller's.  The host form takes the longest pairs from hostLongestPairs into a
 * temporary of its own (gapsigOnHost).
 * The open tail (the anchors loaded and the handle checked to hold them), the order of the checks, the scan, the pair temporaries and the
 * generation re-check of the three forms are the frame of verify_calls.h; this file's own is the plan, the parser, the tables, the run's arguments
 * (gapsigRunLocked) and the host search.
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

struct PFACX_gapsig_s : pfac_internal::HandleObject {
    size_t numIds = 0;                        /* F of the anchor set it loaded */
    size_t numSigs = 0;                       /* S */
    /* by signature id (entry 0 unused): the handle's pattern id of its anchor, the part that holds it, its offset inside that part, its length */
    std::vector<int> anchorId, anchorPart, anchorOff, anchorLen;
    /* by handle id q: the signatures of its class at sigs[sigOff[q], sigOff[q + 1]), by signature id descending */
    std::vector<unsigned int> sigOff;         /* [F + 2] */
    std::vector<pfac::GapSigEntry> sigs;      /* [S] */
    std::vector<pfac::GapSigPart> parts;      /* the parts of every signature, a signature's in a row */
    std::vector<unsigned int> blob;           /* per part (len + 3) / 4 value dwords, then as many mask dwords; the bytes behind len: mask 0 */
    /* the same on the device, uploaded by the first device call: state of the object (deviceTableBytes), freed by PFACX_gapsigClose */
    pfac::DeviceBuffer<unsigned int> d_sigOff, d_blob;
    pfac::DeviceBuffer<pfac::GapSigEntry> d_sigs;
    pfac::DeviceBuffer<pfac::GapSigPart> d_parts;

    template <class Self, class F> static void forEachDeviceBuffer(Self &self, F f) { f(self.d_sigOff); f(self.d_sigs); f(self.d_parts); f(self.d_blob); }
    PFAC_status_t uploadTables() { return pfac_internal::uploadAll(d_sigOff, sigOff, d_sigs, sigs, d_parts, parts, d_blob, blob); }
    ~PFACX_gapsig_s() override { forEachDeviceBuffer(*this, [](auto &b) { b.release(); }); }
    size_t deviceBytes() const override { size_t n = 0; forEachDeviceBuffer(*this, [&n](const auto &b) { n += b.bytes(); }); return n; }
};

using namespace pfac_internal;

namespace {

constexpr size_t kMaxPartLen = 65535, kMaxGap = 65535, kMaxParts = 64, kDefaultAnchorLen = 32;
constexpr unsigned long long kSpanLimit = 0x7fffffffull;          /* a span of 2^31 - 1 or more is refused */

/* the caller's signatures, copied and canonicalised, with the anchor of each and the anchor set as the reader's text */
struct GapSigPlan {
    std::vector<unsigned char> values, masks;         /* all parts back to back */
    std::vector<size_t> partOff;                      /* [P + 1] into both */
    std::vector<size_t> sigPart;                      /* [S + 1] into partOff */
    std::vector<unsigned int> lo, hi;                 /* [P]: the gap behind a part; 0 behind a signature's last */
    std::vector<int> anchorId, anchorPart, anchorOff, anchorLen;  /* by signature id */
    StringSet anchors;                                /* by handle id - 1: the distinct anchors, and the anchor set as the reader's text */
};

/* The anchor of one signature over its `count` parts: the longest run of bytes with mask 0xFF and a value other than '\n' (the pattern reader
 * splits lines there) inside ONE part, of equal ones the one in the lowest part, then the leftmost, cut to its first maxAnchorLen bytes.
 * false: the signature has no such byte */
bool chooseAnchor(const unsigned char *v, const unsigned char *m, const size_t *partOff, size_t count, size_t maxAnchorLen, size_t *part, size_t *off,
                  size_t *alen)
{
    size_t best = 0, bestPart = 0, bestAt = 0;
    for (size_t j = 0; j < count; j++) {
        const size_t from = partOff[j], len = partOff[j + 1] - from;
        for (size_t i = 0; i < len;) {
            if (m[from + i] != 0xFF || v[from + i] == '\n') { i++; continue; }
            size_t k = i;
            while (k < len && m[from + k] == 0xFF && v[from + k] != '\n') k++;
            if (k - i > best) { best = k - i; bestPart = j; bestAt = i; }
            i = k;
        }
    }
    *part = bestPart;
    *off = bestAt;
    *alen = std::min(best, maxAnchorLen);
    return best > 0;
}

/* The plan of S signatures.  INVALID_PARAMETER with *badSig = the id of the first signature that is refused: no part or more than 64, an empty
 * part or one longer than 65 535 bytes, a gap with lo > hi or hi > 65 535, a slack above 63, a span of 2^31 - 1 or more, no fully specified byte
 * other than '\n' */
PFAC_status_t planSignatures(const unsigned char *h_values, const unsigned char *h_masks, const size_t *h_partOff, const size_t *h_sigPart,
                             const unsigned int *h_gapLo, const unsigned int *h_gapHi, size_t numSigs, size_t maxAnchorLen, GapSigPlan *plan, int *badSig)
{
    const size_t S = numSigs, cut = maxAnchorLen ? maxAnchorLen : kDefaultAnchorLen;
    plan->sigPart.assign(S + 1, 0);
    plan->partOff.assign(1, 0);
    plan->anchorId.assign(S + 1, 0);
    plan->anchorPart.assign(S + 1, 0);
    plan->anchorOff.assign(S + 1, 0);
    plan->anchorLen.assign(S + 1, 0);
    size_t blobWords = 0;
    for (size_t i = 1; i <= S; i++) {
        *badSig = (int)i;
        const size_t first = h_sigPart[i - 1], behind = h_sigPart[i];
        if (behind <= first || behind - first > kMaxParts) return PFAC_STATUS_INVALID_PARAMETER;
        unsigned long long slack = 0, span = 0;
        for (size_t j = first; j < behind; j++) {
            if (h_partOff[j + 1] <= h_partOff[j] || h_partOff[j + 1] - h_partOff[j] > kMaxPartLen) return PFAC_STATUS_INVALID_PARAMETER;
            const size_t len = h_partOff[j + 1] - h_partOff[j];
            const bool last = j + 1 == behind;
            const unsigned int lo = last ? 0u : h_gapLo[j], hi = last ? 0u : h_gapHi[j];
            if (lo > hi || hi > kMaxGap) return PFAC_STATUS_INVALID_PARAMETER;
            slack += hi - lo;
            span += len + hi;
            plan->partOff.push_back(plan->partOff.back() + len);
            plan->lo.push_back(lo);
            plan->hi.push_back(hi);
            blobWords += 2 * ((len + 3) / 4);
        }
        if (slack > PFACX_GAPSIG_MAX_SLACK || span >= kSpanLimit) return PFAC_STATUS_INVALID_PARAMETER;
        plan->sigPart[i] = plan->sigPart[i - 1] + (behind - first);
    }
    *badSig = 0;
    if (blobWords > kMaxInt || plan->lo.size() > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;          /* the tables index parts and blob with ints */
    plan->values.resize(plan->partOff.back());
    plan->masks.resize(plan->partOff.back());
    for (size_t i = 1; i <= S; i++) {
        const size_t first = plan->sigPart[i - 1], count = plan->sigPart[i] - first;
        for (size_t j = 0; j < count; j++) {
            const size_t from = h_partOff[h_sigPart[i - 1] + j], at = plan->partOff[first + j], len = plan->partOff[first + j + 1] - at;
            for (size_t k = 0; k < len; k++) {
                plan->masks[at + k] = h_masks[from + k];
                plan->values[at + k] = (unsigned char)(h_values[from + k] & h_masks[from + k]);
            }
        }
        size_t apart = 0, aoff = 0, alen = 0;
        if (!chooseAnchor(plan->values.data(), plan->masks.data(), plan->partOff.data() + first, count, cut, &apart, &aoff, &alen)) {
            *badSig = (int)i;
            return PFAC_STATUS_INVALID_PARAMETER;
        }
        plan->anchorId[i] = plan->anchors.idOf(std::string(reinterpret_cast<const char *>(plan->values.data()) + plan->partOff[first + apart] + aoff, alen));
        plan->anchorPart[i] = (int)apart;
        plan->anchorOff[i] = (int)aoff;
        plan->anchorLen[i] = (int)alen;
    }
    return PFAC_STATUS_SUCCESS;
}

/* the tables of `sg` from the plan: the classes by handle id, each by signature id descending, the parts and the blob */
void buildTables(const GapSigPlan &plan, PFACX_gapsig_s *sg)
{
    const size_t S = plan.sigPart.size() - 1, F = plan.anchors.size(), P = plan.lo.size();
    sg->numIds = F;
    sg->numSigs = S;
    sg->anchorId = plan.anchorId;
    sg->anchorPart = plan.anchorPart;
    sg->anchorOff = plan.anchorOff;
    sg->anchorLen = plan.anchorLen;
    sg->parts.assign(P, pfac::GapSigPart{0, 0, 0, 0});
    sg->blob.clear();
    for (size_t j = 0; j < P; j++) {
        const size_t at = plan.partOff[j], len = plan.partOff[j + 1] - at, words = (len + 3) / 4, blobAt = sg->blob.size();
        sg->blob.resize(blobAt + 2 * words, 0u);
        std::memcpy(sg->blob.data() + blobAt, plan.values.data() + at, len);
        std::memcpy(sg->blob.data() + blobAt + words, plan.masks.data() + at, len);
        sg->parts[j] = pfac::GapSigPart{(unsigned int)len, (unsigned int)blobAt, plan.lo[j], plan.hi[j]};
    }
    sg->sigOff.assign(F + 2, 0u);
    for (size_t i = 1; i <= S; i++) sg->sigOff[(size_t)plan.anchorId[i] + 1]++;
    for (size_t q = 1; q <= F + 1; q++) sg->sigOff[q] += sg->sigOff[q - 1];      /* sigOff[q + 1] = the end of class q; sigOff[q]: its start */
    std::vector<unsigned int> next(sg->sigOff.begin(), sg->sigOff.end());
    sg->sigs.assign(S, pfac::GapSigEntry{0, 0, 0, 0});
    for (size_t i = S; i >= 1; i--) {                                              /* id descending within every class */
        const size_t first = plan.sigPart[i - 1], count = plan.sigPart[i] - first;
        sg->sigs[next[(size_t)plan.anchorId[i]]++] =
            pfac::GapSigEntry{(int)i, (unsigned int)first, (unsigned int)count | (unsigned int)plan.anchorPart[i] << 16, (unsigned int)plan.anchorOff[i]};
    }
}

/* what parseText puts together */
struct ParsedText {
    std::vector<unsigned char> values, masks;
    std::vector<size_t> partOff{0}, sigPart{0};
    std::vector<unsigned int> lo, hi;                   /* one entry per part */
};

/* the text of PFACX_gapsigOpenText into CSR arrays; false with *badLine = the 1-based line that is refused */
bool parseText(const char *text, size_t size, ParsedText &out, int *badLine)
{
    const auto nibble = [](char c) -> int {          /* 0 .. 15, 16: '?', -1: neither */
        if (c >= '0' && c <= '9') return c - '0';
        if (c >= 'a' && c <= 'f') return c - 'a' + 10;
        if (c >= 'A' && c <= 'F') return c - 'A' + 10;
        return c == '?' ? 16 : -1;
    };
    size_t line = 1;
    for (size_t i = 0; i < size; line++) {
        *badLine = (int)std::min(line, kMaxInt);
        const void *nl = std::memchr(text + i, '\n', size - i);
        if (!nl) return false;                                                 /* bytes behind the last '\n' */
        const size_t stop = (size_t)(static_cast<const char *>(nl) - text);
        size_t end = stop;
        if (end > i && text[end - 1] == '\r') end--;
        bool gapOpen = false;                                                  /* a gap token stands behind the last byte pair */
        size_t partStart = out.values.size();
        for (size_t j = i; j < end;) {
            if (text[j] == ' ' || text[j] == '\t') { j++; continue; }
            if (text[j] == '{' || text[j] == '[') {
                /* {n}, {n-m}, {-m}: digits, at most one '-', a number behind it; the closing character matches the opening one */
                const char close = text[j] == '{' ? '}' : ']';
                if (gapOpen || out.values.size() == partStart) return false;    /* two gaps in a row, or a gap at the start of the line */
                unsigned long num[2] = {0, 0};
                bool have[2] = {false, false};
                int which = 0;
                for (j++; j < end && text[j] != close; j++) {
                    if (text[j] == '-' && which == 0) { which = 1; continue; }
                    if (text[j] < '0' || text[j] > '9') return false;
                    num[which] = num[which] * 10 + (unsigned long)(text[j] - '0');
                    if (num[which] > kMaxGap) return false;
                    have[which] = true;
                }
                if (j >= end) return false;                                     /* no closing character */
                j++;
                if (which == 0 ? !have[0] : !have[1]) return false;             /* {}, {n-} and {-}: an unbounded gap, or none */
                const unsigned long lo = which == 0 || have[0] ? num[0] : 0ul, hi = which == 0 ? num[0] : num[1];
                if (lo > hi) return false;
                out.partOff.push_back(out.values.size());
                out.lo.push_back((unsigned int)lo);
                out.hi.push_back((unsigned int)hi);
                partStart = out.values.size();
                gapOpen = true;
                continue;
            }
            const int hi = nibble(text[j]), lo = j + 1 < end ? nibble(text[j + 1]) : -1;
            if (hi < 0 || lo < 0) return false;                                 /* another character ('*' among them), or a digit without its partner */
            out.values.push_back((unsigned char)((hi < 16 ? hi << 4 : 0) | (lo < 16 ? lo : 0)));
            out.masks.push_back((unsigned char)((hi < 16 ? 0xF0 : 0) | (lo < 16 ? 0x0F : 0)));
            gapOpen = false;
            j += 2;
        }
        if (gapOpen || out.values.size() == partStart) return false;            /* a gap at the end of the line, or an empty line */
        out.partOff.push_back(out.values.size());
        out.lo.push_back(0u);
        out.hi.push_back(0u);
        out.sigPart.push_back(out.lo.size());
        i = stop + 1;
    }
    *badLine = 0;
    return true;
}

/* the passes over `count` ordered longest pairs, behind the argument checks; the caller holds c->lock */
PFAC_status_t gapsigRunLocked(PFACX_gapsig_s *sg, const VerifyCall &call, int *d_end, const int *d_pairIds, const int *d_pairPos, size_t count)
{
    PFACX_gapsigRun_t run{};
    const PFAC_status_t st = fillRunFrame(sg, call, d_pairIds, d_pairPos, count, &run.v);
    if (st != PFAC_STATUS_SUCCESS) return st;
    run.d_sigOff = sg->d_sigOff.get();
    run.d_sigs = sg->d_sigs.get();
    run.numSigs = sg->sigs.size();
    run.d_parts = sg->d_parts.get();
    run.numParts = sg->parts.size();
    run.d_end = d_end;
    return finishRun(sg->handle, sg->handle->gapsig_run_ptr, run, call);
}

/* The three functions below are scan_gapsig.hip's search written out once more for the host, step for step: the host form and the device forms
 * share the algorithm, so their agreeing with each other is no evidence of either.  What they are checked against is tests/gapsig_ref.py, which
 * shares nothing with them (a recursion over every gap width, sets of offsets for the owner, Python's re). */
/* scan_gapsig.hip's smear: the OR of m << k for k = 0 .. w, w <= 63 */
uint64_t smear(uint64_t m, unsigned int w)
{
    unsigned int c = 1;
    while (2u * c <= w + 1u) {
        m |= m << c;
        c *= 2u;
    }
    return m | m << (w + 1u - c);
}

/* scan_gapsig.hip's holdsWhere with a plain byte loop: the bits t of m at which part q holds at offset base + dir * t inside [0, n) */
uint64_t holdsWhere(const PFACX_gapsig_s &sg, const unsigned char *in, size_t n, const pfac::GapSigPart &q, long long base, int dir, uint64_t m)
{
    const size_t len = q.len;
    const unsigned char *val = reinterpret_cast<const unsigned char *>(sg.blob.data()) + 4 * (size_t)q.blobOff, *mask = val + 4 * ((len + 3) / 4);
    uint64_t held = 0;
    for (int t = 0; t < 64; t++) {
        if (!(m >> t & 1ull)) continue;
        const long long o = base + (long long)dir * t;
        if (o < 0 || o + (long long)len > (long long)n) continue;
        size_t k = 0;
        while (k < len && ((in[(size_t)o + k] ^ val[k]) & mask[k]) == 0) k++;
        if (k == len) held |= 1ull << t;
    }
    return held;
}

/* scan_gapsig.hip's searchSignature: emit(start, end) for what the anchor occurrence at p owns of signature e, starts ascending */
template <class Emit>
void searchOnHost(const PFACX_gapsig_s &sg, const unsigned char *in, size_t n, const pfac::GapSigEntry &e, int p, Emit emit)
{
    const unsigned int count = e.partsAnchor & 0xFFFFu, anchor = e.partsAnchor >> 16;
    if (e.anchorOff > (unsigned int)p) return;                                     /* it would lie in front of the input */
    const pfac::GapSigPart *parts = sg.parts.data() + e.firstPart;
    const long long x = (long long)p - (long long)e.anchorOff;
    uint64_t back = holdsWhere(sg, in, n, parts[anchor], x, -1, 1ull);
    long long tight = x;
    for (unsigned int j = anchor; j > 0u && back != 0ull; j--) {
        const pfac::GapSigPart &q = parts[j - 1u];
        tight -= (long long)q.len + (long long)q.lo;
        back = holdsWhere(sg, in, n, q, tight, -1, smear(back, q.hi - q.lo));
    }
    for (int tb = 63; tb >= 0; tb--) {                                             /* the starts, ascending */
        if (!(back >> tb & 1ull)) continue;
        const long long s = tight - tb;
        uint64_t all = 1ull;
        long long at = s;
        for (unsigned int j = 0; j < anchor && all != 0ull; j++) {
            const pfac::GapSigPart &q = parts[j];
            at += (long long)q.len + (long long)q.lo;
            all = holdsWhere(sg, in, n, parts[j + 1u], at, 1, smear(all, q.hi - q.lo));
        }
        const long long tx = x - at;
        if (tx < 0 || tx > 63) continue;
        uint64_t eq = all & (1ull << tx), lt = all & ((1ull << tx) - 1ull);
        for (unsigned int j = anchor; j + 1u < count && eq != 0ull; j++) {
            const pfac::GapSigPart &q = parts[j];
            const unsigned int w = q.hi - q.lo;
            at += (long long)q.len + (long long)q.lo;
            all = holdsWhere(sg, in, n, parts[j + 1u], at, 1, smear(all, w));
            lt = smear(lt, w) & all;
            eq = smear(eq, w) & all;
        }
        if (eq == 0ull || lt != 0ull) continue;                                    /* not on an embedding at s, or a nearer anchor occurrence owns it */
        emit((int)s, (int)(at + __builtin_ctzll(all) + (long long)parts[count - 1u].len));
    }
}

/* The host loop: what the chains of `count` ordered longest pairs own into ids / pos / end (slots >= capacity are not written; end may be
 * null); returns the full length of the list */
size_t gapsigOnHost(const pfac::Automaton &fa, const PFACX_gapsig_s &sg, const unsigned char *in, size_t n, const int *pairIds, const int *pairPos,
                    size_t count, int *ids, int *pos, int *end, size_t capacity)
{
    size_t total = 0;
    for (size_t i = 0; i < count; i++) {
        const int p = pairPos[i];
        if (p < 0 || (size_t)p >= n) continue;
        forEachChainMember(fa, pairIds[i], [&](int q) {                       /* (the caller's pin: fa.numPatterns == sg.numIds) */
            for (size_t v = sg.sigOff[(size_t)q]; v < sg.sigOff[(size_t)q + 1]; v++) {
                const pfac::GapSigEntry &e = sg.sigs[v];
                searchOnHost(sg, in, n, e, p, [&](int s, int behind) {
                    if (total < capacity) {
                        ids[total] = e.id;
                        pos[total] = s;
                        if (end) end[total] = behind;
                    }
                    total++;
                });
            }
            return true;
        });
    }
    return total;
}

} // namespace

extern "C" {

PFAC_status_t PFACX_gapsigOpen(PFAC_handle_t handle, const unsigned char *h_values, const unsigned char *h_masks, const size_t *h_partOff,
                               const size_t *h_sigPart, const unsigned int *h_gapLo, const unsigned int *h_gapHi, size_t numSigs, size_t maxAnchorLen,
                               PFACX_gapsig_t *sig, int *badSig)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!sig) return PFAC_STATUS_INVALID_PARAMETER;
    *sig = nullptr;
    int bad = 0;
    if (badSig) *badSig = 0;
    if (!h_values || !h_masks || !h_partOff || !h_sigPart || !h_gapLo || !h_gapHi || numSigs == 0 || numSigs >= kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;
    GapSigPlan plan;
    try {
        const PFAC_status_t st = planSignatures(h_values, h_masks, h_partOff, h_sigPart, h_gapLo, h_gapHi, numSigs, maxAnchorLen, &plan, &bad);
        if (badSig) *badSig = bad;
        if (st != PFAC_STATUS_SUCCESS) return st;                             /* nothing of the handle has changed */
    } catch (const std::bad_alloc &) { return PFAC_STATUS_ALLOC_FAILED; }
    return adoptOverStrings(handle, plan.anchors, sig, [&](PFACX_gapsig_s &obj) -> PFAC_status_t {    /* (verify_calls.h: the tables hold only over the anchors) */
        buildTables(plan, &obj);
        return PFAC_STATUS_SUCCESS;
    });
}

PFAC_status_t PFACX_gapsigOpenText(PFAC_handle_t handle, const char *text, size_t size, size_t maxAnchorLen, PFACX_gapsig_t *sig, int *badLine)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!sig) return PFAC_STATUS_INVALID_PARAMETER;
    *sig = nullptr;
    int bad = 0;
    if (badLine) *badLine = 0;
    if (!text) return PFAC_STATUS_INVALID_PARAMETER;
    ParsedText parsed;
    try {
        const bool ok = parseText(text, size, parsed, &bad);
        if (badLine) *badLine = bad;
        if (!ok || parsed.sigPart.size() < 2) return PFAC_STATUS_INVALID_PARAMETER;  /* (no line at all: numSigs == 0) */
    } catch (const std::bad_alloc &) { return PFAC_STATUS_ALLOC_FAILED; }
    /* a line is a signature: the id the binary form refuses is the line */
    return PFACX_gapsigOpen(handle, parsed.values.data(), parsed.masks.data(), parsed.partOff.data(), parsed.sigPart.data(), parsed.lo.data(),
                            parsed.hi.data(), parsed.sigPart.size() - 1, maxAnchorLen, sig, badLine);
}

PFAC_status_t PFACX_gapsigClose(PFACX_gapsig_t sig) { return closeObject(sig); }

PFAC_status_t PFACX_gapsigGetAnchors(PFACX_gapsig_t sig, int *h_anchorId, int *h_anchorPart, int *h_anchorOff, int *h_anchorLen, size_t n)
{
    if (!sig || !sig->handle) return PFAC_STATUS_INVALID_HANDLE;
    PFAC_context *c = sig->handle;
    std::lock_guard<std::mutex> guard(c->lock);
    const PFAC_status_t st = checkSetGeneration(c, sig->generation);
    if (st != PFAC_STATUS_SUCCESS) return st;
    if (n < sig->numSigs + 1) return PFAC_STATUS_INVALID_PARAMETER;
    const size_t bytes = (sig->numSigs + 1) * sizeof(int);
    if (h_anchorId) std::memcpy(h_anchorId, sig->anchorId.data(), bytes);
    if (h_anchorPart) std::memcpy(h_anchorPart, sig->anchorPart.data(), bytes);
    if (h_anchorOff) std::memcpy(h_anchorOff, sig->anchorOff.data(), bytes);
    if (h_anchorLen) std::memcpy(h_anchorLen, sig->anchorLen.data(), bytes);
    return PFAC_STATUS_SUCCESS;
}

PFAC_status_t PFACX_gapsigMatchFromDevice(PFACX_gapsig_t sig, char *d_input, size_t size, int *d_ids, int *d_pos, int *d_end, size_t capacity,
                                          size_t *h_num_matched)
{
    const VerifyCall call{d_input, size, d_ids, d_pos, capacity, h_num_matched};
    return verifyFromDevice(sig, call, [&](const int *ids, const int *pos, size_t count) { return gapsigRunLocked(sig, call, d_end, ids, pos, count); });
}

PFAC_status_t PFACX_gapsigMatchFromHost(PFACX_gapsig_t sig, char *h_input, size_t size, int *h_ids, int *h_pos, int *h_end, size_t capacity,
                                        size_t *h_num_matched)
{
    const VerifyCall call{h_input, size, h_ids, h_pos, capacity, h_num_matched};
    return verifyFromHost(sig, call, [&](const int *ids, const int *pos, size_t count) {
        return gapsigOnHost(sig->handle->fa, *sig, reinterpret_cast<const unsigned char *>(h_input), size, ids, pos, count, h_ids, h_pos, h_end, capacity);
    });
}

PFAC_status_t PFACX_gapsigPairsFromDevice(PFACX_gapsig_t sig, const char *d_input, size_t size, const int *d_pairIds, const int *d_pairPos,
                                          size_t numPairs, int *d_ids, int *d_pos, int *d_end, size_t capacity, size_t *h_num_matched)
{
    const VerifyCall call{d_input, size, d_ids, d_pos, capacity, h_num_matched};
    return verifyPairsFromDevice(sig, call, d_pairIds, d_pairPos, numPairs, {d_ids, d_pos, d_end}, [&](const int *ids, const int *pos, size_t count) {
        return gapsigRunLocked(sig, call, d_end, ids, pos, count);
    });
}

} /* extern "C" */
