/*
 * clsig_api.cpp -- PFACX_clsigOpen / PFACX_clsigOpenText / PFACX_clsigGetAnchors / PFACX_clsigClose / PFACX_clsigMatchFromDevice /
 * ...FromHost / PFACX_clsigPairsFromDevice (include/pfac_ext.h): signatures of byte classes with bounded repeats.
 *
 * A signature is a sequence of elements (class, lo, hi).  PFACX_clsigOpen copies the caller's arrays, checks every element, FUSES the maximal
 * runs of one-byte classes with lo == hi into literal parts and checks the limits (planSignatures: parts, slack, literal length, span), picks one
 * run inside one literal part of each signature as its ANCHOR (chooseAnchor: the longest run of bytes other than '\n', of equal ones the one in the
 * lowest part, then the leftmost, cut to its first maxAnchorLen bytes), loads the distinct anchors into the handle through the reader every
 * pattern set goes through -- one line per anchor, in order of first appearance, so handle id q is the q-th distinct anchor -- and builds per
 * handle id q the signatures of its class (buildTables): {signature id, first part, parts | anchor part << 16, anchorOff} {notBefore, notAfter} by
 * id descending, in CSR form by q, the parts {0, len, blobOff} / {1, class, lo, hi}, a dword-aligned blob of the literal parts' bytes and the
 * class table.  PFACX_clsigOpenText is a parser in front of it (parseText).  All three match forms work on the LONGEST pairs of the anchor set
 * and walk each pair's prefix chain, member by member through its class; per (anchor occurrence, signature) they run the search that
 * scan_clsig.hip's header describes.  The host form's search (searchOnHost) is written on its own: a part step there is a loop over the set bits
 * with a run counted from each, not the kernel's one walk over the window.  The device form runs the unchanged compacted-output path with its
 * ordered pairs in handle scratch (PFACX_allReduce) and the passes of scan_clsig.hip (PFACX_clsigRun) behind it; the pairs form runs those
 * passes over a list of the caller's.  The host form takes the longest pairs from hostLongestPairs into a temporary of its own (clsigOnHost).
 * The three batch forms (PFACX_clsigBatch*) are the same three functions with offsets: the scan stays the plain one over the whole buffer, the
 * device passes get the offsets and clamp them (scan_clsig.hip), the host loop finds each pair's segment in the validated offsets and searches
 * that segment's bytes as if they were the whole input.
 * The open tail (the anchors loaded and the handle checked to hold them), the order of the checks, the scan, the pair temporaries and the
 * generation re-check of the three forms, plain and batch, are the frame of verify_calls.h (ClSigForms hands it the segments' check and the
 * all-zero segFirst of an empty list); this file's own is the plan, the parser, the tables, the run's arguments (clsigRunLocked) and the host search.
 */
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "pfac_host.h"
#include "verify_calls.h"

struct PFACX_clsig_s : pfac_internal::HandleObject {
    size_t numIds = 0;                        /* F of the anchor set it loaded */
    size_t numSigs = 0;                       /* S */
    unsigned int flags = 0;                   /* PFACX_CLSIG_SHORTEST_END */
    /* by signature id (entry 0 unused): the handle's pattern id of its anchor, the part that holds it, its offset inside that part, its length */
    std::vector<int> anchorId, anchorPart, anchorOff, anchorLen;
    /* by handle id q: the signatures of its class at sigs[sigOff[q], sigOff[q + 1]), by signature id descending */
    std::vector<unsigned int> sigOff;         /* [F + 2] */
    std::vector<pfac::ClSigEntry> sigs;       /* [S] */
    std::vector<pfac::ClSigPart> parts;       /* the parts of every signature, a signature's in a row */
    std::vector<unsigned int> blob;           /* per literal part (len + 3) / 4 value dwords */
    std::vector<unsigned int> classes;        /* [8 numClasses] */
    /* the same on the device, uploaded by the first device call: state of the object (deviceTableBytes), freed by PFACX_clsigClose */
    pfac::DeviceBuffer<unsigned int> d_sigOff, d_blob, d_classes;
    pfac::DeviceBuffer<pfac::ClSigEntry> d_sigs;
    pfac::DeviceBuffer<pfac::ClSigPart> d_parts;

    template <class Self, class F> static void forEachDeviceBuffer(Self &self, F f)
    {
        f(self.d_sigOff); f(self.d_sigs); f(self.d_parts); f(self.d_blob); f(self.d_classes);
    }
    PFAC_status_t uploadTables()
    {
        return pfac_internal::uploadAll(d_sigOff, sigOff, d_sigs, sigs, d_parts, parts, d_blob, blob, d_classes, classes);
    }
    ~PFACX_clsig_s() override { forEachDeviceBuffer(*this, [](auto &b) { b.release(); }); }
    size_t deviceBytes() const override { size_t n = 0; forEachDeviceBuffer(*this, [&n](const auto &b) { n += b.bytes(); }); return n; }
};

using namespace pfac_internal;

namespace {

constexpr size_t kMaxRepeat = 65535, kMaxParts = 64, kMaxClasses = 65535, kDefaultAnchorLen = 32;
constexpr unsigned long long kSpanLimit = 1ull << 23;             /* a span of 2^23 or more is refused */

using ByteClass = std::array<unsigned int, 8>;

bool inClass(const unsigned int *cls, unsigned int b) { return (cls[b >> 5] >> (b & 31u) & 1u) != 0u; }

/* one part after fusion */
struct PlanPart {
    bool literal = false;
    std::string bytes;                                /* a literal part's */
    unsigned int cls = 0, lo = 0, hi = 0;             /* a class part's */
};

/* the caller's signatures, checked and fused, with the anchor of each and the anchor set as the reader's text */
struct ClSigPlan {
    std::vector<PlanPart> parts;                      /* all parts, a signature's in a row */
    std::vector<size_t> sigPart;                      /* [S + 1] into parts */
    std::vector<int> notBefore, notAfter;             /* by signature id - 1 */
    std::vector<int> anchorId, anchorPart, anchorOff, anchorLen;  /* by signature id */
    StringSet anchors;                                /* by handle id - 1: the distinct anchors, and the anchor set as the reader's text */
};

/* The anchor of one signature over its `count` parts: the longest run of bytes other than '\n' (the pattern reader splits lines there) inside ONE
 * literal part, of equal ones the one in the lowest part, then the leftmost, cut to its first maxAnchorLen bytes.  false: there is no such byte */
bool chooseAnchor(const PlanPart *parts, size_t count, size_t maxAnchorLen, size_t *part, size_t *off, size_t *alen)
{
    size_t best = 0, bestPart = 0, bestAt = 0;
    for (size_t j = 0; j < count; j++) {
        if (!parts[j].literal) continue;
        const std::string &b = parts[j].bytes;
        for (size_t i = 0; i < b.size();) {
            if (b[i] == '\n') { i++; continue; }
            size_t k = i;
            while (k < b.size() && b[k] != '\n') k++;
            if (k - i > best) { best = k - i; bestPart = j; bestAt = i; }
            i = k;
        }
    }
    *part = bestPart;
    *off = bestAt;
    *alen = std::min(best, maxAnchorLen);
    return best > 0;
}

/* The plan of S signatures over a class table that has been checked (single[c]: the one byte of class c, or -1).  INVALID_PARAMETER with *badSig =
 * the id of the first signature that is refused: the header (pfac_ext.h: PFACX_clsigOpen) lists why */
PFAC_status_t planSignatures(const std::vector<int> &single, const unsigned int *h_elemClass, const unsigned int *h_elemLo, const unsigned int *h_elemHi,
                             const size_t *h_sigElem, const int *h_notBefore, const int *h_notAfter, size_t numSigs, size_t maxAnchorLen, ClSigPlan *plan,
                             int *badSig)
{
    const size_t S = numSigs, C = single.size(), cut = maxAnchorLen ? maxAnchorLen : kDefaultAnchorLen;
    plan->sigPart.assign(1, 0);
    plan->anchorId.assign(S + 1, 0);
    plan->anchorPart.assign(S + 1, 0);
    plan->anchorOff.assign(S + 1, 0);
    plan->anchorLen.assign(S + 1, 0);
    for (size_t i = 1; i <= S; i++) {
        *badSig = (int)i;
        const size_t first = h_sigElem[i - 1], behind = h_sigElem[i];
        if (behind <= first) return PFAC_STATUS_INVALID_PARAMETER;
        const int nb = h_notBefore ? h_notBefore[i - 1] : -1, na = h_notAfter ? h_notAfter[i - 1] : -1;
        if (nb < -1 || na < -1 || (nb >= 0 && (size_t)nb >= C) || (na >= 0 && (size_t)na >= C)) return PFAC_STATUS_INVALID_PARAMETER;
        unsigned long long slack = 0, span = 0;
        size_t count = 0;
        bool open = false;                            /* the last part is a literal part that the next fixed one-byte element extends */
        for (size_t k = first; k < behind; k++) {
            const unsigned int c = h_elemClass[k], lo = h_elemLo[k], hi = h_elemHi[k];
            if (c >= C || lo > hi || hi == 0 || hi > kMaxRepeat) return PFAC_STATUS_INVALID_PARAMETER;
            slack += hi - lo;
            span += hi;
            if (slack > PFACX_CLSIG_MAX_SLACK || span >= kSpanLimit) return PFAC_STATUS_INVALID_PARAMETER;
            if (single[c] >= 0 && lo == hi) {
                if (!open) {
                    if (++count > kMaxParts) return PFAC_STATUS_INVALID_PARAMETER;
                    plan->parts.emplace_back();
                    plan->parts.back().literal = true;
                    open = true;
                }
                std::string &bytes = plan->parts.back().bytes;
                if (bytes.size() + lo > kMaxRepeat) return PFAC_STATUS_INVALID_PARAMETER;
                bytes.append((size_t)lo, (char)single[c]);
            } else {
                if (++count > kMaxParts) return PFAC_STATUS_INVALID_PARAMETER;
                plan->parts.emplace_back();
                plan->parts.back().cls = c;
                plan->parts.back().lo = lo;
                plan->parts.back().hi = hi;
                open = false;
            }
        }
        plan->sigPart.push_back(plan->parts.size());
        plan->notBefore.push_back(nb);
        plan->notAfter.push_back(na);
    }
    *badSig = 0;
    if (plan->parts.size() > kMaxInt) return PFAC_STATUS_INVALID_PARAMETER;                            /* the tables index the parts with ints */
    for (size_t i = 1; i <= S; i++) {
        const size_t first = plan->sigPart[i - 1], count = plan->sigPart[i] - first;
        size_t apart = 0, aoff = 0, alen = 0;
        if (!chooseAnchor(plan->parts.data() + first, count, cut, &apart, &aoff, &alen)) {
            *badSig = (int)i;
            return PFAC_STATUS_INVALID_PARAMETER;
        }
        plan->anchorId[i] = plan->anchors.idOf(plan->parts[first + apart].bytes.substr(aoff, alen));
        plan->anchorPart[i] = (int)apart;
        plan->anchorOff[i] = (int)aoff;
        plan->anchorLen[i] = (int)alen;
    }
    return PFAC_STATUS_SUCCESS;
}

/* the tables of `sg` from the plan: the classes of signatures by handle id, each by signature id descending, the parts and the blob; false: the
 * blob would pass what an int indexes */
bool buildTables(const ClSigPlan &plan, PFACX_clsig_s *sg)
{
    const size_t S = plan.sigPart.size() - 1, F = plan.anchors.size(), P = plan.parts.size();
    sg->numIds = F;
    sg->numSigs = S;
    sg->anchorId = plan.anchorId;
    sg->anchorPart = plan.anchorPart;
    sg->anchorOff = plan.anchorOff;
    sg->anchorLen = plan.anchorLen;
    sg->parts.assign(P, pfac::ClSigPart{0, 0, 0, 0});
    sg->blob.clear();
    for (size_t j = 0; j < P; j++) {
        const PlanPart &p = plan.parts[j];
        if (!p.literal) {
            sg->parts[j] = pfac::ClSigPart{1u, p.cls, p.lo, p.hi};
            continue;
        }
        const size_t len = p.bytes.size(), words = (len + 3) / 4, blobAt = sg->blob.size();
        if (blobAt + words > kMaxInt) return false;
        sg->blob.resize(blobAt + words, 0u);
        std::memcpy(sg->blob.data() + blobAt, p.bytes.data(), len);
        sg->parts[j] = pfac::ClSigPart{0u, (unsigned int)len, (unsigned int)blobAt, 0u};
    }
    sg->sigOff.assign(F + 2, 0u);
    for (size_t i = 1; i <= S; i++) sg->sigOff[(size_t)plan.anchorId[i] + 1]++;
    for (size_t q = 1; q <= F + 1; q++) sg->sigOff[q] += sg->sigOff[q - 1];      /* sigOff[q + 1] = the end of class q; sigOff[q]: its start */
    std::vector<unsigned int> next(sg->sigOff.begin(), sg->sigOff.end());
    sg->sigs.assign(S, pfac::ClSigEntry{0, 0, 0, 0, -1, -1, {0, 0}});
    for (size_t i = S; i >= 1; i--) {                                              /* id descending within every class */
        const size_t first = plan.sigPart[i - 1], count = plan.sigPart[i] - first;
        sg->sigs[next[(size_t)plan.anchorId[i]]++] =
            pfac::ClSigEntry{(int)i, (unsigned int)first, (unsigned int)count | (unsigned int)plan.anchorPart[i] << 16, (unsigned int)plan.anchorOff[i],
                             plan.notBefore[i - 1], plan.notAfter[i - 1], {0u, 0u}};
    }
    return true;
}

/* ------------------------------------------------------------------ the text form */

/* what parseText puts together */
struct ParsedText {
    std::vector<unsigned int> classes;                  /* 8 words per distinct class */
    std::map<ByteClass, unsigned int> known;
    std::vector<unsigned int> elemClass, lo, hi;
    std::vector<size_t> sigElem{0};
    std::vector<int> notBefore, notAfter;

    unsigned int classOf(const ByteClass &c)
    {
        const auto placed = known.emplace(c, (unsigned int)known.size());
        if (placed.second) classes.insert(classes.end(), c.begin(), c.end());
        return placed.first->second;
    }
};

void addByte(ByteClass &c, unsigned int b) { c[b >> 5] |= 1u << (b & 31u); }
void addRange(ByteClass &c, unsigned int from, unsigned int to) { for (unsigned int b = from; b <= to; b++) addByte(c, b); }
bool isEmpty(const ByteClass &c) { return std::all_of(c.begin(), c.end(), [](unsigned int w) { return w == 0u; }); }
void invert(ByteClass &c) { for (unsigned int &w : c) w = ~w; }

int hexDigit(char c)
{
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

/* the escape behind the '\' at text[j - 1], j < end: one byte (the return value, 0 .. 255) or a class escape (256, added to *cls), -1: unknown.
 * inSet: `\-` is an escape too.  j moves behind it */
int parseEscape(const char *text, size_t &j, size_t end, bool inSet, ByteClass *cls)
{
    const char e = text[j++];
    switch (e) {
    case 'n': return '\n';
    case 'r': return '\r';
    case 't': return '\t';
    case 'f': return '\f';
    case 'v': return '\v';
    case '0': return j < end && text[j] >= '0' && text[j] <= '9' ? -1 : 0;      /* (an octal escape of more digits: not in the subset) */
    case 'x': {
        if (end - j < 2 || hexDigit(text[j]) < 0 || hexDigit(text[j + 1]) < 0) return -1;
        const int b = hexDigit(text[j]) * 16 + hexDigit(text[j + 1]);
        j += 2;
        return b;
    }
    case 'd': case 'D': case 'w': case 'W': case 's': case 'S': {
        ByteClass c{};
        if (e == 'd' || e == 'D') addRange(c, '0', '9');
        if (e == 'w' || e == 'W') { addRange(c, '0', '9'); addRange(c, 'A', 'Z'); addRange(c, 'a', 'z'); addByte(c, '_'); }
        if (e == 's' || e == 'S') { addByte(c, ' '); addRange(c, '\t', '\r'); }   /* \t \n \v \f \r are 9 .. 13 */
        if (e == 'D' || e == 'W' || e == 'S') invert(c);
        for (size_t w = 0; w < 8; w++) (*cls)[w] |= c[w];
        return 256;
    }
    default:
        if (std::strchr("\\.[](){}?*+|^$", e) != nullptr && e != '\0') return (unsigned char)e;
        if (inSet && e == '-') return '-';
        return -1;
    }
}

/* the body of a bracket set behind its '[' at text[j - 1] up to and over its ']' into *out; false: unclosed, empty, a descending range, an unknown
 * escape, a class escape as the end of a range */
bool parseSet(const char *text, size_t &j, size_t end, ByteClass *out)
{
    ByteClass c{};
    bool negated = false;
    if (j < end && text[j] == '^') { negated = true; j++; }
    for (;;) {
        if (j >= end) return false;                                              /* unclosed */
        if (text[j] == ']') { j++; break; }
        int from;
        if (text[j] == '\\') {
            if (++j >= end) return false;
            from = parseEscape(text, j, end, true, &c);
            if (from < 0) return false;
        } else {
            from = (unsigned char)text[j++];
        }
        if (j + 1 < end && text[j] == '-' && text[j + 1] != ']') {              /* a range: a '-' that is not the last place */
            if (from > 255) return false;
            j++;
            int to;
            if (text[j] == '\\') {
                if (++j >= end) return false;
                ByteClass none{};
                to = parseEscape(text, j, end, true, &none);
                if (to < 0 || to > 255) return false;
            } else {
                to = (unsigned char)text[j++];
            }
            if (to < from) return false;
            addRange(c, (unsigned int)from, (unsigned int)to);
        } else if (from <= 255) {
            addByte(c, (unsigned int)from);
        }
    }
    if (isEmpty(c)) return false;                                                /* `[]`, `[^]`: to re the ']' there is a literal */
    if (negated) invert(c);
    if (isEmpty(c)) return false;
    *out = c;
    return true;
}

/* `(?<![set])` / `(?![set])` at text[j ...]: its class; false: something else */
bool parseBoundary(const char *text, size_t &j, size_t end, const char *opening, ByteClass *out)
{
    const size_t open = std::strlen(opening);
    if (end - j < open || std::memcmp(text + j, opening, open) != 0) return false;
    j += open;
    if (!parseSet(text, j, end, out)) return false;
    if (j >= end || text[j] != ')') return false;
    j++;
    return true;
}

/* a decimal number of at least one digit at text[j ...], at most 65 535 */
bool parseNumber(const char *text, size_t &j, size_t end, unsigned int *out)
{
    if (j >= end || text[j] < '0' || text[j] > '9') return false;
    unsigned long v = 0;
    for (; j < end && text[j] >= '0' && text[j] <= '9'; j++) {
        v = v * 10 + (unsigned long)(text[j] - '0');
        if (v > kMaxRepeat) return false;
    }
    *out = (unsigned int)v;
    return true;
}

/* the text of PFACX_clsigOpenText into the arrays of the binary form; false with *badLine = the 1-based line that is refused */
bool parseText(const char *text, size_t size, ParsedText &out, int *badLine)
{
    size_t line = 1;
    for (size_t i = 0; i < size; line++) {
        *badLine = (int)std::min(line, kMaxInt);
        const void *nl = std::memchr(text + i, '\n', size - i);
        if (!nl) return false;                                                 /* bytes behind the last '\n' */
        const size_t stop = (size_t)(static_cast<const char *>(nl) - text);
        size_t end = stop;
        if (end > i && text[end - 1] == '\r') end--;
        int notBefore = -1, notAfter = -1;
        size_t j = i;
        ByteClass c{};
        if (end - j >= 4 && std::memcmp(text + j, "(?<!", 4) == 0) {
            if (!parseBoundary(text, j, end, "(?<![", &c)) return false;
            notBefore = (int)out.classOf(c);
        }
        const size_t firstElem = out.elemClass.size();
        bool quantifiable = false;                                              /* a unit stands right in front */
        while (j < end) {
            const char ch = text[j];
            if (ch == '(') {
                if (!parseBoundary(text, j, end, "(?![", &c) || j != end) return false;
                notAfter = (int)out.classOf(c);
                break;
            }
            if (ch == '{' || ch == '?') {
                if (!quantifiable) return false;                                /* no unit in front, or a quantifier */
                unsigned int lo = 0, hi = 1;
                j++;
                if (ch == '{') {
                    if (!parseNumber(text, j, end, &lo)) return false;          /* {,m} and {} among them */
                    hi = lo;
                    if (j < end && text[j] == ',') {
                        j++;
                        if (!parseNumber(text, j, end, &hi)) return false;      /* {n,} */
                    }
                    if (j >= end || text[j] != '}' || lo > hi) return false;
                    j++;
                }
                out.lo.back() = lo;
                out.hi.back() = hi;
                quantifiable = false;
                continue;
            }
            c = ByteClass{};
            j++;
            if (ch == '[') {
                if (!parseSet(text, j, end, &c)) return false;
            } else if (ch == '.') {
                invert(c);
            } else if (ch == '\\') {
                if (j >= end) return false;
                const int b = parseEscape(text, j, end, false, &c);
                if (b < 0) return false;
                if (b <= 255) addByte(c, (unsigned int)b);
            } else if (ch != '\0' && std::strchr("])}*+|^$", ch) != nullptr) {
                return false;
            } else {
                addByte(c, (unsigned char)ch);
            }
            out.elemClass.push_back(out.classOf(c));
            out.lo.push_back(1u);
            out.hi.push_back(1u);
            quantifiable = true;
        }
        if (out.elemClass.size() == firstElem) return false;                    /* an empty line, or boundaries alone */
        out.sigElem.push_back(out.elemClass.size());
        out.notBefore.push_back(notBefore);
        out.notAfter.push_back(notAfter);
        i = stop + 1;
    }
    *badLine = 0;
    return true;
}

/* ------------------------------------------------------------------ the calls */

/* the segments of a batch call (a plain call: all null); the device forms hand them to the passes, the host form to its loop */
struct Segments {
    const size_t *offsets = nullptr;
    size_t count = 0;
    size_t *segFirst = nullptr;
};

/* the passes over `count` ordered longest pairs, behind the argument checks; the caller holds c->lock.  seg: a batch (include/pfac_module.h) */
PFAC_status_t clsigRunLocked(PFACX_clsig_s *sg, const VerifyCall &call, int *d_end, const Segments &seg, const int *d_pairIds, const int *d_pairPos,
                             size_t count)
{
    PFACX_clsigRun_t run{};
    const PFAC_status_t st = fillRunFrame(sg, call, d_pairIds, d_pairPos, count, &run.v);
    if (st != PFAC_STATUS_SUCCESS) return st;
    run.d_sigOff = sg->d_sigOff.get();
    run.d_sigs = sg->d_sigs.get();
    run.numSigs = sg->sigs.size();
    run.d_parts = sg->d_parts.get();
    run.numParts = sg->parts.size();
    run.d_classes = sg->d_classes.get();
    run.numClasses = sg->classes.size() / 8;
    run.flags = sg->flags;
    run.d_end = d_end;
    run.d_offsets = seg.offsets;
    run.numSegments = seg.count;
    run.d_segFirst = seg.segFirst;
    return finishRun(sg->handle, sg->handle->clsig_run_ptr, run, call);
}

/* The host form's own search.  A mask holds where a BOUNDARY between two parts can lie: bit t = t bytes behind (forwards) or in front of
 * (backwards) its offset with every run at lo.  What it is checked against is tests/clsig_ref.py, which shares nothing with it. */
struct HostReach {
    uint64_t all, lt, eq;
};

/* one part forwards: r at base -> the boundary behind the part, at base + (its least length) */
HostReach partForward(const PFACX_clsig_s &sg, const unsigned char *in, size_t n, const pfac::ClSigPart &q, long long base, const HostReach &r)
{
    HostReach out{0, 0, 0};
    for (int t = 0; t < 64; t++) {
        if (!(r.all >> t & 1ull)) continue;
        const long long o = base + t;
        if (o < 0 || o > (long long)n) continue;
        uint64_t span = 0;
        if (q.kind == 0u) {
            const size_t len = q.a;
            if ((size_t)o + len <= n && std::memcmp(in + o, reinterpret_cast<const unsigned char *>(sg.blob.data() + q.b), len) == 0) span = 1ull << t;
        } else {
            const unsigned int *cls = sg.classes.data() + 8 * (size_t)q.a;
            size_t run = 0;
            while (run < q.c && (size_t)o + run < n && inClass(cls, in[(size_t)o + run])) run++;
            for (size_t len = q.b; len <= run; len++)
                if (t + (len - q.b) < 64) span |= 1ull << (t + (len - q.b));
        }
        out.all |= span;
        if (r.lt >> t & 1ull) out.lt |= span;
        if (r.eq >> t & 1ull) out.eq |= span;
    }
    return out;
}

/* one part backwards: m = where the boundary behind the part lies, base - t -> the boundary in front of it, at base - (its least length) - t' */
uint64_t partBackward(const PFACX_clsig_s &sg, const unsigned char *in, size_t n, const pfac::ClSigPart &q, long long base, uint64_t m)
{
    uint64_t out = 0;
    for (int t = 0; t < 64; t++) {
        if (!(m >> t & 1ull)) continue;
        const long long o = base - t;                                              /* the part ends in front of o */
        if (o < 0 || o > (long long)n) continue;
        if (q.kind == 0u) {
            const size_t len = q.a;
            if ((size_t)o >= len && std::memcmp(in + o - len, reinterpret_cast<const unsigned char *>(sg.blob.data() + q.b), len) == 0) out |= 1ull << t;
        } else {
            const unsigned int *cls = sg.classes.data() + 8 * (size_t)q.a;
            size_t run = 0;
            while (run < q.c && run < (size_t)o && inClass(cls, in[(size_t)o - 1 - run])) run++;
            for (size_t len = q.b; len <= run; len++)
                if (t + (len - q.b) < 64) out |= 1ull << (t + (len - q.b));
        }
    }
    return out;
}

unsigned int leastLength(const pfac::ClSigPart &q) { return q.kind == 0u ? q.a : q.b; }

/* emit(start, end) for what the anchor occurrence at p owns of signature e, starts ascending */
template <class Emit>
void searchOnHost(const PFACX_clsig_s &sg, const unsigned char *in, size_t n, const pfac::ClSigEntry &e, int p, Emit emit)
{
    const unsigned int count = e.partsAnchor & 0xFFFFu, anchor = e.partsAnchor >> 16;
    if (e.anchorOff > (unsigned int)p) return;                                     /* it would lie in front of the input */
    const pfac::ClSigPart *parts = sg.parts.data() + e.firstPart;
    const long long x = (long long)p - (long long)e.anchorOff;
    if (partForward(sg, in, n, parts[anchor], x, HostReach{1, 0, 0}).all == 0) return;
    uint64_t back = 1;
    long long tight = x;
    for (unsigned int j = anchor; j > 0u && back != 0ull; j--) {
        back = partBackward(sg, in, n, parts[j - 1u], tight, back);
        tight -= leastLength(parts[j - 1u]);
    }
    for (int tb = 63; tb >= 0; tb--) {                                             /* the starts, ascending */
        if (!(back >> tb & 1ull)) continue;
        const long long s = tight - tb;
        if (s < 0) continue;
        if (s > 0 && e.notBefore >= 0 && inClass(sg.classes.data() + 8 * (size_t)e.notBefore, in[s - 1])) continue;
        HostReach r{1, 0, 0};
        long long at = s;
        for (unsigned int j = 0; j < anchor && r.all != 0ull; j++) {
            r = partForward(sg, in, n, parts[j], at, r);
            at += leastLength(parts[j]);
        }
        const long long tx = x - at;
        if (tx < 0 || tx > 63) continue;
        r.eq = r.all & (1ull << tx);
        r.lt = r.all & ((1ull << tx) - 1ull);
        for (unsigned int j = anchor; j < count && r.eq != 0ull; j++) {
            r = partForward(sg, in, n, parts[j], at, r);
            at += leastLength(parts[j]);
        }
        if (r.eq == 0ull) continue;
        if (e.notAfter >= 0) {
            const unsigned int *cls = sg.classes.data() + 8 * (size_t)e.notAfter;
            uint64_t valid = 0;
            for (int t = 0; t < 64; t++) {
                const long long end = at + t;
                if ((r.all >> t & 1ull) && (end >= (long long)n || !inClass(cls, in[end]))) valid |= 1ull << t;
            }
            r.all &= valid;
            r.lt &= valid;
            r.eq &= valid;
        }
        if (r.eq == 0ull || r.lt != 0ull) continue;                                /* not on a valid embedding at s, or a nearer anchor occurrence owns it */
        emit((int)s, (int)(at + ((sg.flags & PFACX_CLSIG_SHORTEST_END) ? __builtin_ctzll(r.all) : 63 - __builtin_clzll(r.all))));
    }
}

/* The host loop: what the chains of `count` ordered longest pairs own into ids / pos / end (slots >= capacity are not written; end may be
 * null); returns the full length of the list.  offsets (validated: 0 ... n, never decreasing; null: one segment, the buffer): a pair is searched
 * inside the WINDOW [offsets[k], offsets[k + 1]) that holds its position -- the search sees the window's bytes as its whole input, and what it
 * finds is shifted back --, and segFirst[k] (numSegments + 1 entries; may be null) = the length of the list in front of segment k */
size_t clsigOnHost(const pfac::Automaton &fa, const PFACX_clsig_s &sg, const unsigned char *in, size_t n, const int *pairIds, const int *pairPos,
                   size_t count, int *ids, int *pos, int *end, size_t capacity, const size_t *offsets = nullptr, size_t numSegments = 1,
                   size_t *segFirst = nullptr)
{
    const size_t whole[2] = {0, n};
    if (!offsets) { offsets = whole; numSegments = 1; }
    size_t total = 0, k = 0;                                                  /* k: the segments whose segFirst is written */
    for (size_t i = 0; i < count; i++) {
        const int p = pairPos[i];
        if (p < 0 || (size_t)p >= n) continue;
        /* the last segment that starts at or in front of p: behind the empty ones that start there too */
        const size_t seg = (size_t)(std::upper_bound(offsets, offsets + numSegments + 1, (size_t)p) - offsets) - 1;   /* offsets[0] == 0 <= p < n == offsets[numSegments] */
        if (segFirst)
            for (; k <= seg; k++) segFirst[k] = total;
        const size_t lo = offsets[seg], hi = offsets[seg + 1];
        forEachChainMember(fa, pairIds[i], [&](int q) {                       /* (the caller's pin: fa.numPatterns == sg.numIds) */
            for (size_t v = sg.sigOff[(size_t)q]; v < sg.sigOff[(size_t)q + 1]; v++) {
                const pfac::ClSigEntry &e = sg.sigs[v];
                searchOnHost(sg, in + lo, hi - lo, e, p - (int)lo, [&](int s, int behind) {
                    if (total < capacity) {
                        ids[total] = e.id;
                        pos[total] = s + (int)lo;
                        if (end) end[total] = behind + (int)lo;
                    }
                    total++;
                });
            }
            return true;
        });
    }
    if (segFirst)
        for (; k <= numSegments; k++) segFirst[k] = total;
    return total;
}

} // namespace

extern "C" {

PFAC_status_t PFACX_clsigOpen(PFAC_handle_t handle, const unsigned int *h_classes, size_t numClasses, const unsigned int *h_elemClass,
                              const unsigned int *h_elemLo, const unsigned int *h_elemHi, const size_t *h_sigElem, const int *h_notBefore,
                              const int *h_notAfter, size_t numSigs, size_t maxAnchorLen, unsigned int flags, PFACX_clsig_t *sig, int *badSig)
{
    if (!handle) return PFAC_STATUS_INVALID_HANDLE;
    if (!sig) return PFAC_STATUS_INVALID_PARAMETER;
    *sig = nullptr;
    int bad = 0;
    if (badSig) *badSig = 0;
    if (!h_classes || !h_elemClass || !h_elemLo || !h_elemHi || !h_sigElem || numSigs == 0 || numSigs >= kMaxInt || numClasses == 0 ||
        numClasses > kMaxClasses || (flags & ~PFACX_CLSIG_SHORTEST_END) != 0u)
        return PFAC_STATUS_INVALID_PARAMETER;
    ClSigPlan plan;
    std::vector<unsigned int> classes;
    try {
        std::vector<int> single(numClasses, -1);                               /* the one byte of a class, -1: it has more */
        for (size_t c = 0; c < numClasses; c++) {
            int members = 0, last = 0;
            for (unsigned int b = 0; b < 256; b++)
                if (inClass(h_classes + 8 * c, b)) { members++; last = (int)b; }
            if (members == 0) return PFAC_STATUS_INVALID_PARAMETER;            /* an empty class */
            if (members == 1) single[c] = last;
        }
        classes.assign(h_classes, h_classes + 8 * numClasses);
        const PFAC_status_t st =
            planSignatures(single, h_elemClass, h_elemLo, h_elemHi, h_sigElem, h_notBefore, h_notAfter, numSigs, maxAnchorLen, &plan, &bad);
        if (badSig) *badSig = bad;
        if (st != PFAC_STATUS_SUCCESS) return st;                             /* nothing of the handle has changed */
    } catch (const std::bad_alloc &) { return PFAC_STATUS_ALLOC_FAILED; }
    return adoptOverStrings(handle, plan.anchors, sig, [&](PFACX_clsig_s &obj) -> PFAC_status_t {     /* (verify_calls.h: the tables hold only over the anchors) */
        if (!buildTables(plan, &obj)) return PFAC_STATUS_INVALID_PARAMETER;
        obj.classes = std::move(classes);
        obj.flags = flags;
        return PFAC_STATUS_SUCCESS;
    });
}

PFAC_status_t PFACX_clsigOpenText(PFAC_handle_t handle, const char *text, size_t size, size_t maxAnchorLen, unsigned int flags, PFACX_clsig_t *sig,
                                  int *badLine)
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
        if (!ok || parsed.sigElem.size() < 2) return PFAC_STATUS_INVALID_PARAMETER;  /* (no line at all: numSigs == 0) */
    } catch (const std::bad_alloc &) { return PFAC_STATUS_ALLOC_FAILED; }
    /* a line is a signature: the id the binary form refuses is the line */
    return PFACX_clsigOpen(handle, parsed.classes.data(), parsed.classes.size() / 8, parsed.elemClass.data(), parsed.lo.data(), parsed.hi.data(),
                           parsed.sigElem.data(), parsed.notBefore.data(), parsed.notAfter.data(), parsed.sigElem.size() - 1, maxAnchorLen, flags, sig,
                           badLine);
}

PFAC_status_t PFACX_clsigClose(PFACX_clsig_t sig) { return closeObject(sig); }

PFAC_status_t PFACX_clsigGetAnchors(PFACX_clsig_t sig, int *h_anchorId, int *h_anchorPart, int *h_anchorOff, int *h_anchorLen, size_t n)
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

/* The three forms, plain (batch == false: no offsets, no segFirst) and batch, over the frame of verify_calls.h.  The device form scans the WHOLE
 * buffer for the anchors, plain and ordered, also for a batch: every anchor that fits a segment at p is a prefix of the longest one at p, and the
 * search rejects per signature what leaves the segment.  What a batch adds: the check of its segments in front of the lock (the
 * offsets, their number -- 0 only with size == 0 --, and on the host their values), and segFirst all zero where there is no pair */
namespace {

struct ClSigForms {
    PFACX_clsig_t sig;
    VerifyCall call;
    int *end;
    bool batch;
    Segments seg;

    PFAC_status_t checkSegments(bool onHost) const
    {
        if (!batch) return PFAC_STATUS_SUCCESS;
        if (!seg.offsets || seg.count >= kMaxInt || (call.size && seg.count == 0)) return PFAC_STATUS_INVALID_PARAMETER;
        if (onHost && call.size && !batchOffsetsValid(seg.offsets, seg.count, call.size)) return PFAC_STATUS_INVALID_PARAMETER;
        return PFAC_STATUS_SUCCESS;
    }
    auto run() const
    {
        return [this](const int *ids, const int *pos, size_t count) { return clsigRunLocked(sig, call, end, seg, ids, pos, count); };
    }
    auto noPairs() const
    {
        return [this]() { return seg.segFirst ? zeroSegmentArrays(seg.segFirst, nullptr, seg.count) : PFAC_STATUS_SUCCESS; };
    }

    PFAC_status_t fromDevice() const { return verifyFromDevice(sig, call, run(), [this]() { return checkSegments(false); }, noPairs()); }
    PFAC_status_t fromHost() const
    {
        /* the longest pairs of the whole buffer on every platform (the GPU platform: the staged host path), the segments in the search alone */
        return verifyFromHost(
            sig, call,
            [this](const int *ids, const int *pos, size_t count) {
                return clsigOnHost(sig->handle->fa, *sig, reinterpret_cast<const unsigned char *>(call.input), call.size, ids, pos, count, call.ids, call.pos,
                                   end, call.capacity, batch ? seg.offsets : nullptr, seg.count, seg.segFirst);
            },
            [this]() { return checkSegments(true); });
    }
    PFAC_status_t pairsFromDevice(const int *d_pairIds, const int *d_pairPos, size_t numPairs) const
    {
        return verifyPairsFromDevice(sig, call, d_pairIds, d_pairPos, numPairs, {call.ids, call.pos, end}, run(), [this]() { return checkSegments(false); },
                                     noPairs());
    }
};

} // namespace

PFAC_status_t PFACX_clsigMatchFromDevice(PFACX_clsig_t sig, char *d_input, size_t size, int *d_ids, int *d_pos, int *d_end, size_t capacity,
                                         size_t *h_num_matched)
{
    return ClSigForms{sig, {d_input, size, d_ids, d_pos, capacity, h_num_matched}, d_end, false, {}}.fromDevice();
}

PFAC_status_t PFACX_clsigMatchFromHost(PFACX_clsig_t sig, char *h_input, size_t size, int *h_ids, int *h_pos, int *h_end, size_t capacity,
                                       size_t *h_num_matched)
{
    return ClSigForms{sig, {h_input, size, h_ids, h_pos, capacity, h_num_matched}, h_end, false, {}}.fromHost();
}

PFAC_status_t PFACX_clsigPairsFromDevice(PFACX_clsig_t sig, const char *d_input, size_t size, const int *d_pairIds, const int *d_pairPos,
                                         size_t numPairs, int *d_ids, int *d_pos, int *d_end, size_t capacity, size_t *h_num_matched)
{
    return ClSigForms{sig, {d_input, size, d_ids, d_pos, capacity, h_num_matched}, d_end, false, {}}.pairsFromDevice(d_pairIds, d_pairPos, numPairs);
}

PFAC_status_t PFACX_clsigBatchMatchFromDevice(PFACX_clsig_t sig, char *d_input, size_t size, const size_t *d_offsets, size_t numSegments, int *d_ids,
                                              int *d_pos, int *d_end, size_t capacity, size_t *d_segFirst, size_t *h_num_matched)
{
    return ClSigForms{sig, {d_input, size, d_ids, d_pos, capacity, h_num_matched}, d_end, true, {d_offsets, numSegments, d_segFirst}}.fromDevice();
}

PFAC_status_t PFACX_clsigBatchMatchFromHost(PFACX_clsig_t sig, char *h_input, size_t size, const size_t *h_offsets, size_t numSegments, int *h_ids,
                                            int *h_pos, int *h_end, size_t capacity, size_t *h_segFirst, size_t *h_num_matched)
{
    return ClSigForms{sig, {h_input, size, h_ids, h_pos, capacity, h_num_matched}, h_end, true, {h_offsets, numSegments, h_segFirst}}.fromHost();
}

PFAC_status_t PFACX_clsigBatchPairsFromDevice(PFACX_clsig_t sig, const char *d_input, size_t size, const size_t *d_offsets, size_t numSegments,
                                              const int *d_pairIds, const int *d_pairPos, size_t numPairs, int *d_ids, int *d_pos, int *d_end,
                                              size_t capacity, size_t *d_segFirst, size_t *h_num_matched)
{
    return ClSigForms{sig, {d_input, size, d_ids, d_pos, capacity, h_num_matched}, d_end, true, {d_offsets, numSegments, d_segFirst}}.pairsFromDevice(
        d_pairIds, d_pairPos, numPairs);
}

} /* extern "C" */
