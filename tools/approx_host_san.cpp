/*
 * approx_host_san.cpp -- PFACX_approxOpen, PFACX_approxGetPieces and PFACX_approxMatchFromHost on a host-only handle over the case table of
 * tests/approx_ref.py, for the sanitizer build of the host library (make -C pfac_amd/csrc san: build/approx_host_san links lib/san/libpfac.so;
 * CPU only).  Every case is opened from heap blocks of exactly their size, its pieces are read into arrays of exactly their size and compared with
 * the documented cut, and it runs on both CPU platforms at every capacity from 0 to the list's length + 1, into arrays allocated at exactly
 * `capacity` entries and over an input in a heap block of exactly its size -- a write behind the arrays or a read behind the input is the
 * sanitizer's to find -- and is compared with the definition, evaluated here start by start and pattern by pattern and ordered by the lowest
 * exact piece.  Then every refusal of the open call.  Exit status 0: every list agreed.
 */
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "PFAC.h"
#include "pfac_ext.h"

namespace {

struct Case {
    const char *name;
    std::vector<std::string> patterns;
    std::vector<int> budgets;
    size_t minPiece, maxPiece;
    std::string input;
};

int failures = 0;

void check(bool ok, const char *name, const char *what, int platform)
{
    if (ok) return;
    failures++;
    std::fprintf(stderr, "FAILED %s: %s (platform %d)\n", name, what, platform);
}

std::string mutate(std::string s, std::initializer_list<size_t> where)
{
    for (size_t at : where) s[at] = (char)(s[at] ^ 0x80);
    return s;
}

/* the documented cut: (start, length) of piece j */
std::pair<size_t, size_t> pieceOf(size_t len, size_t k, size_t j, size_t maxPiece)
{
    const size_t from = j * len / (k + 1), to = (j + 1) * len / (k + 1);
    return {from, std::min(to - from, maxPiece ? maxPiece : (size_t)32)};
}

struct Entry { int id, start, mis; };

/* the definition, ordered by the contract: candidate position of the lowest exact piece, the longer piece first, id and piece index descending */
std::vector<Entry> byDefinition(const Case &c)
{
    std::vector<std::tuple<int, int, int, int, int, int>> found;        /* candidate position, -piece length, -id, -piece, start, d */
    const std::string &in = c.input;
    for (size_t i = 0; i < c.patterns.size(); i++) {
        const std::string &p = c.patterns[i];
        const size_t k = (size_t)c.budgets[i];
        for (size_t at = 0; at + p.size() <= in.size(); at++) {
            size_t d = 0;
            for (size_t t = 0; t < p.size(); t++) d += in[at + t] != p[t];
            if (d > k) continue;
            for (size_t j = 0; j <= k; j++) {
                const auto piece = pieceOf(p.size(), k, j, c.maxPiece);
                if (in.compare(at + piece.first, piece.second, p, piece.first, piece.second) != 0) continue;
                found.emplace_back((int)(at + piece.first), -(int)piece.second, -(int)(i + 1), -(int)j, (int)at, (int)d);
                break;
            }
        }
    }
    std::sort(found.begin(), found.end());
    std::vector<Entry> out;
    for (const auto &f : found) out.push_back(Entry{-std::get<2>(f), std::get<4>(f), std::get<5>(f)});
    return out;
}

PFAC_handle_t hostHandle(int platform)
{
    PFAC_handle_t h = nullptr;
    if (PFACX_createHostOnly(&h) == PFAC_STATUS_SUCCESS && PFAC_setPlatform(h, (PFAC_platform_t)platform) == PFAC_STATUS_SUCCESS) return h;
    if (h) PFAC_destroy(h);
    return nullptr;
}

/* PFACX_approxOpen from heap blocks of exactly their size; offsets that start at `lead` (the CSR form need not start at 0) */
PFAC_status_t openExact(PFAC_handle_t h, const std::vector<std::string> &patterns, const std::vector<int> &budgets, size_t minPiece, size_t maxPiece,
                        PFACX_approx_t *ap, int *bad, size_t lead = 0)
{
    size_t bytes = lead;
    for (const std::string &p : patterns) bytes += p.size();
    std::unique_ptr<unsigned char[]> blob(new unsigned char[bytes ? bytes : 1]);
    std::unique_ptr<size_t[]> off(new size_t[patterns.size() + 1]);
    std::unique_ptr<int[]> budget(new int[patterns.size() ? patterns.size() : 1]);
    std::memset(blob.get(), '.', lead);
    off[0] = lead;
    for (size_t i = 0; i < patterns.size(); i++) {
        std::memcpy(blob.get() + off[i], patterns[i].data(), patterns[i].size());
        off[i + 1] = off[i] + patterns[i].size();
        budget[i] = budgets[i];
    }
    return PFACX_approxOpen(h, blob.get(), off.get(), budget.get(), patterns.size(), minPiece, maxPiece, ap, bad);
}

void runPieces(const Case &c, PFACX_approx_t ap, int platform)
{
    const size_t S = c.patterns.size();
    size_t pieces = 0;
    for (int k : c.budgets) pieces += (size_t)k + 1;
    std::unique_ptr<size_t[]> off(new size_t[S + 2]);                  /* exactly S + 2 and exactly the number of pieces */
    std::unique_ptr<int[]> id(new int[pieces]), start(new int[pieces]), len(new int[pieces]);
    check(PFACX_approxGetPieces(ap, off.get(), id.get(), start.get(), len.get(), pieces - 1) == PFAC_STATUS_INVALID_PARAMETER, c.name, "the getter with n too small", platform);
    check(PFACX_approxGetPieces(ap, off.get(), nullptr, nullptr, nullptr, 0) == PFAC_STATUS_SUCCESS && off[S + 1] == pieces, c.name, "the offsets alone", platform);
    check(PFACX_approxGetPieces(ap, off.get(), id.get(), start.get(), len.get(), pieces) == PFAC_STATUS_SUCCESS, c.name, "the getter", platform);
    bool ok = off[0] == 0 && off[1] == 0;
    std::vector<std::string> distinct;
    for (size_t i = 1; ok && i <= S; i++) {
        const std::string &p = c.patterns[i - 1];
        const size_t k = (size_t)c.budgets[i - 1];
        ok = off[i + 1] == off[i] + k + 1;
        for (size_t j = 0; ok && j <= k; j++) {
            const auto piece = pieceOf(p.size(), k, j, c.maxPiece);
            const std::string text = p.substr(piece.first, piece.second);
            size_t q = (size_t)(std::find(distinct.begin(), distinct.end(), text) - distinct.begin());
            if (q == distinct.size()) distinct.push_back(text);
            const size_t e = off[i] + j;
            ok = id[e] == (int)q + 1 && start[e] == (int)piece.first && len[e] == (int)piece.second;
        }
    }
    check(ok, c.name, "the pieces against the documented cut", platform);
}

void runLists(const Case &c, PFACX_approx_t ap, int platform)
{
    const size_t n = c.input.size();
    const std::vector<Entry> want = byDefinition(c);
    check(!want.empty(), c.name, "the case has no occurrence", platform);
    for (int withMis = 0; withMis < 2; withMis++)
        for (size_t capacity = 0; capacity <= want.size() + 1; capacity++) {
            std::unique_ptr<char[]> input(new char[n]);              /* exactly n bytes */
            std::memcpy(input.get(), c.input.data(), n);
            std::unique_ptr<int[]> ids(new int[capacity]), pos(new int[capacity]), mis(new int[capacity]);
            std::fill(ids.get(), ids.get() + capacity, -7);
            std::fill(pos.get(), pos.get() + capacity, -7);
            std::fill(mis.get(), mis.get() + capacity, -7);
            size_t total = 12345;
            const PFAC_status_t st = PFACX_approxMatchFromHost(ap, input.get(), n, capacity ? ids.get() : nullptr, capacity ? pos.get() : nullptr,
                                                               capacity && withMis ? mis.get() : nullptr, capacity, &total);
            check(st == (want.size() > capacity ? PFACX_STATUS_OUTPUT_TRUNCATED : PFAC_STATUS_SUCCESS), c.name, "the status", platform);
            check(total == want.size(), c.name, "the length of the list", platform);
            check(std::memcmp(input.get(), c.input.data(), n) == 0, c.name, "the caller's bytes", platform);
            for (size_t k = 0; k < capacity; k++) {
                const bool in = k < want.size();
                check(ids[k] == (in ? want[k].id : -7) && pos[k] == (in ? want[k].start : -7), c.name, "an entry", platform);
                check(mis[k] == (in && withMis ? want[k].mis : -7), c.name, "a distance", platform);
            }
        }
}

void runCase(const Case &c)
{
    for (int platform : {(int)PFAC_PLATFORM_CPU, (int)PFAC_PLATFORM_CPU_OMP}) {
        PFAC_handle_t h = hostHandle(platform);
        if (!h) { check(false, c.name, "no host-only handle", platform); continue; }
        PFACX_approx_t ap = nullptr;
        int bad = -1;
        const PFAC_status_t st = openExact(h, c.patterns, c.budgets, c.minPiece, c.maxPiece, &ap, &bad, platform == (int)PFAC_PLATFORM_CPU ? 0 : 3);
        check(st == PFAC_STATUS_SUCCESS && ap && bad == 0, c.name, "the open call", platform);
        if (ap) {
            runPieces(c, ap, platform);
            runLists(c, ap, platform);
            check(PFACX_approxClose(ap) == PFAC_STATUS_SUCCESS, c.name, "the close call", platform);
        }
        PFAC_destroy(h);
    }
}

void runRefusals()
{
    struct Refusal { const char *why; std::vector<std::string> patterns; std::vector<int> budgets; size_t minPiece, maxPiece; int bad; };
    const std::vector<Refusal> refusals = {
        {"an empty pattern", {"abcd", "", "efgh"}, {0, 0, 0}, 0, 0, 2},
        {"65 536 bytes", {"abcd", std::string(65536, 'x')}, {0, 0}, 0, 0, 2},
        {"a budget of 8", {"abcd", std::string(64, 'x')}, {0, 8}, 0, 0, 2},
        {"a negative budget", {std::string(64, 'x')}, {-1}, 0, 0, 1},
        {"7 bytes for two pieces of 4", {"abcdefg"}, {1}, 0, 0, 1},
        {"9 bytes for two pieces of 5", {"abcdefghi"}, {1}, 5, 0, 1},
        {"fewer bytes than parts", {"ab"}, {2}, 1, 0, 1},
        {"a minPieceLen no pattern can have", {"abcd"}, {0}, 65536, 0, 1},
        {"0x0A in the only piece", {"abcd", "ab\ncdefgh"}, {0, 0}, 0, 0, 2},
        {"0x0A at the head of piece 1", {"abcdefgh", "abcd\nfgh"}, {1, 1}, 0, 0, 2},
        {"0x0A as the last byte the cut keeps", {"abcde\nfgh"}, {0}, 0, 6, 1},
    };
    PFAC_handle_t h = hostHandle((int)PFAC_PLATFORM_CPU);
    if (!h) { check(false, "refusals", "no host-only handle", 0); return; }
    char kept[] = "kept\n";
    check(PFACX_readPatternFromMemory(h, kept, 5) == PFAC_STATUS_SUCCESS, "refusals", "the set that must stay", 0);
    for (const Refusal &r : refusals) {
        PFACX_approx_t ap = reinterpret_cast<PFACX_approx_t>(&failures);
        int bad = -1;
        check(openExact(h, r.patterns, r.budgets, r.minPiece, r.maxPiece, &ap, &bad) == PFAC_STATUS_INVALID_PARAMETER && ap == nullptr && bad == r.bad,
              "refusals", r.why, 0);
        int id[4] = {0, 0, 0, 0};                                       /* one result per input byte */
        char text[] = "kept";
        check(PFAC_matchFromHost(h, text, 4, id) == PFAC_STATUS_SUCCESS && id[0] == 1, "refusals", "a refusal leaves the handle's set alone", 0);
    }
    /* the argument rows */
    const unsigned char blob[] = "abcdefgh";
    const size_t off[] = {0, 4, 8}, descending[] = {0, 6, 4};
    const int budget[] = {0, 0};
    PFACX_approx_t ap = nullptr;
    int bad = -1;
    check(PFACX_approxOpen(nullptr, blob, off, budget, 2, 0, 0, &ap, &bad) == PFAC_STATUS_INVALID_HANDLE, "refusals", "no handle", 0);
    check(PFACX_approxOpen(h, nullptr, off, budget, 2, 0, 0, &ap, &bad) == PFAC_STATUS_INVALID_PARAMETER, "refusals", "no bytes", 0);
    check(PFACX_approxOpen(h, blob, nullptr, budget, 2, 0, 0, &ap, &bad) == PFAC_STATUS_INVALID_PARAMETER, "refusals", "no offsets", 0);
    check(PFACX_approxOpen(h, blob, off, nullptr, 2, 0, 0, &ap, &bad) == PFAC_STATUS_INVALID_PARAMETER, "refusals", "no budgets", 0);
    check(PFACX_approxOpen(h, blob, off, budget, 2, 0, 0, nullptr, &bad) == PFAC_STATUS_INVALID_PARAMETER, "refusals", "no object pointer", 0);
    check(PFACX_approxOpen(h, blob, off, budget, 0, 0, 0, &ap, &bad) == PFAC_STATUS_INVALID_PARAMETER && bad == 0, "refusals", "numPatterns == 0", 0);
    check(PFACX_approxOpen(h, blob, off, budget, 0x7fffffff, 0, 0, &ap, &bad) == PFAC_STATUS_INVALID_PARAMETER && bad == 0, "refusals", "numPatterns >= 2^31 - 1", 0);
    check(PFACX_approxOpen(h, blob, descending, budget, 2, 0, 0, &ap, &bad) == PFAC_STATUS_INVALID_PARAMETER && bad == 2, "refusals", "offsets that descend", 0);
    check(PFACX_approxOpen(h, blob, off, budget, 2, 0, 0, &ap, nullptr) == PFAC_STATUS_SUCCESS && ap, "refusals", "badPattern may be null", 0);
    if (ap) {
        /* the stale object: the handle reads another set, only the close call works */
        check(PFACX_readPatternFromMemory(h, kept, 5) == PFAC_STATUS_SUCCESS, "refusals", "another read", 0);
        size_t total = 0;
        char text[] = "abcd";
        check(PFACX_approxMatchFromHost(ap, text, 4, nullptr, nullptr, nullptr, 0, &total) == PFAC_STATUS_INVALID_PARAMETER, "refusals", "a stale object", 0);
        check(PFACX_approxGetPieces(ap, nullptr, nullptr, nullptr, nullptr, 0) == PFAC_STATUS_INVALID_PARAMETER, "refusals", "the getter of a stale object", 0);
        check(PFACX_approxClose(ap) == PFAC_STATUS_SUCCESS, "refusals", "the close call of a stale object", 0);
    }
    check(PFACX_approxClose(nullptr) == PFAC_STATUS_INVALID_HANDLE, "refusals", "closing nothing", 0);
    PFAC_destroy(h);
}

} // namespace

int main()
{
    const std::string p32 = "ABCDEFGHIJKLMNOPQRSTUVWXYZ012345";          /* k = 3: four parts of 8 bytes */
    std::string eachPieceAlone;
    for (size_t j = 0; j < 4; j++) {
        std::string v = p32;
        for (size_t e = 0; e < 4; e++)
            if (e != j) v[8 * e + 3] = (char)(v[8 * e + 3] ^ 0x80);
        eachPieceAlone += (j ? " " : "") + v;
    }
    /* an edge set of its own: lengths around the dwords and the 16-byte test, a substitution in the last byte, in byte 0, two of them */
    Case edges{"compare-edges", {}, {}, 1, 0, "."};
    for (size_t len : {2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 64}) {
        std::string p;
        for (size_t i = 0; i < len; i++) p += (char)(0x30 + (11 * i + 5 * len) % 0x4B);
        edges.patterns.push_back(p);
        edges.budgets.push_back(1);
        edges.input += p + "." + mutate(p, {len - 1}) + ".." + mutate(p, {0}) + "..." + mutate(p, {0, len - 1}) + ".";
    }
    edges.input += edges.patterns.back();                                /* the input ends with an occurrence */
    const std::vector<Case> cases = {
        {"keywords-with-typos", {"password", "username", "creditcard", "passport"}, {1, 1, 1, 1}, 0, 0,
         "pasword password passw0rd usermame user_name creditcard cred1tcarb passp0rt pa55port xpassworx"},
        {"each-piece-alone", {p32}, {3}, 0, 0, eachPieceAlone},
        {"all-pieces-exact-one-entry", {p32}, {3}, 0, 0, "--" + p32 + "--" + p32},
        {"pieces-1-and-3-exact", {p32}, {3}, 0, 0, "-" + mutate(p32, {0, 20}) + "-"},
        {"four-substitutions-are-too-many", {p32}, {3}, 0, 0, mutate(p32, {1, 9, 17, 25}) + " " + mutate(p32, {9, 10, 17, 25}) + " " + mutate(p32, {9, 17, 25})},
        {"one-piece-string-thrice", {"abcdabcdabcd"}, {2}, 0, 0, "abcdabcdabcdabcdabcdabcdabcdabcd"},
        {"two-patterns-share-a-piece", {"sharedXYZW", "QRSTshared", "sharedshar"}, {0, 1, 0}, 0, 6, "sharedXYZW QRSTshared QRSTsharex xRSTshared sharedshared"},
        {"identical-patterns-budgets-0-and-2", {"identicalxyz", "identicalxyz"}, {0, 2}, 0, 0, "identicalxyz idemticalxyy idxnticalxyz ixentxcalxyx"},
        {"a-piece-is-a-prefix-of-another", {"abcdefgh", "abcdWXYZ", "abcdefXY"}, {0, 1, 0}, 0, 0, "abcdefgh abcdWXYy abcdefXY abcdWXYZabcdefgh"},
        {"newline-outside-the-pieces", {"abc\ndefg", "abcd\nefgh"}, {1, 0}, 0, 3, "abc\ndefg abcxdefg abc\ndexg abcd\nefgh abcdxefgh xbc\ndefg"},
        {"the-cut-of-a-piece", {"0123456789abcdefghij"}, {1}, 0, 5, "0123456789abcdefghij 01234x6789abcdefghij x123456789abcdefghij 0123456789xbcdefghij"},
        {"not-sorted-by-start", {"xxxxxxxxabcd", "xyxx"}, {1, 0}, 0, 0, "xxxxxyxxabcd"},
        {"single-bytes", {"a", "b", "a"}, {0, 0, 0}, 1, 0, "abab"},
        {"one-byte-parts", {"abc", "abd"}, {2, 1}, 1, 0, "abc abd xbc axx xxc abx"},
        edges,
    };
    for (const Case &c : cases) runCase(c);
    runRefusals();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("approx_host_san: %zu cases on both CPU platforms at every capacity, the getter and the refusals: all agreed\n", cases.size());
    return 0;
}
