/*
 * case_host_san.cpp -- PFACX_caseOpen and PFACX_caseMatchFromHost on a host-only handle over the case table of tests/case_ref.py, for the sanitizer
 * build of the host library (make -C pfac_amd/csrc san: build/case_host_san links lib/san/libpfac.so; CPU only).  Every case runs in both modes, on
 * both CPU platforms, at every capacity from 0 to the list's length, into arrays allocated at exactly `capacity` entries and over an input in a heap
 * block of exactly its size -- a write behind the arrays or a read behind the input is the sanitizer's to find -- and is compared with the
 * definition, evaluated here position by position and line by line.  Then the refusals of the open call.  Exit status 0: every list agreed.
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
    std::vector<unsigned char> sensitive;       /* by line, line 1 first */
    std::string input;
};

unsigned char fold(unsigned char b) { return b >= 'A' && b <= 'Z' ? (unsigned char)(b + 32) : b; }

std::string folded(const std::string &s)
{
    std::string out = s;
    for (char &ch : out) ch = (char)fold((unsigned char)ch);
    return out;
}

/* the definition: (position, id) of every distinct occurring pattern, by position, length descending, id descending; !all: the first of a position */
std::vector<std::pair<int, int>> byDefinition(const Case &c, bool all)
{
    const std::string &in = c.input;
    const size_t n = in.size(), F = c.patterns.size();
    std::vector<std::tuple<int, int, int>> found;               /* position, -length, -id */
    for (size_t k = 0; k < F; k++) {
        const std::string &pat = c.patterns[k];
        const bool s = c.sensitive[k] != 0;
        bool later = false;                                      /* the same pattern under a higher id: reported there */
        for (size_t j = k + 1; j < F && !later; j++)
            later = (c.sensitive[j] != 0) == s && (s ? c.patterns[j] == pat : folded(c.patterns[j]) == folded(pat));
        if (later || pat.empty()) continue;
        for (size_t p = 0; p + pat.size() <= n; p++) {
            const std::string piece = in.substr(p, pat.size());
            if (s ? piece == pat : folded(piece) == folded(pat)) found.emplace_back((int)p, -(int)pat.size(), -(int)(k + 1));
        }
    }
    std::sort(found.begin(), found.end());
    std::vector<std::pair<int, int>> out;
    for (const auto &f : found)
        if (all || out.empty() || out.back().first != std::get<0>(f)) out.emplace_back(std::get<0>(f), -std::get<2>(f));
    return out;
}

int failures = 0;

void check(bool ok, const char *name, const char *what, int platform, unsigned int flags)
{
    if (ok) return;
    failures++;
    std::fprintf(stderr, "FAILED %s: %s (platform %d, flags %u)\n", name, what, platform, flags);
}

std::string textOf(const std::vector<std::string> &patterns)
{
    std::string file;
    for (const std::string &p : patterns) file += p + "\n";
    return file;
}

PFAC_handle_t caselessHandle(const std::string &file, int platform)
{
    PFAC_handle_t h = nullptr;
    if (PFACX_createHostOnly(&h) == PFAC_STATUS_SUCCESS && PFAC_setPlatform(h, (PFAC_platform_t)platform) == PFAC_STATUS_SUCCESS &&
        PFACX_readPatternFromMemoryEx(h, file.data(), file.size(), PFACX_READ_NOCASE) == PFAC_STATUS_SUCCESS)
        return h;
    if (h) PFAC_destroy(h);
    return nullptr;
}

void runCase(const Case &c)
{
    const std::string file = textOf(c.patterns);
    std::vector<unsigned char> flags(c.patterns.size() + 1, 0);         /* exactly F + 1 entries, by id */
    std::copy(c.sensitive.begin(), c.sensitive.end(), flags.begin() + 1);
    for (int platform : {PFAC_PLATFORM_CPU, PFAC_PLATFORM_CPU_OMP}) {
        PFAC_handle_t h = caselessHandle(file, platform);
        PFACX_case_t cs = nullptr;
        int most = -1;
        {   /* the text in a heap block of exactly its size: the open call copies what it keeps */
            std::unique_ptr<char[]> text(new char[file.size()]);
            std::memcpy(text.get(), file.data(), file.size());
            if (!h || PFACX_caseOpen(h, text.get(), file.size(), 0, flags.data(), flags.size(), &cs, &most) != PFAC_STATUS_SUCCESS) {
                check(false, c.name, "the handle or the open call", platform, 0);
                if (h) PFAC_destroy(h);
                continue;
            }
        }
        std::fill(flags.begin(), flags.end(), (unsigned char)0xAA);     /* ... and the flags */
        size_t longest = 0;
        for (unsigned int mode : {0u, PFACX_CASE_ALL}) {
            const std::vector<std::pair<int, int>> want = byDefinition(c, mode != 0);
            const size_t n = c.input.size();
            if (mode) {
                size_t run = 0;
                for (size_t k = 0; k < want.size(); k++) {
                    run = k && want[k].first == want[k - 1].first ? run + 1 : 1;
                    longest = std::max(longest, run);
                }
            }
            for (size_t capacity = 0; capacity <= want.size() + 1; capacity++) {
                std::unique_ptr<char[]> input(new char[n]);              /* exactly n bytes */
                std::memcpy(input.get(), c.input.data(), n);
                std::unique_ptr<int[]> ids(new int[capacity]), pos(new int[capacity]);
                std::fill(ids.get(), ids.get() + capacity, -7);
                std::fill(pos.get(), pos.get() + capacity, -7);
                size_t total = 12345;
                const PFAC_status_t st = PFACX_caseMatchFromHost(cs, input.get(), n, mode, capacity ? ids.get() : nullptr, capacity ? pos.get() : nullptr,
                                                                 capacity, &total);
                check(st == (want.size() > capacity ? PFACX_STATUS_OUTPUT_TRUNCATED : PFAC_STATUS_SUCCESS), c.name, "the status", platform, mode);
                check(total == want.size(), c.name, "the length of the list", platform, mode);
                check(std::memcmp(input.get(), c.input.data(), n) == 0, c.name, "the caller's bytes", platform, mode);
                for (size_t k = 0; k < capacity; k++) {
                    const bool listed = k < want.size();
                    check(listed ? (pos[k] == want[k].first && ids[k] == want[k].second) : (pos[k] == -7 && ids[k] == -7), c.name, "a pair", platform, mode);
                }
            }
        }
        check((size_t)most >= longest && most >= 1, c.name, "maxMatchesPerPosition is below what one position of this input has", platform, 0);
        std::copy(c.sensitive.begin(), c.sensitive.end(), flags.begin() + 1);
        flags[0] = 0;
        check(PFACX_caseClose(cs) == PFAC_STATUS_SUCCESS, c.name, "the close call", platform, 0);
        PFAC_destroy(h);
    }
}

void runRefusals()
{
    const std::vector<std::string> pats = {"GET", "get", "Host: "};
    const std::string file = textOf(pats);
    const unsigned char flags[4] = {0, 1, 1, 0};
    PFAC_handle_t h = caselessHandle(file, PFAC_PLATFORM_CPU);
    PFAC_handle_t plain = nullptr;
    PFACX_case_t cs = nullptr;
    const auto open = [&](PFAC_handle_t handle, const std::string &text, size_t numFlags) {
        return PFACX_caseOpen(handle, text.data(), text.size(), 0, flags, numFlags, &cs, nullptr);
    };
    bool ok = h && PFACX_createHostOnly(&plain) == PFAC_STATUS_SUCCESS &&
              PFACX_readPatternFromMemoryEx(plain, file.data(), file.size(), 0) == PFAC_STATUS_SUCCESS;
    ok = ok && open(plain, file, 4) == PFAC_STATUS_INVALID_PARAMETER && !cs;                        /* the handle is not caseless */
    ok = ok && open(h, textOf({"GET", "get"}), 4) == PFAC_STATUS_INVALID_PARAMETER && !cs;          /* another F */
    ok = ok && open(h, textOf({"GET", "gex", "Host: "}), 4) == PFAC_STATUS_INVALID_PARAMETER;       /* one folded line differs */
    ok = ok && open(h, textOf({"GET", "get", "Host:"}), 4) == PFAC_STATUS_INVALID_PARAMETER;        /* ... is shorter */
    ok = ok && open(h, file, 3) == PFAC_STATUS_INVALID_PARAMETER && !cs;                            /* numFlags < F + 1 */
    ok = ok && open(h, file, 4) == PFAC_STATUS_SUCCESS && cs;
    if (ok) {                                                                                       /* stale after a re-read; closed by PFAC_destroy */
        char input[] = "GET get";
        int ids[8], pos[8];
        size_t total = 0;
        ok = PFACX_caseMatchFromHost(cs, input, 7, 0, ids, pos, 8, &total) == PFAC_STATUS_SUCCESS && total == 2 && ids[0] == 1 && ids[1] == 2;
        ok = ok && PFACX_readPatternFromMemoryEx(h, file.data(), file.size(), PFACX_READ_NOCASE) == PFAC_STATUS_SUCCESS;
        ok = ok && PFACX_caseMatchFromHost(cs, input, 7, 0, ids, pos, 8, &total) == PFAC_STATUS_INVALID_PARAMETER;
    }
    if (!ok) { std::fprintf(stderr, "FAILED: the refusals of the open call or the stale object\n"); failures++; }
    if (h) PFAC_destroy(h);
    if (plain) PFAC_destroy(plain);
}

/* tests/case_ref.py: edge_pattern, flipped, edge_input */
const int kEdgeLengths[] = {1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 64};

std::string edgePattern(int index)
{
    std::string p;
    for (int i = 0; i < kEdgeLengths[index]; i++) p += (char)(('a' + index) ^ ((i & 1) ? 0x20 : 0));
    return p;
}

std::string flipped(std::string p, size_t at)
{
    p[at] = (char)(p[at] ^ 0x20);
    return p;
}

std::string edgeInput()
{
    std::string out;
    for (int k = 0; k < 12; k++) {
        const std::string pat = edgePattern(k);
        const size_t len = pat.size();
        const std::string four[4] = {pat, flipped(pat, 0), flipped(pat, len - 1), flipped(pat, std::min(len - 1, 4 * (len / 8) + 1))};
        for (int j = 0; j < 4; j++) out += four[(j + 4 - k % 4) % 4] + " ";
        out += std::string((size_t)(k % 3), '-') + " ";
    }
    const std::string longest = edgePattern(11);
    return out + longest.substr(0, longest.size() - 1) + " " + edgePattern(10);
}

} // namespace

int main()
{
    std::vector<std::string> edges, twins;
    for (int k = 0; k < 12; k++) edges.push_back(edgePattern(k));
    twins = edges;
    for (int k = 0; k < 12; k++) twins.push_back(folded(edges[(size_t)k]));
    std::vector<unsigned char> twinFlags(12, 1);
    twinFlags.resize(24, 0);
    const std::vector<Case> cases = {
        {"three-variants", {"GET", "get", "Get"}, {1, 1, 0}, "GET get gEt Get"},
        {"exact-duplicates-of-each-kind", {"ab", "AB", "ab", "Ab", "aB", "AB"}, {1, 1, 1, 0, 0, 1}, "ab AB Ab aB"},
        {"a-class-of-one-caseless-line", {"Key", "other"}, {0, 1}, "key KEY kEy ke Key other OTHER"},
        {"longest-sensitive-fails-or-passes-over-a-caseless-prefix", {"foo", "fooBar"}, {0, 1}, "foobar fooBar FOOBAR fooBa"},
        {"every-member-fails", {"Ab", "AbC"}, {1, 1}, "abc ABC aBc xab"},
        {"sensitive-prefix-caseless-longer", {"Foo", "foobar"}, {1, 0}, "FooBAR foobar Foo fOO fooba"},
        {"three-deep-chain", {"a", "Ab", "ab", "aBc", "ABC", "abc"}, {0, 1, 0, 1, 1, 1}, "abc ABC aBc Abc aBC ab a"},
        {"a-match-ends-at-n", {"Tail", "TailXY"}, {1, 1}, "TailXY TailX tail Tail"},
        {"a-candidate-runs-past-n", {"Tail", "TailXY"}, {1, 0}, "xx Tail tailxy TAILX"},
        {"fold-edges", {"@a[", "`A{", "\xc1" "b", "\xe1" "B", "z@", "Z`"}, {0, 1, 0, 1, 0, 1},
         "@A[ @a[ `a{ `A{ \xc1" "B \xc1" "b \xe1" "b \xe1" "B \xe1\x42 Z` z` z@ Z@ {a[ [A{"},
        {"compare-edges", edges, std::vector<unsigned char>(12, 1), edgeInput()},
        {"compare-edges-under-a-caseless-twin", twins, twinFlags, edgeInput()},
    };
    for (const Case &c : cases) runCase(c);
    {   /* the three-variant list of the header */
        const std::vector<std::pair<int, int>> all = byDefinition(cases[0], true);
        const std::vector<std::pair<int, int>> want = {{0, 3}, {0, 1}, {4, 3}, {4, 2}, {8, 3}, {12, 3}};
        if (all != want) { std::fprintf(stderr, "FAILED: the definition itself\n"); failures++; }
    }
    runRefusals();
    if (failures) return 1;
    std::printf("case_host_san: %zu cases x 2 platforms x 2 modes x every capacity agree with the definition; the open call refuses what it must\n", cases.size());
    return 0;
}
