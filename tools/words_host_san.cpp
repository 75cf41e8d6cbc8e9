/*
 * words_host_san.cpp -- PFACX_matchWordsFromHost on a host-only handle over the case table of tests/words_ref.py, for the sanitizer build of the host
 * library (make -C pfac_amd/csrc san: build/words_host_san links lib/san/libpfac.so; CPU only).  Every case runs in both modes, on both CPU
 * platforms, at a capacity that fits and at one that truncates, into arrays allocated at exactly `capacity` entries -- a write behind them is the
 * sanitizer's to find -- and is compared with the definition, evaluated here position by position.  Exit status 0: every list agreed.
 */
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "PFAC.h"
#include "pfac_ext.h"

namespace {

struct Case {
    const char *name;
    std::vector<std::string> patterns;
    std::string input;
    int cls;                     /* 0 default, 1 empty, 2 full, 3 all but '\n', 4 all but ',' and '\n', 5 a-z */
    bool nocase;
};

std::string rep(const std::string &s, int k)
{
    std::string out;
    for (int i = 0; i < k; i++) out += s;
    return out;
}

std::vector<std::string> nested()
{
    std::vector<std::string> p;
    for (int k = 1; k <= 8; k++) p.push_back(rep("a", k));
    return p;
}

void classWords(int cls, unsigned int w[8])
{
    for (int k = 0; k < 8; k++) w[k] = cls == 1 ? 0u : 0xFFFFFFFFu;
    auto drop = [&](unsigned char b) { w[b >> 5] &= ~(1u << (b & 31)); };
    if (cls == 3) drop('\n');
    if (cls == 4) { drop('\n'); drop(','); }
    if (cls == 0 || cls == 5) {
        for (int k = 0; k < 8; k++) w[k] = 0;
        for (int b = 0; b < 256; b++) {
            const bool in = cls == 5 ? (b >= 'a' && b <= 'z') : ((b >= '0' && b <= '9') || (b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z') || b == '_');
            if (in) w[b >> 5] |= 1u << (b & 31);
        }
    }
}

unsigned char fold(unsigned char b, bool nocase) { return nocase && b >= 'A' && b <= 'Z' ? (unsigned char)(b + 32) : b; }

/* the definition: (position, id) of every bounded occurrence, ascending position, longest first; !all: the first of each position */
std::vector<std::pair<int, int>> byDefinition(const Case &c, const unsigned int w[8], bool all)
{
    auto inW = [&](unsigned char b) { return (w[b >> 5] >> (b & 31)) & 1u; };
    const std::string &in = c.input;
    const size_t n = in.size();
    std::vector<std::tuple<int, int, int>> found;               /* position, -length, id */
    for (size_t p = 0; p < n; p++) {
        if (p > 0 && inW((unsigned char)in[p - 1])) continue;
        for (size_t k = 0; k < c.patterns.size(); k++) {
            const std::string &pat = c.patterns[k];
            bool later = false;                                  /* duplicate lines report under the highest id */
            for (size_t j = k + 1; j < c.patterns.size() && !later; j++) {
                later = c.patterns[j].size() == pat.size();
                for (size_t i = 0; i < pat.size() && later; i++) later = fold((unsigned char)c.patterns[j][i], c.nocase) == fold((unsigned char)pat[i], c.nocase);
            }
            if (later || pat.empty() || p + pat.size() > n) continue;
            bool same = true;
            for (size_t i = 0; i < pat.size() && same; i++) same = fold((unsigned char)in[p + i], c.nocase) == fold((unsigned char)pat[i], c.nocase);
            if (!same || (p + pat.size() < n && inW((unsigned char)in[p + pat.size()]))) continue;
            found.emplace_back((int)p, -(int)pat.size(), (int)k + 1);
        }
    }
    std::sort(found.begin(), found.end());
    std::vector<std::pair<int, int>> out;
    for (const auto &f : found)
        if (all || out.empty() || out.back().first != std::get<0>(f)) out.emplace_back(std::get<0>(f), std::get<2>(f));
    return out;
}

int failures = 0;

void check(bool ok, const Case &c, const char *what, int platform, unsigned int flags)
{
    if (ok) return;
    failures++;
    std::fprintf(stderr, "FAILED %s: %s (platform %d, flags %u)\n", c.name, what, platform, flags);
}

void runCase(const Case &c)
{
    std::string file;
    for (const std::string &p : c.patterns) file += p + "\n";
    unsigned int w[8];
    classWords(c.cls, w);
    for (int platform : {PFAC_PLATFORM_CPU, PFAC_PLATFORM_CPU_OMP}) {
        PFAC_handle_t h = nullptr;
        if (PFACX_createHostOnly(&h) != PFAC_STATUS_SUCCESS || PFAC_setPlatform(h, (PFAC_platform_t)platform) != PFAC_STATUS_SUCCESS ||
            PFACX_readPatternFromMemoryEx(h, file.data(), file.size(), c.nocase ? PFACX_READ_NOCASE : 0u) != PFAC_STATUS_SUCCESS) {
            check(false, c, "the handle", platform, 0);
            if (h) PFAC_destroy(h);
            continue;
        }
        for (unsigned int flags : {0u, PFACX_WORDS_ALL}) {
            const std::vector<std::pair<int, int>> want = byDefinition(c, w, flags != 0);
            const size_t n = c.input.size();
            for (size_t capacity : {std::max(n, want.size()), n}) {
                std::string input = c.input;                    /* the call takes a char *: it must hand the bytes back as they were */
                std::vector<int> ids(capacity, -7), pos(capacity, -7);
                size_t total = 12345;
                const PFAC_status_t st = PFACX_matchWordsFromHost(h, &input[0], n, c.cls == 0 ? nullptr : w, flags, ids.data(), pos.data(), capacity, &total);
                check(st == (want.size() > capacity ? PFACX_STATUS_OUTPUT_TRUNCATED : PFAC_STATUS_SUCCESS), c, "the status", platform, flags);
                check(total == want.size(), c, "the length of the list", platform, flags);
                check(input == c.input, c, "the caller's bytes", platform, flags);
                for (size_t k = 0; k < capacity; k++) {
                    const bool listed = k < want.size();
                    check(listed ? (pos[k] == want[k].first && ids[k] == want[k].second) : (pos[k] == -7 && ids[k] == -7), c, "a pair", platform, flags);
                }
            }
        }
        PFAC_destroy(h);
    }
}

} // namespace

int main()
{
    const std::vector<std::string> spaced = {"a", "a a", "a a a", "a a a a", "a a a a a"};
    const std::vector<Case> cases = {
        {"at-0-and-ends-at-n", {"foo", "bar"}, "foo x bar", 0, false},
        {"longest-fails-prefix-passes", {"foo", "foobar"}, "foo bar foobar foobarx foo", 0, false},
        {"every-member-fails", {"ab", "abc"}, "xabcd abcd", 0, false},
        {"one-byte-patterns", {"a", "I", "-"}, "a I am-a - aa", 0, false},
        {"edge-bytes-outside-the-class", {"-x-", "+", "c++"}, "a -x- b-x-c c++ d+e +", 0, false},
        {"nested-a", nested(), rep("a", 5) + " " + rep("a", 8) + " " + rep("a", 9) + ".aa", 0, false},
        {"fifteen-pairs-in-nine-bytes", spaced, "a a a a a", 0, false},
        {"empty-class", {"ab", "abc", "b", "cab"}, "abcab.b abc", 1, false},
        {"empty-class-nested", nested(), "b" + rep("a", 11) + "b" + rep("a", 3), 1, false},
        {"full-class", {"whole", "whole buffer", "buffer"}, "whole buffer", 2, false},
        {"full-class-nothing", {"ab", "b"}, "abab", 2, false},
        {"grep-x-with-a-last-newline", {"line", "line two", "x"}, "line\nline two\nline twox\nx line\nx\n", 3, false},
        {"grep-x-without-a-last-newline", {"line", "line two", "x"}, "x\n\nline two\nline", 3, false},
        {"csv-fields", {"key", "key1", "k"}, "key,key1,xkey,k\nkey1x,k,key", 4, false},
        {"caseless-asymmetric-class", {"Key", "KEYS"}, "xKEYx XkeyX akeysa AKeYsA AKEYSa", 5, true},
        {"caseless-default-class", {"Needle", "NEE", "get"}, "a NEEDLE, nEe-GeT needles Get", 0, true},
        {"duplicate-lines", {"ab", "cd", "ab"}, "ab cd abcd ab", 0, false},
        {"a-run-of-4000", {"a", "aa", "aaa"}, rep("a", 4000), 1, false},
    };
    for (const Case &c : cases) runCase(c);
    {   /* the 15 pairs of the header's example */
        unsigned int w[8];
        classWords(0, w);
        if (byDefinition(cases[6], w, true).size() != 15) { std::fprintf(stderr, "FAILED: the definition itself\n"); failures++; }
    }
    if (failures) return 1;
    std::printf("words_host_san: %zu cases x 2 platforms x 2 modes x 2 capacities agree with the definition\n", cases.size());
    return 0;
}
