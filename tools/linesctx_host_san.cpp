/*
 * linesctx_host_san.cpp -- PFACX_matchLinesContextFromHost on a host-only handle over the edge inputs of tests/linesctx_ref.py, for the sanitizer
 * build of the host library (make -C pfac_amd/csrc san: build/linesctx_host_san links lib/san/libpfac.so; CPU only).  Every input runs on both CPU
 * platforms, with and without PFACX_LINES_INVERT, over a grid of (before, after) that holds 0, the word edges 31 / 32 / 33, more than the input has
 * lines and 0xFFFFFFFF, with and without lineIndex and lineTag, into arrays allocated at exactly `capacity` == size entries -- a write behind them
 * is the sanitizer's to find -- and is compared with the definition, evaluated here line by line.  Exit status 0: every list agreed.
 */
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "PFAC.h"
#include "pfac_ext.h"

namespace {

struct Case {
    const char *name;
    std::vector<std::string> patterns;
    std::string input;
    bool nocase;
};

unsigned char fold(unsigned char b, bool nocase) { return nocase && b >= 'A' && b <= 'Z' ? (unsigned char)(b + 32) : b; }

std::string folded(const std::string &s, bool nocase)
{
    std::string out = s;
    for (char &ch : out) ch = (char)fold((unsigned char)ch, nocase);
    return out;
}

/* `num` lines, empty at odd numbers and "z" at even ones, "x" at the numbers in `hits` */
std::string tinyLines(size_t num, const std::vector<size_t> &hits, bool terminated = true)
{
    std::string out;
    for (size_t k = 0; k < num; k++) {
        bool hit = false;
        for (size_t h : hits) hit = hit || h == k;
        out += hit ? "x" : (k & 1 ? "" : "z");
        if (k + 1 < num || terminated) out += "\n";
    }
    return out;
}

std::string rep(const std::string &s, size_t k)
{
    std::string out;
    for (size_t i = 0; i < k; i++) out += s;
    return out;
}

struct Want {
    std::vector<int> start, len, index, tag;
    size_t lines = 0, matching = 0, groups = 0;
};

/* the definition: H from strstr per line, then k is selected if some h of H has h - before <= k <= h + after, in 64-bit arithmetic */
Want byDefinition(const Case &c, bool invert, unsigned int before, unsigned int after)
{
    std::vector<size_t> s, e;
    const std::string &in = c.input;
    for (size_t at = 0; at < in.size();) {
        size_t q = in.find('\n', at);
        if (q == std::string::npos) q = in.size();
        s.push_back(at);
        e.push_back(q);
        at = q + 1;
    }
    const size_t n = s.size();
    std::vector<char> member(n, 0), selected(n, 0);
    for (size_t k = 0; k < n; k++) {
        const std::string line = folded(in.substr(s[k], e[k] - s[k]), c.nocase);
        bool hit = false;
        for (const std::string &p : c.patterns) hit = hit || line.find(folded(p, c.nocase)) != std::string::npos;
        member[k] = hit != invert;
    }
    Want w;
    w.lines = n;
    for (size_t h = 0; h < n; h++) {
        if (!member[h]) continue;
        w.matching++;
        const long long lo = (long long)h - (long long)before, hi = (long long)h + (long long)after;
        for (long long k = lo < 0 ? 0 : lo; k <= hi && k < (long long)n; k++) selected[(size_t)k] = 1;
    }
    for (size_t k = 0; k < n; k++) {
        if (!selected[k]) continue;
        if (k == 0 || !selected[k - 1]) w.groups++;
        w.start.push_back((int)s[k]);
        w.len.push_back((int)(e[k] - s[k]));
        w.index.push_back((int)k);
        w.tag.push_back((int)(((w.groups - 1) << 1) | (member[k] ? 1u : 0u)));
    }
    return w;
}

int failures = 0;

void check(bool ok, const Case &c, const char *what, int platform, bool invert, unsigned int before, unsigned int after)
{
    if (ok) return;
    failures++;
    std::fprintf(stderr, "FAILED %s: %s (platform %d, invert %d, before %u, after %u)\n", c.name, what, platform, (int)invert, before, after);
}

size_t calls = 0;

void runCase(const Case &c)
{
    std::string file;
    for (const std::string &p : c.patterns) file += p + "\n";
    const unsigned int windows[] = {0u, 1u, 3u, 31u, 32u, 33u, 5000u, 0xFFFFFFFFu};
    for (int platform : {PFAC_PLATFORM_CPU, PFAC_PLATFORM_CPU_OMP}) {
        PFAC_handle_t h = nullptr;
        if (PFACX_createHostOnly(&h) != PFAC_STATUS_SUCCESS || PFAC_setPlatform(h, (PFAC_platform_t)platform) != PFAC_STATUS_SUCCESS ||
            PFACX_readPatternFromMemoryEx(h, file.data(), file.size(), c.nocase ? PFACX_READ_NOCASE : 0u) != PFAC_STATUS_SUCCESS) {
            check(false, c, "the handle", platform, false, 0, 0);
            if (h) PFAC_destroy(h);
            continue;
        }
        for (bool invert : {false, true})
            for (unsigned int before : windows)
                for (unsigned int after : windows) {
                    const Want want = byDefinition(c, invert, before, after);
                    for (int nulls = 0; nulls < 4; nulls++) {              /* bit 0: no lineIndex, bit 1: no lineTag */
                        if (nulls && (before != 1u || after != 33u)) continue;
                        std::string input = c.input;                    /* the call takes a char *: it must hand the bytes back as they were */
                        const size_t capacity = input.size();
                        std::vector<int> start(capacity, -7), len(capacity, -7), index(capacity, -7), tag(capacity, -7);
                        size_t nl = 12345, ns = 12345, nm = 12345, ng = 12345;
                        const PFAC_status_t st = PFACX_matchLinesContextFromHost(
                            h, &input[0], input.size(), invert ? PFACX_LINES_INVERT : 0u, before, after, start.data(), len.data(),
                            (nulls & 1) ? nullptr : index.data(), (nulls & 2) ? nullptr : tag.data(), capacity, &nl, &ns, &nm, &ng);
                        calls++;
                        check(st == PFAC_STATUS_SUCCESS, c, "the status", platform, invert, before, after);
                        check(input == c.input, c, "the caller's bytes", platform, invert, before, after);
                        check(nl == want.lines && ns == want.start.size() && nm == want.matching && ng == want.groups, c, "the counts", platform, invert,
                              before, after);
                        if (ns != want.start.size()) continue;
                        bool same = true;
                        for (size_t k = 0; k < ns; k++) {
                            same = same && start[k] == want.start[k] && len[k] == want.len[k];
                            same = same && ((nulls & 1) ? index[k] == -7 : index[k] == want.index[k]);
                            same = same && ((nulls & 2) ? tag[k] == -7 : tag[k] == want.tag[k]);
                        }
                        check(same, c, "the list", platform, invert, before, after);
                    }
                }
        PFAC_destroy(h);
    }
}

} // namespace

int main()
{
    const std::vector<std::string> x = {"x"};
    std::vector<Case> cases = {
        {"hit-on-line-0", x, tinyLines(9, {0}), false},
        {"hit-on-the-last-line", x, tinyLines(9, {8}), false},
        {"hit-on-an-unterminated-last-line", x, tinyLines(9, {8}, false), false},
        {"a-single-line", x, "x\n", false},
        {"a-single-unterminated-byte", x, "x", false},
        {"only-a-newline", x, "\n", false},
        {"no-hit-at-all", x, tinyLines(70, {}), false},
        {"every-line-matches-1", x, rep("x\n", 1), false},
        {"every-line-matches-31", x, rep("x\n", 31), false},
        {"every-line-matches-32", x, rep("x\n", 32), false},
        {"every-line-matches-33", x, rep("x\n", 33), false},
        {"every-line-matches-64", x, rep("x\n", 64), false},
        {"every-line-matches-2049", x, rep("x\n", 2049), false},
        {"two-hits-ten-apart", x, tinyLines(40, {10, 20}), false},
        {"hits-around-the-word-edges", x, tinyLines(130, {0, 31, 32, 63, 64, 127, 129}), false},
        {"5000-empty-lines-one-hit", x, rep("\n", 2500) + "x\n" + rep("\n", 2499), false},
        {"unterminated-last-line-that-does-not-match", {"z"}, "q\nz\nq\nz\nz\nz\nz\nq", false},
        {"caseless", {"Needle"}, "plain\nnothing\na NEEDLE here\nplain\nmore\nneedle\nlast\n", true},
        {"crlf", {"ab", "needle"}, "one ab\r\ntwo\r\n\r\nthree needle\r\nfour\r\nfive\r\n", false},
    };
    for (size_t hit : {0u, 31u, 32u, 33u, 63u, 64u, 99u}) cases.push_back({"one-hit-at-a-word-edge", x, tinyLines(100, {hit}), false});
    for (const Case &c : cases) runCase(c);
    /* the rows that touch nothing */
    {
        PFAC_handle_t h = nullptr;
        size_t counts[4] = {5, 5, 5, 5};
        int one[4] = {-7, -7, -7, -7};
        char byte = 'x';
        const bool ok = PFACX_createHostOnly(&h) == PFAC_STATUS_SUCCESS && PFAC_setPlatform(h, PFAC_PLATFORM_CPU) == PFAC_STATUS_SUCCESS &&
                        PFACX_readPatternFromMemoryEx(h, "x\n", 2, 0u) == PFAC_STATUS_SUCCESS &&
                        PFACX_matchLinesContextFromHost(h, &byte, 0, 0u, 3, 3, one, one + 1, one + 2, one + 3, 0, counts, counts + 1, counts + 2, counts + 3) ==
                            PFAC_STATUS_SUCCESS &&
                        counts[0] + counts[1] + counts[2] + counts[3] == 0 && one[0] == -7 && one[1] == -7 && one[2] == -7 && one[3] == -7 &&
                        PFACX_matchLinesContextFromHost(h, &byte, 1, 0u, 3, 3, one, one + 1, one + 2, one + 3, 0, counts, counts + 1, counts + 2, counts + 3) ==
                            PFAC_STATUS_INVALID_PARAMETER &&
                        PFACX_matchLinesContextFromHost(h, &byte, 1, 2u, 3, 3, one, one + 1, one + 2, one + 3, 1, counts, counts + 1, counts + 2, counts + 3) ==
                            PFAC_STATUS_INVALID_PARAMETER &&
                        PFACX_matchLinesContextFromDevice(h, &byte, 1, 0u, 3, 3, one, one + 1, one + 2, one + 3, 1, counts, counts + 1, counts + 2, counts + 3) ==
                            PFAC_STATUS_LIB_NOT_EXIST &&
                        one[0] == -7;
        if (!ok) {
            std::fprintf(stderr, "FAILED: size == 0, capacity < size, an unknown flag or the device form on a host-only handle\n");
            failures++;
        }
        if (h) PFAC_destroy(h);
    }
    if (failures) return 1;
    std::printf("linesctx_host_san: %zu inputs, %zu calls agree with the definition\n", cases.size(), calls);
    return 0;
}
