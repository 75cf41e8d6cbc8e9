/*
 * groups_host_san.cpp -- PFACX_groupsMatchFromHost on a host-only handle over the case table of tests/groups_ref.py, for the sanitizer build of the
 * host library (make -C pfac_amd/csrc san: build/groups_host_san links lib/san/libpfac.so; CPU only).  Every case runs in both modes, on both CPU
 * platforms -- the longest pairs of every segment come from HostBatchPairs (batch_api.cpp), which the rules and the count-batch host forms share --,
 * at a capacity that fits and at ones that truncate (0, 1, the length minus 1), into arrays allocated at exactly `capacity`, numSegments +
 * 1 and numSegments entries -- a write behind them is the sanitizer's to find -- and is compared with the definition, evaluated here position by
 * position.  Exit status 0: every list agreed.
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

typedef unsigned long long u64;

struct Case {
    const char *name;
    std::vector<std::string> patterns;
    std::vector<u64> masks;                  /* by id, entry 0 unused */
    std::string input;
    std::vector<size_t> offsets;             /* empty: offsets == NULL, one segment */
    std::vector<u64> segMasks;               /* empty: segMasks == NULL */
    bool nocase;
};

std::string rep(const std::string &s, int k)
{
    std::string out;
    for (int i = 0; i < k; i++) out += s;
    return out;
}

unsigned char fold(unsigned char b, bool nocase) { return nocase && b >= 'A' && b <= 'Z' ? (unsigned char)(b + 32) : b; }

bool equalFolded(const std::string &a, const std::string &b, bool nocase)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (fold((unsigned char)a[i], nocase) != fold((unsigned char)b[i], nocase)) return false;
    return true;
}

struct Want {
    std::vector<std::pair<int, int>> pairs;  /* (position, id) */
    std::vector<size_t> first;
    std::vector<u64> groups;
};

/* the definition: per segment every occurrence that lies inside it, of equal lines the highest id with the OR of their masks, longest first */
Want byDefinition(const Case &c, bool all)
{
    const size_t F = c.patterns.size();
    std::vector<u64> m(F + 1, 0);
    std::vector<bool> reported(F + 1, false);
    for (size_t k = 0; k < F; k++) {
        size_t to = k;
        for (size_t j = k + 1; j < F; j++)
            if (equalFolded(c.patterns[j], c.patterns[k], c.nocase)) to = j;
        m[to + 1] |= c.masks[k + 1];
        reported[to + 1] = true;
    }
    const std::vector<size_t> whole = {0, c.input.size()};
    const std::vector<size_t> &off = c.offsets.empty() ? whole : c.offsets;
    Want w;
    w.first.push_back(0);
    for (size_t s = 0; s + 1 < off.size(); s++) {
        const u64 sm = c.segMasks.empty() ? ~0ull : c.segMasks[s];
        u64 hit = 0;
        for (size_t p = off[s]; p < off[s + 1]; p++) {
            std::vector<std::tuple<int, int>> found;             /* -length, id */
            for (size_t id = 1; id <= F; id++) {
                const std::string &pat = c.patterns[id - 1];
                if (!reported[id] || pat.empty() || p + pat.size() > off[s + 1] || !(m[id] & sm)) continue;
                if (!equalFolded(c.input.substr(p, pat.size()), pat, c.nocase)) continue;
                found.emplace_back(-(int)pat.size(), (int)id);
                hit |= m[id] & sm;
            }
            std::sort(found.begin(), found.end());
            for (size_t k = 0; k < found.size() && (all || k == 0); k++) w.pairs.emplace_back((int)p, std::get<1>(found[k]));
        }
        w.first.push_back(w.pairs.size());
        w.groups.push_back(hit);
    }
    return w;
}

int failures = 0;

void check(bool ok, const Case &c, const char *what, int platform, unsigned int flags, size_t capacity)
{
    if (ok) return;
    failures++;
    std::fprintf(stderr, "FAILED %s: %s (platform %d, flags %u, capacity %zu)\n", c.name, what, platform, flags, capacity);
}

void runCase(const Case &c)
{
    std::string file;
    for (const std::string &p : c.patterns) file += p + "\n";
    const size_t segments = c.offsets.empty() ? 1 : c.offsets.size() - 1;
    for (int platform : {PFAC_PLATFORM_CPU, PFAC_PLATFORM_CPU_OMP}) {
        PFAC_handle_t h = nullptr;
        PFACX_groups_t g = nullptr;
        if (PFACX_createHostOnly(&h) != PFAC_STATUS_SUCCESS || PFAC_setPlatform(h, (PFAC_platform_t)platform) != PFAC_STATUS_SUCCESS ||
            PFACX_readPatternFromMemoryEx(h, file.data(), file.size(), c.nocase ? PFACX_READ_NOCASE : 0u) != PFAC_STATUS_SUCCESS ||
            PFACX_groupsOpen(h, c.masks.data(), c.masks.size(), &g) != PFAC_STATUS_SUCCESS) {
            check(false, c, "the handle", platform, 0, 0);
            if (h) PFAC_destroy(h);
            continue;
        }
        for (unsigned int flags : {0u, PFACX_GROUPS_ALL}) {
            const Want want = byDefinition(c, flags != 0);
            const size_t total = want.pairs.size();
            for (size_t capacity : {total, (size_t)0, (size_t)1, total ? total - 1 : 0}) {
                std::string input = c.input;                    /* the call takes a char *: it must hand the bytes back as they were */
                std::vector<int> ids(capacity, -7), pos(capacity, -7);
                std::vector<size_t> first(segments + 1, 12345);
                std::vector<u64> groups(segments, 12345);
                std::vector<size_t> offsets = c.offsets;
                std::vector<u64> segMasks = c.segMasks;
                size_t n = 12345;
                const PFAC_status_t st = PFACX_groupsMatchFromHost(g, &input[0], input.size(), offsets.empty() ? nullptr : offsets.data(), segments,
                                                                   segMasks.empty() ? nullptr : segMasks.data(), flags, capacity ? ids.data() : nullptr,
                                                                   capacity ? pos.data() : nullptr, capacity, first.data(), groups.data(), &n);
                check(st == (total > capacity ? PFACX_STATUS_OUTPUT_TRUNCATED : PFAC_STATUS_SUCCESS), c, "the status", platform, flags, capacity);
                check(n == total, c, "the length of the list", platform, flags, capacity);
                check(input == c.input, c, "the caller's bytes", platform, flags, capacity);
                check(first == want.first, c, "segFirst", platform, flags, capacity);
                check(groups == want.groups, c, "segGroups", platform, flags, capacity);
                for (size_t k = 0; k < capacity; k++) {
                    const bool listed = k < total;
                    check(listed ? (pos[k] == want.pairs[k].first && ids[k] == want.pairs[k].second) : (pos[k] == -7 && ids[k] == -7), c, "a pair", platform,
                          flags, capacity);
                }
            }
        }
        if (PFACX_groupsClose(g) != PFAC_STATUS_SUCCESS) check(false, c, "the close", platform, 0, 0);
        PFAC_destroy(h);
    }
}

} // namespace

int main()
{
    const u64 B31 = 1ull << 31, B32 = 1ull << 32, B63 = 1ull << 63;
    std::vector<std::string> nested;
    std::vector<u64> nestedMasks = {0};
    for (int k = 1; k <= 8; k++) { nested.push_back(rep("a", k)); nestedMasks.push_back(1ull << (k - 1)); }
    const std::vector<Case> cases = {
        {"foo-foobar-masks-1-2-3-0", {"foo", "foobar"}, {0, 1, 2}, rep("foobar foo", 4), {0, 10, 20, 30, 40}, {1, 2, 3, 0}, false},
        {"chain-of-three-middle-enabled", {"ab", "abc", "abcd"}, {0, 1, 2, 4}, "abcd abc ab", {0, 11}, {2}, false},
        {"duplicate-lines-bits-0-and-63", {"ab", "cd", "ab"}, {0, 1, 2, B63}, "ab cd ab", {0, 3, 6, 8}, {1, B63, B63}, false},
        {"a-pattern-with-mask-0", {"x", "xy"}, {0, 0, 5}, "xy x", {}, {}, false},
        {"bit-31-against-bit-32", {"p", "q"}, {0, B31, B32}, "pq pq", {0, 3, 5}, {B32, B31}, false},
        {"a-match-across-a-border", {"abcd", "ab"}, {0, 1, 1}, "xabcdx", {0, 3, 6}, {1, 1}, false},
        {"empty-segments", {"a"}, {0, 1}, "aa", {0, 0, 1, 1, 1, 1, 2, 2}, {}, false},
        {"one-byte-segments", {"a", "b", "ab"}, {0, 1, 2, 4}, "abab", {0, 1, 2, 3, 4}, {3, 3, 1, 2}, false},
        {"nested-a-longer-than-the-input", nested, nestedMasks, rep("a", 12), {0, 12}, {}, false},
        {"nested-a-every-other-group", nested, nestedMasks, rep("a", 12), {0, 5, 12}, {0xAA, 0x55}, false},
        {"the-whole-buffer-is-one-segment", {"foo", "foobar"}, {0, 1, 2}, "foobar foo", {}, {1}, false},
        {"caseless", {"Foo", "FOOBAR"}, {0, 1, 2}, "fooBAR FOO", {}, {1}, true},
        {"a-run-of-4000", {"a", "aa", "aaa"}, {0, 1, 2, 4}, rep("a", 4000), {0, 1, 1999, 4000}, {5, 2, 7}, false},
    };
    for (const Case &c : cases) runCase(c);
    if (byDefinition(cases[0], false).pairs.size() != 5 || byDefinition(cases[0], true).pairs.size() != 6) {
        std::fprintf(stderr, "FAILED: the definition itself\n");
        failures++;
    }
    if (failures) return 1;
    std::printf("groups_host_san: %zu cases x 2 platforms x 2 modes x 4 capacities agree with the definition\n", cases.size());
    return 0;
}
