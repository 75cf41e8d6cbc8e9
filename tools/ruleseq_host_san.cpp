/*
 * ruleseq_host_san.cpp -- PFACX_rulesOpenSeq and PFACX_rulesMatchFromHost on a host-only handle, for the sanitizer build of the host library (make -C
 * pfac_amd/csrc san: build/ruleseq_host_san links lib/san/libpfac.so; CPU only).  Chains over segments of a few and of several hundred pairs, on
 * both CPU platforms, at a capacity that fits and at ones that truncate (0, 1, the length minus 1), into arrays allocated at exactly `capacity` and
 * numSegments + 1 entries -- a write behind them is the sanitizer's to find -- compared with a search over all assignments made here; then the
 * refusals of the open call.  Exit status 0: every list agreed and every refusal was one.
 */
#include <cstdio>
#include <string>
#include <vector>

#include "PFAC.h"
#include "pfac_ext.h"

namespace {

constexpr unsigned int REL = PFACX_RULE_RELATIVE, NOT = PFACX_RULE_NOT, END = PFACX_RULE_FROM_END;
typedef PFACX_rule_seq_member_t M;

struct Case {
    const char *name;
    std::vector<std::string> patterns;
    std::vector<std::vector<M>> rules;
    std::vector<std::string> pieces;
};

bool inWindow(const M &m, size_t len, size_t s, size_t n)
{
    const unsigned long long a = (m.flags & END) ? n - s - len : s;
    return a >= m.offset && (m.depth == 0 || a + len <= (unsigned long long)m.offset + m.depth);
}

bool place(const Case &c, const std::vector<M> &ms, size_t j, size_t last, unsigned long long e, const std::string &piece)
{
    if (j == last) return true;
    const std::string &pat = c.patterns[(size_t)ms[j].pattern - 1];
    for (size_t s = piece.find(pat); s != std::string::npos; s = piece.find(pat, s + 1))
        if (inWindow(ms[j], pat.size(), s, piece.size()) && s >= e + ms[j].distance && (ms[j].within == 0 || s + pat.size() <= e + ms[j].within) &&
            place(c, ms, j + 1, last, s + pat.size(), piece))
            return true;
    return false;
}

bool fires(const Case &c, const std::vector<M> &ms, const std::string &piece)
{
    for (size_t j = 0; j < ms.size();) {
        size_t last = j + 1;
        while (last < ms.size() && (ms[last].flags & REL)) last++;
        const std::string &pat = c.patterns[(size_t)ms[j].pattern - 1];
        bool some = false;
        for (size_t s = piece.find(pat); s != std::string::npos && !some; s = piece.find(pat, s + 1))
            some = inWindow(ms[j], pat.size(), s, piece.size()) && place(c, ms, j + 1, last, s + pat.size(), piece);
        if (some == ((ms[j].flags & NOT) != 0)) return false;
        j = last;
    }
    return true;
}

int fail(const char *what, const char *name)
{
    fprintf(stderr, "FAILED: %s (%s)\n", what, name);
    return 1;
}

int runCase(const Case &c, int platform)
{
    std::string file, input;
    for (const std::string &p : c.patterns) file += p + "\n";
    std::vector<size_t> offsets = {0};
    for (const std::string &p : c.pieces) { input += p; offsets.push_back(input.size()); }
    std::vector<int> ruleOff = {0};
    std::vector<M> members;
    for (const std::vector<M> &r : c.rules) { members.insert(members.end(), r.begin(), r.end()); ruleOff.push_back((int)members.size()); }
    std::vector<int> wantSeg, wantRule;
    std::vector<size_t> wantFirst;
    for (size_t k = 0; k < c.pieces.size(); k++) {
        wantFirst.push_back(wantSeg.size());
        for (size_t r = 0; r < c.rules.size(); r++)
            if (fires(c, c.rules[r], c.pieces[k])) { wantSeg.push_back((int)k); wantRule.push_back((int)r); }
    }
    wantFirst.push_back(wantSeg.size());

    PFAC_handle_t h = nullptr;
    if (PFACX_createHostOnly(&h) != PFAC_STATUS_SUCCESS || PFAC_setPlatform(h, (PFAC_platform_t)platform) != PFAC_STATUS_SUCCESS ||
        PFACX_readPatternFromMemory(h, file.data(), file.size()) != PFAC_STATUS_SUCCESS)
        return fail("handle", c.name);
    PFACX_rules_t set = nullptr;
    if (PFACX_rulesOpenSeq(h, ruleOff.data(), members.data(), c.rules.size(), &set) != PFAC_STATUS_SUCCESS) return fail("open", c.name);
    const size_t total = wantSeg.size();
    for (const size_t capacity : {total, (size_t)0, (size_t)1, total ? total - 1 : 0}) {
        std::vector<int> seg(capacity), rule(capacity);
        std::vector<size_t> first(c.pieces.size() + 1);
        std::string copy = input;
        size_t fired = 0;
        const PFAC_status_t st = PFACX_rulesMatchFromHost(set, &copy[0], copy.size(), offsets.data(), c.pieces.size(), capacity ? seg.data() : nullptr,
                                                          capacity ? rule.data() : nullptr, capacity, first.data(), &fired);
        if (st != (capacity < total ? PFACX_STATUS_OUTPUT_TRUNCATED : PFAC_STATUS_SUCCESS) || fired != total) return fail("status or count", c.name);
        const size_t kept = capacity < total ? capacity : total;
        for (size_t i = 0; i < kept; i++)
            if (seg[i] != wantSeg[i] || rule[i] != wantRule[i]) return fail("list", c.name);
        if (first != wantFirst || copy != input) return fail("segFirst or input", c.name);
    }
    if (PFACX_rulesClose(set) != PFAC_STATUS_SUCCESS || PFAC_destroy(h) != PFAC_STATUS_SUCCESS) return fail("close", c.name);
    return 0;
}

int refusals()
{
    const std::string file = "a\nb\nc\n";
    PFAC_handle_t h = nullptr;
    if (PFACX_createHostOnly(&h) != PFAC_STATUS_SUCCESS || PFACX_readPatternFromMemory(h, file.data(), file.size()) != PFAC_STATUS_SUCCESS)
        return fail("handle", "refusals");
    const std::vector<std::vector<M>> bad = {
        {{1, REL, 0, 0, 0, 0}},                                    /* RELATIVE on the first member */
        {{1, 0, 0, 0, 0, 0}, {2, REL | NOT, 0, 0, 0, 0}},          /* together with NOT */
        {{1, 0, 0, 0, 0, 0}, {2, NOT, 0, 0, 0, 0}, {3, REL, 0, 0, 0, 0}},      /* behind a NOT member */
        {{1, 0, 0, 0, 1, 0}},                                      /* distance without RELATIVE */
        {{1, 0, 0, 0, 0, 1}},                                      /* within without RELATIVE */
        {{1, 8, 0, 0, 0, 0}},                                      /* an unknown flag bit */
        {{4, 0, 0, 0, 0, 0}, {1, REL, 0, 0, 0, 0}},                /* an id above F */
    };
    for (const std::vector<M> &r : bad) {
        const int off[2] = {0, (int)r.size()};
        PFACX_rules_t set = reinterpret_cast<PFACX_rules_t>(&h);
        if (PFACX_rulesOpenSeq(h, off, r.data(), 1, &set) != PFAC_STATUS_INVALID_PARAMETER || set != nullptr) return fail("a refusal", "refusals");
    }
    std::vector<M> many(33, M{1, REL, 0, 0, 0, 0});
    many[0].flags = 0;
    const int off[2] = {0, 33};
    PFACX_rules_t set = nullptr;
    if (PFACX_rulesOpenSeq(h, off, many.data(), 1, &set) != PFAC_STATUS_INVALID_PARAMETER) return fail("33 members", "refusals");
    return PFAC_destroy(h) == PFAC_STATUS_SUCCESS ? 0 : fail("destroy", "refusals");
}

} // namespace

int main()
{
    const std::string trips = "A" + std::string(255, 'x') + "B" + std::string(255, 'x') + "C";
    const std::vector<Case> cases = {
        {"traps", {"XX", "AA", "BB"},
         {{{1, 0, 0, 0, 0, 0}, {2, REL, 0, 0, 0, 0}, {3, REL, 0, 0, 0, 4}}, {{1, 0, 0, 0, 0, 0}, {2, REL, 0, 0, 0, 5}, {3, REL, 0, 0, 0, 4}},
          {{2, 0, 0, 0, 0, 0}, {3, REL, 0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu}}, {{2, 0, 0, 0, 0, 0}, {3, REL | END, 0, 2, 1, 0}, {1, NOT, 0, 2, 0, 0}}},
         {"XX.AA.BB.AA", "XX.AA......AA.BB", "XX.AA.....AA.BB", "", "AA.BB", "AABB"}},
        {"same-pattern-twice-and-two-chains", {"aa", "b"},
         {{{1, 0, 0, 0, 0, 0}, {1, REL, 0, 0, 0, 0}}, {{1, 0, 0, 0, 0, 0}, {2, REL, 0, 0, 0, 0}, {1, 0, 0, 0, 0, 0}, {1, REL, 0, 0, 1, 0}}},
         {"aaa", "aaaa", "aab", "aa.aab", ""}},
        {"links-in-different-trips", {"x", "A", "B", "C"},
         {{{2, 0, 0, 0, 0, 0}, {3, REL, 0, 0, 255, 0}, {4, REL, 0, 0, 255, 256}}, {{2, 0, 0, 0, 0, 0}, {3, REL, 0, 0, 256, 0}},
          {{1, 0, 0, 0, 0, 0}, {1, REL, 0, 0, 509, 0}}, {{1, 0, 0, 0, 0, 0}, {1, REL, 0, 0, 510, 0}}},
         {trips, trips.substr(0, 257), "x", trips.substr(1)}},
    };
    for (const Case &c : cases)
        for (const int platform : {(int)PFAC_PLATFORM_CPU, (int)PFAC_PLATFORM_CPU_OMP})
            if (runCase(c, platform)) return 1;
    if (refusals()) return 1;
    printf("ruleseq_host_san: %zu cases x 2 platforms and the refusals agreed\n", cases.size());
    return 0;
}
