/*
 * segframe_host_san.cpp -- the host forms that share the list frame of pfac_host.h (sortedSegmentLists, touchedRuleMasks):
 * PFACX_countBatchFromHost with and without PFACX_COUNT_LONGEST, PFACX_rulesMatchFromHost over a plain and a conditioned set, and
 * PFACX_flowRulesPairsFromHost, on a host-only handle, for the sanitizer build of the host library (make -C pfac_amd/csrc san:
 * build/segframe_host_san links lib/san/libpfac.so; CPU only).  A handful of tiny batches -- empty first, middle and last segments, a match across a
 * border, offsets == NULL -- on both CPU platforms, at EVERY capacity from 0 to the length of the list plus 1: the input, the offsets and every output
 * array are heap blocks of exactly their size (capacity 0: null outputs), so a write behind one is the sanitizer's to find, and each list is
 * compared with the definition, evaluated here position by position.  A flow-rules call that was truncated is repeated with room and must then
 * fire the whole list: the truncated call committed nothing.  Exit status 0: every list agreed.
 */
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "PFAC.h"
#include "pfac_ext.h"

namespace {

const std::vector<std::string> kPatterns = {"a", "aa", "aaa", "b", "ab"};       /* ids 1 .. 5; a < aa < aaa and a < ab are prefix chains */

struct Batch {
    std::string input;
    std::vector<size_t> offsets;             /* empty: offsets == NULL, one segment */
};

int failures = 0;

void check(bool ok, const char *call, const char *what, size_t batch, size_t capacity)
{
    if (ok) return;
    failures++;
    std::fprintf(stderr, "FAILED %s: %s (batch %zu, capacity %zu)\n", call, what, batch, capacity);
}

/* a heap block of exactly n entries with a copy of v in it */
template <class T>
std::unique_ptr<T[]> exactly(const T *v, size_t n)
{
    std::unique_ptr<T[]> p(new T[n]);
    std::copy(v, v + n, p.get());
    return p;
}
template <class T>
std::unique_ptr<T[]> filled(size_t n, T value)
{
    std::unique_ptr<T[]> p(new T[n]);
    std::fill(p.get(), p.get() + n, value);
    return p;
}

std::vector<size_t> boundsOf(const Batch &b) { return b.offsets.empty() ? std::vector<size_t>{0, b.input.size()} : b.offsets; }

/* does pattern id occur at p inside [p, end)? */
bool occursAt(const Batch &b, int id, size_t p, size_t end)
{
    const std::string &pat = kPatterns[(size_t)id - 1];
    return p + pat.size() <= end && b.input.compare(p, pat.size(), pat) == 0;
}

/* ---- PFACX_countBatchFromHost ---- */
struct Counts {
    std::vector<std::pair<int, unsigned int>> entries;
    std::vector<size_t> first;
    unsigned long long sum = 0;
};

Counts countsByDefinition(const Batch &b, bool longest)
{
    const std::vector<size_t> off = boundsOf(b);
    Counts w;
    for (size_t s = 0; s + 1 < off.size(); s++) {
        w.first.push_back(w.entries.size());
        std::vector<unsigned int> n(kPatterns.size() + 1, 0u);
        for (size_t p = off[s]; p < off[s + 1]; p++) {
            int best = 0;
            for (int id = 1; id <= (int)kPatterns.size(); id++) {
                if (!occursAt(b, id, p, off[s + 1])) continue;
                if (!longest) n[(size_t)id]++;
                if (best == 0 || kPatterns[(size_t)id - 1].size() > kPatterns[(size_t)best - 1].size()) best = id;
            }
            if (longest && best) n[(size_t)best]++;
        }
        for (int id = 1; id <= (int)kPatterns.size(); id++)
            if (n[(size_t)id]) { w.entries.emplace_back(id, n[(size_t)id]); w.sum += n[(size_t)id]; }
    }
    w.first.push_back(w.entries.size());
    return w;
}

void runCounts(PFAC_handle_t h, const Batch &b, size_t batch)
{
    const size_t segments = boundsOf(b).size() - 1;
    for (unsigned int flags : {0u, PFACX_COUNT_LONGEST}) {
        const char *call = flags ? "countBatch/longest" : "countBatch";
        const Counts want = countsByDefinition(b, flags != 0);
        const size_t total = want.entries.size();
        for (size_t capacity = 0; capacity <= total + 1; capacity++) {
            const auto input = exactly(b.input.data(), b.input.size());
            const auto offsets = exactly(b.offsets.data(), b.offsets.size());
            const auto ids = filled<int>(capacity, -7);
            const auto counts = filled<unsigned int>(capacity, 77u);
            const auto first = filled<size_t>(segments + 1, 12345);
            size_t n = 12345;
            unsigned long long sum = 12345;
            const PFAC_status_t st = PFACX_countBatchFromHost(h, input.get(), b.input.size(), b.offsets.empty() ? nullptr : offsets.get(), segments, flags,
                                                              capacity ? ids.get() : nullptr, capacity ? counts.get() : nullptr, capacity, first.get(), &n, &sum);
            check(st == (total > capacity ? PFACX_STATUS_OUTPUT_TRUNCATED : PFAC_STATUS_SUCCESS), call, "the status", batch, capacity);
            check(n == total && sum == want.sum, call, "the length of the list or the sum", batch, capacity);
            check(std::equal(want.first.begin(), want.first.end(), first.get()), call, "segFirst", batch, capacity);
            for (size_t k = 0; k < capacity; k++)
                check(k < total ? (ids[k] == want.entries[k].first && counts[k] == want.entries[k].second) : (ids[k] == -7 && counts[k] == 77u), call,
                      "an entry", batch, capacity);
        }
    }
}

/* ---- PFACX_rulesMatchFromHost ---- */
struct RuleSet {
    const char *name;
    std::vector<int> ruleOff;
    std::vector<PFACX_rule_member_t> members;
    bool conditioned;                        /* PFACX_rulesOpenEx; else PFACX_rulesOpen over the members' patterns */
};

struct Fired {
    std::vector<std::pair<int, int>> entries;       /* (segment or piece, rule) */
    std::vector<size_t> first;
};

Fired firedByDefinition(const Batch &b, const RuleSet &rs)
{
    const std::vector<size_t> off = boundsOf(b);
    Fired w;
    for (size_t s = 0; s + 1 < off.size(); s++) {
        w.first.push_back(w.entries.size());
        const long long n = (long long)(off[s + 1] - off[s]);
        for (size_t r = 0; r + 1 < rs.ruleOff.size(); r++) {
            bool fires = true;
            for (int j = rs.ruleOff[r]; j < rs.ruleOff[r + 1]; j++) {
                const PFACX_rule_member_t &m = rs.members[(size_t)j];
                const long long len = (long long)kPatterns[(size_t)m.pattern - 1].size();
                bool some = false;
                for (size_t p = off[s]; p < off[s + 1]; p++) {
                    if (!occursAt(b, m.pattern, p, off[s + 1])) continue;
                    const long long at = (long long)(p - off[s]), a = (m.flags & PFACX_RULE_FROM_END) ? n - at - len : at;
                    if (a >= (long long)m.offset && (m.depth == 0 || a + len <= (long long)m.offset + (long long)m.depth)) some = true;
                }
                if (some == ((m.flags & PFACX_RULE_NOT) != 0)) fires = false;
            }
            if (fires) w.entries.emplace_back((int)s, (int)r);
        }
    }
    w.first.push_back(w.entries.size());
    return w;
}

void checkFired(const char *call, const Fired &want, const int *seg, const int *rule, size_t capacity, size_t batch)
{
    for (size_t k = 0; k < capacity; k++)
        check(k < want.entries.size() ? (seg[k] == want.entries[k].first && rule[k] == want.entries[k].second) : (seg[k] == -7 && rule[k] == -7), call,
              "an entry", batch, capacity);
}

void runRules(PFAC_handle_t h, const RuleSet &rs, const Batch &b, size_t batch)
{
    PFACX_rules_t rules = nullptr;
    std::vector<int> patterns;
    for (const PFACX_rule_member_t &m : rs.members) patterns.push_back(m.pattern);
    const size_t numRules = rs.ruleOff.size() - 1;
    const PFAC_status_t opened = rs.conditioned ? PFACX_rulesOpenEx(h, rs.ruleOff.data(), rs.members.data(), numRules, &rules)
                                                : PFACX_rulesOpen(h, rs.ruleOff.data(), patterns.data(), numRules, &rules);
    check(opened == PFAC_STATUS_SUCCESS, rs.name, "the open", batch, 0);
    if (opened != PFAC_STATUS_SUCCESS) return;
    const size_t segments = boundsOf(b).size() - 1;
    const Fired want = firedByDefinition(b, rs);
    const size_t total = want.entries.size();
    for (size_t capacity = 0; capacity <= total + 1; capacity++) {
        const bool withFirst = capacity % 2 == 0 || capacity == total;             /* segFirst may be null */
        const auto input = exactly(b.input.data(), b.input.size());
        const auto offsets = exactly(b.offsets.data(), b.offsets.size());
        const auto seg = filled<int>(capacity, -7), rule = filled<int>(capacity, -7);
        const auto first = filled<size_t>(segments + 1, 12345);
        size_t n = 12345;
        const PFAC_status_t st = PFACX_rulesMatchFromHost(rules, input.get(), b.input.size(), b.offsets.empty() ? nullptr : offsets.get(), segments,
                                                          capacity ? seg.get() : nullptr, capacity ? rule.get() : nullptr, capacity,
                                                          withFirst ? first.get() : nullptr, &n);
        check(st == (total > capacity ? PFACX_STATUS_OUTPUT_TRUNCATED : PFAC_STATUS_SUCCESS), rs.name, "the status", batch, capacity);
        check(n == total, rs.name, "the length of the list", batch, capacity);
        check(!withFirst || std::equal(want.first.begin(), want.first.end(), first.get()), rs.name, "segFirst", batch, capacity);
        checkFired(rs.name, want, seg.get(), rule.get(), capacity, batch);
    }
    check(PFACX_rulesClose(rules) == PFAC_STATUS_SUCCESS, rs.name, "the close", batch, 0);
}

/* ---- PFACX_flowRulesPairsFromHost ---- */
struct FlowCall {
    std::vector<int> ids;                    /* longest-match ids, whatever a caller may hand in: 0 and 6 name no pattern */
    std::vector<int> pieceFirst;
    std::vector<unsigned int> flows;
};

/* the patterns that occur with pair id: the pattern and every pattern that is a prefix of it */
void occurWith(int id, std::set<int> &now)
{
    if (id < 1 || id > (int)kPatterns.size()) return;
    for (int q = 1; q <= (int)kPatterns.size(); q++)
        if (kPatterns[(size_t)id - 1].compare(0, kPatterns[(size_t)q - 1].size(), kPatterns[(size_t)q - 1]) == 0) now.insert(q);
}

/* the fired list of one call over the flows' states, which move on (a call that fits) */
Fired flowFiredByDefinition(const FlowCall &c, const RuleSet &rs, std::vector<std::set<int>> &seen)
{
    Fired w;
    for (size_t k = 0; k < c.flows.size(); k++) {
        w.first.push_back(w.entries.size());
        std::set<int> now, &old = seen[c.flows[k]];
        for (int i = c.pieceFirst[k]; i < c.pieceFirst[k + 1]; i++) occurWith(c.ids[(size_t)i], now);
        for (size_t r = 0; r + 1 < rs.ruleOff.size(); r++) {
            bool before = true, after = true;
            for (int j = rs.ruleOff[r]; j < rs.ruleOff[r + 1]; j++) {
                const int q = rs.members[(size_t)j].pattern;
                before = before && old.count(q);
                after = after && (old.count(q) || now.count(q));
            }
            if (after && !before) w.entries.emplace_back((int)k, (int)r);
        }
        old.insert(now.begin(), now.end());
    }
    w.first.push_back(w.entries.size());
    return w;
}

void runFlowRules(PFAC_handle_t h, const RuleSet &rs, const std::vector<FlowCall> &calls, size_t schedule)
{
    const size_t numFlows = 4;
    std::vector<int> patterns;
    for (const PFACX_rule_member_t &m : rs.members) patterns.push_back(m.pattern);
    size_t longestList = 0;
    for (size_t capacity = 0; capacity <= longestList + 1; capacity++) {         /* every call of the schedule at this capacity first */
        PFACX_flowRules_t fr = nullptr;
        const PFAC_status_t opened = PFACX_flowRulesOpen(h, rs.ruleOff.data(), patterns.data(), rs.ruleOff.size() - 1, numFlows, &fr);
        check(opened == PFAC_STATUS_SUCCESS, "flowRules", "the open", schedule, capacity);
        if (opened != PFAC_STATUS_SUCCESS) return;
        std::vector<std::set<int>> seen(numFlows);
        for (const FlowCall &c : calls) {
            const Fired want = flowFiredByDefinition(c, rs, seen);
            const size_t total = want.entries.size(), pieces = c.flows.size();
            longestList = std::max(longestList, total);
            for (size_t room : {capacity, total}) {                                 /* truncated: again with room, the same list */
                const bool withFirst = room % 2 == 0 || room == total;
                const auto ids = exactly(c.ids.data(), c.ids.size());
                const auto pieceFirst = exactly(c.pieceFirst.data(), c.pieceFirst.size());
                const auto flows = exactly(c.flows.data(), c.flows.size());
                const auto piece = filled<int>(room, -7), rule = filled<int>(room, -7);
                const auto first = filled<size_t>(pieces + 1, 12345);
                size_t n = 12345;
                const PFAC_status_t st = PFACX_flowRulesPairsFromHost(fr, ids.get(), c.ids.size(), pieceFirst.get(), flows.get(), pieces,
                                                                      room ? piece.get() : nullptr, room ? rule.get() : nullptr, room,
                                                                      withFirst ? first.get() : nullptr, &n);
                check(st == (total > room ? PFACX_STATUS_OUTPUT_TRUNCATED : PFAC_STATUS_SUCCESS), "flowRules", "the status", schedule, room);
                check(n == total, "flowRules", "the length of the list", schedule, room);
                check(!withFirst || std::equal(want.first.begin(), want.first.end(), first.get()), "flowRules", "pieceFiredFirst", schedule, room);
                checkFired("flowRules", want, piece.get(), rule.get(), room, schedule);
                if (total <= room) break;                                           /* it fitted: the flows have moved on */
            }
        }
        check(PFACX_flowRulesClose(fr) == PFAC_STATUS_SUCCESS, "flowRules", "the close", schedule, capacity);
    }
}

} // namespace

int main()
{
    const std::vector<Batch> batches = {
        {"aaabab", {0, 3, 3, 6}},                /* an empty middle segment */
        {"abaa", {0, 0, 2, 4, 4}},               /* an empty first and last segment */
        {"aaaa", {}},                            /* offsets == NULL */
        {"xbxaab", {0, 1, 2, 6}},                /* a segment without a match */
        {"abab", {0, 1, 2, 4}},                  /* "ab" across a border does not count */
        {"", {0, 0, 0}},                         /* size 0 */
    };
    const unsigned int NOT = PFACX_RULE_NOT, END = PFACX_RULE_FROM_END;
    const RuleSet plain = {"rules/plain", {0, 2, 3, 5}, {{1, 0, 0, 0}, {4, 0, 0, 0}, {3, 0, 0, 0}, {5, 0, 0, 0}, {2, 0, 0, 0}}, false};
    const RuleSet conditioned = {"rules/conditioned", {0, 1, 3, 5}, {{1, 0, 0, 1}, {4, END, 0, 1}, {3, NOT, 0, 0}, {2, 0, 1, 0}, {5, NOT | END, 0, 2}}, true};
    const std::vector<std::vector<FlowCall>> schedules = {
        /* members from different calls, the same pairs twice, an empty first and last piece, ids that name no pattern */
        {{{1, 0, 6}, {0, 0, 3, 3}, {2, 0, 1}}, {{4, 3, 5, 2}, {0, 1, 2, 4}, {0, 3, 1}}, {{4, 3, 5, 2}, {0, 1, 2, 4}, {0, 3, 1}}, {{5, 4, 3}, {0, 2, 3}, {3, 2}}},
        /* no pair at all, then one piece that completes every rule */
        {{{}, {0, 0}, {1}}, {{3, 5, 4}, {0, 3}, {1}}},
    };
    for (int platform : {PFAC_PLATFORM_CPU, PFAC_PLATFORM_CPU_OMP}) {
        std::string file;
        for (const std::string &p : kPatterns) file += p + "\n";
        PFAC_handle_t h = nullptr;
        if (PFACX_createHostOnly(&h) != PFAC_STATUS_SUCCESS || PFAC_setPlatform(h, (PFAC_platform_t)platform) != PFAC_STATUS_SUCCESS ||
            PFACX_readPatternFromMemoryEx(h, file.data(), file.size(), 0u) != PFAC_STATUS_SUCCESS) {
            std::fprintf(stderr, "FAILED: the handle (platform %d)\n", platform);
            return 1;
        }
        for (size_t k = 0; k < batches.size(); k++) {
            runCounts(h, batches[k], k);
            runRules(h, plain, batches[k], k);
            runRules(h, conditioned, batches[k], k);
        }
        for (size_t k = 0; k < schedules.size(); k++) runFlowRules(h, plain, schedules[k], k);
        PFAC_destroy(h);
    }
    /* the definitions themselves, on lists written out by hand */
    const Counts c0 = countsByDefinition(batches[0], false);
    const Fired f0 = firedByDefinition(batches[0], plain);
    if (c0.entries != std::vector<std::pair<int, unsigned int>>{{1, 3}, {2, 2}, {3, 1}, {1, 1}, {4, 2}, {5, 1}} || c0.sum != 10 ||
        f0.entries != std::vector<std::pair<int, int>>{{0, 1}, {2, 0}} || f0.first != std::vector<size_t>{0, 1, 1, 2}) {
        std::fprintf(stderr, "FAILED: the definitions themselves\n");
        failures++;
    }
    if (failures) return 1;
    std::printf("segframe_host_san: %zu batches and %zu flow schedules x 2 platforms, every capacity, agree with the definitions\n", batches.size(),
                schedules.size());
    return 0;
}
