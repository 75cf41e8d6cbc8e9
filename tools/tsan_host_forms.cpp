/* tools/tsan_host_forms.cpp -- the host forms that scan and then read the compiled set (PFACX_matchAllFromHost, countFromHost, matchWordsFromHost in
 * both modes, matchSpansFromHost, matchDisjointFromHost, matchLinesFromHost), PFACX_replaceFromHost and the batch host forms over the input cut at
 * its newlines (PFACX_countBatchFromHost, rulesMatchFromHost, groupsMatchFromHost), and a stream and a flow set opened, fed from the host in two
 * pieces, flushed and closed within one call, under ThreadSanitizer (`make -C pfac_amd/csrc tsan`): four
 * threads call them on one host-only handle while a fifth replaces its pattern set, cycling through three sets.  A and B have the same number of
 * patterns -- A with chains of prefixes, B with none, and other lengths per id --, C has more.  Every call must end in the documented refusal
 * (PATTERNS_NOT_READY; INVALID_PARAMETER for a rule set, a group table, a stream or a flow set opened on a set that has been replaced: the thread opens a new one) or in
 * success with the single-threaded answer of one of the sets, a mixture of two sets never; and every form must have given every set's answer at
 * least once, so that a library that refuses everything does not pass.  CPU only.   tsan_host_forms [rounds] [pause in microseconds] */
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "PFAC.h"
#include "pfac_ext.h"

namespace {

enum Form { kAll, kCount, kWordsList, kWordsAll, kSpans, kDisjoint, kLines, kReplace, kCountBatch, kRules, kGroups, kStream, kFlows, kForms };
const char *const kFormName[kForms] = {"matchAll", "count", "words", "words(all)", "spans", "disjoint", "lines", "replace", "countBatch", "rules", "groups", "stream", "flows"};

const std::string kSets[3] = {
    "a\nab\nabc\nabcd\nhe\nhers\n",                          /* A: chains a < ab < abc < abcd, he < hers */
    "she\nhi\nbcda\nx\ndog\ncats\n",                         /* B: as many patterns, none a prefix of another, other lengths per id */
    "abc\nab\nshe\nhe\nhers\ndog\ndo\ncat\nhis\n",           /* C: more patterns */
};
constexpr size_t kNumA = 6, kNumC = 9, kCanaries = 4, kBatchSegments = 16;
constexpr unsigned long long kCanary = 0xC0FFEE0DDF00Dull;

struct Fixture {
    PFAC_handle_t h = nullptr;
    std::string input;
    std::vector<int> tokIds, tokPos;                         /* the disjoint tokens of set A: what PFACX_replaceFromHost is given, whatever set is loaded */
    std::vector<int> replOff;                                /* two offsets for every id of the largest set */
    std::string replBytes;
    std::vector<size_t> offsets;                             /* the batch forms: the first kBatchSegments lines, a segment each (a call short enough to end between two swaps) */
    std::vector<unsigned long long> segMasks;
    size_t pieces[3] = {0, 0, 0};                            /* the stream and the flows forms: the same lines in two pieces, cut inside an occurrence */
};

/* the rule set and the group table of the batch forms; every id is one that all three sets have.  Rules: pattern 1; 2 and 5; 3 within the first 8
 * bytes of the segment and no 6 */
const int kRuleOff[4] = {0, 1, 3, 5};
const PFACX_rule_member_t kRuleMembers[5] = {{1, 0u, 0u, 0u}, {2, 0u, 0u, 0u}, {5, 0u, 0u, 0u}, {3, 0u, 0u, 8u}, {6, PFACX_RULE_NOT, 0u, 0u}};
const unsigned long long kPatternMasks[10] = {0, 1, 2, 4, 8, 16, 32, 1, 2, 4};

struct Scratch {
    std::vector<int> a, b, c;
    std::vector<unsigned long long> counts;                  /* exactly kNumA + 1 entries, then the canaries */
    std::string out;
    std::vector<size_t> first;                               /* segFirst of the batch forms */
    std::vector<unsigned long long> groups;                  /* segGroups */
    PFACX_rules_t rules = nullptr;                           /* this thread's, opened on the set that was loaded then; null: none */
    PFACX_groups_t table = nullptr;
    Scratch(size_t n, size_t segments) : a(4 * n), b(4 * n), c(n), counts(kNumA + 1 + kCanaries, kCanary), out(8 * n, '\0'), first(segments + 1), groups(segments) {}
    void closeTables()
    {
        if (rules) (void)PFACX_rulesClose(rules);
        if (table) (void)PFACX_groupsClose(table);
        rules = nullptr;
        table = nullptr;
    }
};

/* The stream and the flows form open their object, feed x.pieces from the host, flush and close, all inside the one call: the open and the close
 * race with the thread that replaces the set as well.  The pairs of every step go to w.a / w.b one behind the other, *listed = their number; a close
 * that does not succeed is no documented outcome.  The stream: two piece calls and the flush, positions made relative to the stream's start */
PFAC_status_t streamForm(const Fixture &x, Scratch &w, size_t *listed)
{
    PFACX_stream_t s = nullptr;
    PFAC_status_t st = PFACX_streamOpen(x.h, &s);
    if (st != PFAC_STATUS_SUCCESS) return st;
    size_t at = 0;
    for (int k = 0; k < 3 && st == PFAC_STATUS_SUCCESS; k++) {
        int n = 0;
        unsigned long long base = x.pieces[2];               /* the flush: relative to the stream's end */
        if (k < 2)
            st = PFACX_streamMatchFromHost(s, const_cast<char *>(x.input.data()) + x.pieces[k], x.pieces[k + 1] - x.pieces[k], w.a.data() + at, w.b.data() + at,
                                           w.a.size() - at, &n, &base);
        else
            st = PFACX_streamFlush(s, w.a.data() + at, w.b.data() + at, w.a.size() - at, &n);
        if (st != PFAC_STATUS_SUCCESS) break;
        for (int i = 0; i < n; i++) w.b[at + (size_t)i] += (int)base;
        at += (size_t)n;
    }
    if (PFACX_streamClose(s) != PFAC_STATUS_SUCCESS) return PFAC_STATUS_INTERNAL_ERROR;
    *listed = at;
    return st;
}

/* ... a set of two flows: one call with a piece for each, then the flush of both; *r = pieceFirst of the call, then `first` of the flush */
PFAC_status_t flowsForm(const Fixture &x, Scratch &w, size_t *listed, std::vector<long long> *r)
{
    PFACX_flows_t fl = nullptr;
    PFAC_status_t st = PFACX_flowsOpen(x.h, 2, &fl);
    if (st != PFAC_STATUS_SUCCESS) return st;
    const unsigned int flowIds[2] = {0, 1};
    int first[6] = {0, 0, 0, 0, 0, 0}, n = 0, m = 0;
    unsigned long long pieceOffsets[2] = {0, 0};
    st = PFACX_flowsMatchFromHost(fl, const_cast<char *>(x.input.data()), x.pieces[2], x.pieces, flowIds, 2, w.a.data(), w.b.data(), w.a.size(), first, pieceOffsets, &n);
    if (st == PFAC_STATUS_SUCCESS) st = PFACX_flowsFlush(fl, flowIds, 2, w.a.data() + n, w.b.data() + n, w.a.size() - (size_t)n, first + 3, &m);
    if (PFACX_flowsClose(fl) != PFAC_STATUS_SUCCESS) return PFAC_STATUS_INTERNAL_ERROR;
    if (st == PFAC_STATUS_SUCCESS) r->assign(first, first + 6);
    *listed = (size_t)n + (size_t)m;
    return st;
}

/* one call of form f: its status, and on success everything it wrote as one list of numbers.  false: a canary behind counts[] has changed */
bool call(Form f, const Fixture &x, Scratch &w, PFAC_status_t *status, std::vector<long long> *result)
{
    char *in = const_cast<char *>(x.input.data());
    const size_t n = x.input.size();
    size_t u = 0, v = 0, listed = 0;
    std::vector<long long> &r = *result;
    r.clear();
    PFAC_status_t st = PFAC_STATUS_INTERNAL_ERROR;
    switch (f) {
    case kAll: st = PFACX_matchAllFromHost(x.h, in, n, w.a.data(), w.b.data(), w.a.size(), &u); listed = u; break;
    case kCount:
        st = PFACX_countFromHost(x.h, in, n, 0, w.counts.data(), kNumA + 1, &u);
        for (size_t k = 0; k < kCanaries; k++)
            if (w.counts[kNumA + 1 + k] != kCanary) return false;
        if (st == PFAC_STATUS_SUCCESS) r.assign(w.counts.begin(), w.counts.begin() + kNumA + 1);
        break;
    case kWordsList: st = PFACX_matchWordsFromHost(x.h, in, n, nullptr, 0, w.a.data(), w.b.data(), w.a.size(), &u); listed = u; break;
    case kWordsAll: st = PFACX_matchWordsFromHost(x.h, in, n, nullptr, PFACX_WORDS_ALL, w.a.data(), w.b.data(), w.a.size(), &u); listed = u; break;
    case kSpans: st = PFACX_matchSpansFromHost(x.h, in, n, w.a.data(), w.b.data(), w.a.size(), &u, &v); listed = u; break;
    case kDisjoint: st = PFACX_matchDisjointFromHost(x.h, in, n, w.a.data(), w.b.data(), w.a.size(), &u, &v); listed = u; break;
    case kLines:
        st = PFACX_matchLinesFromHost(x.h, in, n, 0, w.a.data(), w.b.data(), w.c.data(), w.c.size(), &v, &u);
        listed = u;
        if (st == PFAC_STATUS_SUCCESS) r.assign(w.c.begin(), w.c.begin() + u);
        break;
    case kReplace:
        st = PFACX_replaceFromHost(x.h, in, n, x.tokIds.data(), x.tokPos.data(), x.tokIds.size(), x.replOff.data(), x.replOff.size(), x.replBytes.data(),
                                   x.replBytes.size(), &w.out[0], w.out.size(), &u);
        if (st == PFAC_STATUS_SUCCESS) r.assign(w.out.begin(), w.out.begin() + u);
        break;
    case kCountBatch: {
        unsigned long long total = 0;
        st = PFACX_countBatchFromHost(x.h, in, x.offsets.back(), x.offsets.data(), x.offsets.size() - 1, 0, w.a.data(), reinterpret_cast<unsigned int *>(w.b.data()),
                                      w.a.size(), w.first.data(), &u, &total);
        v = (size_t)total;
        listed = u;
        if (st == PFAC_STATUS_SUCCESS) r.assign(w.first.begin(), w.first.end());
        break;
    }
    case kRules:
        st = w.rules ? PFAC_STATUS_SUCCESS : PFACX_rulesOpenEx(x.h, kRuleOff, kRuleMembers, 3, &w.rules);
        if (st == PFAC_STATUS_SUCCESS)
            st = PFACX_rulesMatchFromHost(w.rules, in, x.offsets.back(), x.offsets.data(), x.offsets.size() - 1, w.a.data(), w.b.data(), w.a.size(), w.first.data(), &u);
        listed = u;
        if (st == PFAC_STATUS_SUCCESS) r.assign(w.first.begin(), w.first.end());
        break;
    case kGroups:
        st = w.table ? PFAC_STATUS_SUCCESS : PFACX_groupsOpen(x.h, kPatternMasks, kNumC + 1, &w.table);
        if (st == PFAC_STATUS_SUCCESS)
            st = PFACX_groupsMatchFromHost(w.table, in, x.offsets.back(), x.offsets.data(), x.offsets.size() - 1, x.segMasks.data(), PFACX_GROUPS_ALL, w.a.data(), w.b.data(),
                                           w.a.size(), w.first.data(), w.groups.data(), &u);
        listed = u;
        if (st == PFAC_STATUS_SUCCESS) {
            r.assign(w.first.begin(), w.first.end());
            r.insert(r.end(), w.groups.begin(), w.groups.end());
        }
        break;
    case kStream: st = streamForm(x, w, &listed); u = listed; break;
    case kFlows: st = flowsForm(x, w, &listed, &r); u = listed; break;
    default: break;
    }
    *status = st;
    if (st == PFAC_STATUS_INVALID_PARAMETER && (f == kRules || f == kGroups)) w.closeTables();      /* opened on a set that is gone: a new one next time */
    if (st != PFAC_STATUS_SUCCESS) { r.clear(); return true; }
    r.push_back((long long)u);
    r.push_back((long long)v);
    r.insert(r.end(), w.a.begin(), w.a.begin() + listed);
    r.insert(r.end(), w.b.begin(), w.b.begin() + listed);
    return true;
}

bool load(PFAC_handle_t h, int set) { return PFACX_readPatternFromMemory(h, kSets[set].data(), kSets[set].size()) == PFAC_STATUS_SUCCESS; }

} // namespace

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 500, pauseUs = argc > 2 ? atoi(argv[2]) : 2000, threads = 4;
    Fixture x;
    if (PFACX_createHostOnly(&x.h) != PFAC_STATUS_SUCCESS || PFAC_setPlatform(x.h, PFAC_PLATFORM_CPU) != PFAC_STATUS_SUCCESS) return 2;
    /* lines in which all three sets occur, and one line each that only A, only B, only C selects */
    const char *const lines[] = {"abcd she sells hers, his dog and cats", "x marks hi; abc ab a_b (he) hers_", "one penny a piece", "do cat abcda bcda shells", "",
                                 "x: 1 + 2 = 3", "the dogs do chase cats: abcdabcd he she his", "do it once more"};
    for (size_t k = 0; x.input.size() < 4096; k++) {
        x.input += lines[k % 8];
        x.input += '\n';
    }
    x.offsets.push_back(0);
    for (size_t i = 0; i < x.input.size() && x.offsets.size() <= kBatchSegments; i++)
        if (x.input[i] == '\n') x.offsets.push_back(i + 1);
    for (size_t k = 0; k + 1 < x.offsets.size(); k++) x.segMasks.push_back((k * 11 + 1) & 63);
    x.pieces[1] = x.offsets[8] + 2;                          /* inside the abcd that line 8 begins with: ab | cd */
    x.pieces[2] = x.offsets.back();
    for (size_t id = 0; id <= kNumC + 1; id++) {             /* the string of id: <id>; ids 0 and F + 1 have offsets and no string of their own */
        x.replOff.push_back((int)x.replBytes.size());
        if (id >= 1 && id <= kNumC) x.replBytes += "<" + std::to_string(id) + ">";
    }
    /* the single-threaded answers: want[form][set]; count on set C is the refusal of its numCounts check */
    std::vector<long long> want[kForms][3];
    PFAC_status_t wantStatus[kForms][3];
    Scratch w0(x.input.size(), x.offsets.size() - 1);
    for (int set = 0; set < 3; set++) {
        if (!load(x.h, set)) { fprintf(stderr, "set %d refused\n", set); return 2; }
        w0.closeTables();                                    /* a rule set and a group table of this set */
        for (int f = 0; f < kForms; f++) {
            if (f == kReplace && set == 0) {                 /* its tokens: the disjoint list of A, recorded above as {count, covered, ids, positions} */
                const std::vector<long long> &d = want[kDisjoint][0];
                x.tokIds.assign(d.begin() + 2, d.begin() + 2 + d[0]);
                x.tokPos.assign(d.begin() + 2 + d[0], d.end());
            }
            if (!call((Form)f, x, w0, &wantStatus[f][set], &want[f][set])) return 2;
            const PFAC_status_t expected = f == kCount && set == 2 ? PFAC_STATUS_INVALID_PARAMETER : PFAC_STATUS_SUCCESS;
            if (wantStatus[f][set] != expected || (expected == PFAC_STATUS_SUCCESS && want[f][set].size() <= 2)) {
                fprintf(stderr, "%s on set %d alone: status %d, %zu numbers\n", kFormName[f], set, (int)wantStatus[f][set], want[f][set].size());
                return 2;
            }
        }
    }
    w0.closeTables();
    for (int f = 0; f < kForms; f++)                         /* an answer that two sets share would hide a mixture */
        if (want[f][0] == want[f][1] || want[f][0] == want[f][2] || want[f][1] == want[f][2]) { fprintf(stderr, "%s: two sets, one answer\n", kFormName[f]); return 2; }

    std::atomic<bool> done{false};
    std::atomic<long> seen[kForms][3], refused[kForms], wrong{0};
    for (int f = 0; f < kForms; f++) {
        refused[f] = 0;
        for (int set = 0; set < 3; set++) seen[f][set] = 0;
    }
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
        pool.emplace_back([&, t]() {
            Scratch w(x.input.size(), x.offsets.size() - 1);
            std::vector<long long> got;
            for (long i = t; !done.load(); i++) {
                const Form f = (Form)(i % kForms);
                PFAC_status_t st;
                if (!call(f, x, w, &st, &got)) { wrong++; fprintf(stderr, "%s: canary overwritten\n", kFormName[f]); continue; }
                if (st == PFAC_STATUS_PATTERNS_NOT_READY) { refused[f]++; continue; }
                if (st == PFAC_STATUS_INVALID_PARAMETER && (f == kRules || f == kGroups || f == kStream || f == kFlows)) { refused[f]++; continue; }
                int set = -1;
                if (st == PFAC_STATUS_INVALID_PARAMETER && f == kCount) set = 2;
                for (int k = 0; k < 3 && st == PFAC_STATUS_SUCCESS; k++)
                    if (wantStatus[f][k] == PFAC_STATUS_SUCCESS && got == want[f][k]) set = k;
                if (set < 0) { wrong++; fprintf(stderr, "%s: status %d, an answer of no set (%zu numbers)\n", kFormName[f], (int)st, got.size()); }
                else seen[f][set]++;
            }
            w.closeTables();
        });
    int failedLoads = 0;
    for (int r = 0; r < rounds; r++) {
        if (!load(x.h, (r + 1) % 3)) failedLoads++;
        std::this_thread::sleep_for(std::chrono::microseconds(pauseUs));
    }
    done = true;
    for (auto &th : pool) th.join();
    (void)PFAC_destroy(x.h);
    int unseen = 0;
    for (int f = 0; f < kForms; f++) {
        printf("%-11s A %6ld  B %6ld  C %6ld  refused %6ld\n", kFormName[f], seen[f][0].load(), seen[f][1].load(), seen[f][2].load(), refused[f].load());
        for (int set = 0; set < 3; set++) unseen += seen[f][set] == 0 ? 1 : 0;
    }
    printf("tsan_host_forms: %d threads, %d swaps: %ld wrong outcomes, %d failed loads, %d (form, set) answers never seen\n", threads, rounds, wrong.load(),
           failedLoads, unseen);
    return wrong.load() || failedLoads || unseen ? 1 : 0;
}
