/*
 * ruleseq_example.cpp -- alerts over a log whose rules say in which ORDER and how CLOSE strings must stand: "`timeout` within 40 bytes after
 * `payment-service`", "`User-Agent:` and then `sqlmap` in the same line"; Snort's content:"A"; content:"B"; distance:d; within:w;.  A rule is a list
 * of PFACX_rule_seq_member_t -- PFACX_rule_member_t plus distance and within; a member with PFACX_RULE_RELATIVE is tied to the member in front of
 * it -- opened by PFACX_rulesOpenSeq; everything behind the open is the ordinary rules call (include/pfac_ext.h; rulecond_example.cpp has the
 * members without an order).
 *
 *   ruleseq_example                    built-in rules and records, checked against a search over all assignments
 *
 * The records are the lines of the text.  With a GPU the device form runs; without one the host form on a host-only handle.
 */
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "pfac_ext.h"

#define CHECK(call)                                                                            \
    do {                                                                                       \
        const PFAC_status_t st_ = (call);                                                      \
        if (st_ != PFAC_STATUS_SUCCESS) {                                                      \
            fprintf(stderr, "%s: %s\n", #call, PFAC_getErrorString(st_));                      \
            return 1;                                                                          \
        }                                                                                      \
    } while (0)
#define HIP(call)                                                                              \
    do {                                                                                       \
        const hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess) {                                                                \
            fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));                         \
            return 1;                                                                          \
        }                                                                                      \
    } while (0)

struct Member {
    std::string pattern;
    unsigned int flags, offset, depth, distance, within;
};
struct Rule {
    std::string name;
    std::vector<Member> members;
};
constexpr unsigned int REL = PFACX_RULE_RELATIVE;

/* the own window of a member, by hand */
static bool inWindow(const Member &m, size_t s, const std::string &record)
{
    const unsigned long long n = record.size(), len = m.pattern.size();
    const unsigned long long a = (m.flags & PFACX_RULE_FROM_END) ? n - s - len : s;
    return a >= m.offset && (m.depth == 0 || a + len <= (unsigned long long)m.offset + m.depth);
}

/* can members j .. of the chain that ends in front of `last` be placed behind a predecessor that ends at e?  Every assignment is tried */
static bool place(const std::vector<Member> &ms, size_t j, size_t last, unsigned long long e, const std::string &record)
{
    if (j == last) return true;
    const Member &m = ms[j];
    for (size_t s = record.find(m.pattern); s != std::string::npos; s = record.find(m.pattern, s + 1))
        if (inWindow(m, s, record) && s >= e + m.distance && (m.within == 0 || s + m.pattern.size() <= e + m.within) &&
            place(ms, j + 1, last, s + m.pattern.size(), record))
            return true;
    return false;
}

/* the contract, by hand: every chain holds, every member outside a chain holds */
static bool fires(const Rule &r, const std::string &record)
{
    const std::vector<Member> &ms = r.members;
    for (size_t j = 0; j < ms.size();) {
        size_t last = j + 1;
        while (last < ms.size() && (ms[last].flags & REL)) last++;
        bool some = false;
        for (size_t s = record.find(ms[j].pattern); s != std::string::npos && !some; s = record.find(ms[j].pattern, s + 1))
            some = inWindow(ms[j], s, record) && place(ms, j + 1, last, s + ms[j].pattern.size(), record);
        if (some == ((ms[j].flags & PFACX_RULE_NOT) != 0)) return false;
        j = last;
    }
    return true;
}

int main()
{
    const std::vector<Rule> rules = {
        {"payment-timeout", {{"payment-service", 0, 0, 0, 0, 0}, {"timeout", REL, 0, 0, 0, 40}}},              /* timeout ends within 40 bytes behind payment-service */
        {"sqlmap-agent", {{"User-Agent:", 0, 0, 0, 0, 0}, {"sqlmap", REL, 0, 0, 1, 0}, {"Host: intranet", PFACX_RULE_NOT, 0, 0, 0, 0}}},
        {"get-admin-401", {{"GET", 0, 0, 3, 0, 0}, {"/admin", REL, 0, 0, 1, 7}, {"401", REL | PFACX_RULE_FROM_END, 0, 3, 0, 0}}},
        {"retry-twice", {{"retry", 0, 0, 0, 0, 0}, {"retry", REL, 0, 0, 0, 0}}}};                              /* the same pattern twice: two occurrences that do not overlap */
    const std::string text =
        "payment-service: upstream timeout\ntimeout, then payment-service came back\npayment-service was fine for a very long while, and then a timeout\n"
        "GET / User-Agent: sqlmap/1.7\nsqlmap is no User-Agent: curl\nGET / User-Agent: sqlmap Host: intranet\nGET /admin 401\nGET /x/admin 401\n"
        "GET /admin 401 more\nretry\nretry, retry\n";

    std::map<std::string, int> idOf;
    std::string patterns;
    std::vector<int> ruleOff = {0};
    std::vector<PFACX_rule_seq_member_t> members;
    for (const Rule &r : rules) {
        for (const Member &m : r.members) {
            auto it = idOf.find(m.pattern);
            if (it == idOf.end()) {
                it = idOf.emplace(m.pattern, (int)idOf.size() + 1).first;
                patterns += m.pattern + "\n";
            }
            members.push_back(PFACX_rule_seq_member_t{it->second, m.flags, m.offset, m.depth, m.distance, m.within});
        }
        ruleOff.push_back((int)members.size());
    }
    std::string body;
    std::vector<size_t> offsets = {0};
    for (const char ch : text) {
        if (ch == '\n') offsets.push_back(body.size());
        else body += ch;
    }
    const size_t n = body.size(), records = offsets.size() - 1;

    int devices = 0;
    const bool gpu = hipGetDeviceCount(&devices) == hipSuccess && devices > 0;
    PFAC_handle_t handle = nullptr;
    if (gpu) CHECK(PFAC_create(&handle));
    else CHECK(PFACX_createHostOnly(&handle));
    CHECK(PFACX_readPatternFromMemory(handle, patterns.data(), patterns.size()));
    PFACX_rules_t set = nullptr;
    CHECK(PFACX_rulesOpenSeq(handle, ruleOff.data(), members.data(), rules.size(), &set));

    size_t fired = 0;
    const size_t capacity = records * rules.size();                        /* small enough here to skip the count query */
    std::vector<int> seg(capacity), rule(capacity);
    if (gpu) {
        char *d_text = nullptr;
        size_t *d_offsets = nullptr;
        int *d_seg = nullptr, *d_rule = nullptr;
        HIP(hipMalloc(reinterpret_cast<void **>(&d_text), n));
        HIP(hipMalloc(reinterpret_cast<void **>(&d_offsets), offsets.size() * sizeof(size_t)));
        HIP(hipMalloc(reinterpret_cast<void **>(&d_seg), capacity * sizeof(int)));
        HIP(hipMalloc(reinterpret_cast<void **>(&d_rule), capacity * sizeof(int)));
        HIP(hipMemcpy(d_text, body.data(), n, hipMemcpyHostToDevice));
        HIP(hipMemcpy(d_offsets, offsets.data(), offsets.size() * sizeof(size_t), hipMemcpyHostToDevice));
        CHECK(PFACX_rulesMatchFromDevice(set, d_text, n, d_offsets, records, d_seg, d_rule, capacity, nullptr, &fired));
        HIP(hipMemcpy(seg.data(), d_seg, fired * sizeof(int), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(rule.data(), d_rule, fired * sizeof(int), hipMemcpyDeviceToHost));
        for (void *p : {(void *)d_text, (void *)d_offsets, (void *)d_seg, (void *)d_rule}) (void)hipFree(p);
    } else {
        std::string copy = body;                                           /* (the call takes a char *; it does not write) */
        CHECK(PFACX_rulesMatchFromHost(set, &copy[0], n, offsets.data(), records, seg.data(), rule.data(), capacity, nullptr, &fired));
    }
    seg.resize(fired);
    rule.resize(fired);
    CHECK(PFACX_rulesClose(set));
    CHECK(PFAC_destroy(handle));

    for (size_t i = 0; i < fired; i++) printf("record %d: rule %s\n", seg[i], rules[(size_t)rule[i]].name.c_str());
    printf("%zu records, %zu rules, %zu fired (%s form)\n", records, rules.size(), fired, gpu ? "device" : "host");

    std::vector<int> wantSeg, wantRule;
    for (size_t k = 0; k < records; k++) {
        const std::string record = body.substr(offsets[k], offsets[k + 1] - offsets[k]);
        for (size_t r = 0; r < rules.size(); r++)
            if (fires(rules[r], record)) { wantSeg.push_back((int)k); wantRule.push_back((int)r); }
    }
    if (seg != wantSeg || rule != wantRule || fired == 0) {
        fprintf(stderr, "self-check FAILED: want %zu fired\n", wantSeg.size());
        return 1;
    }
    printf("self-check passed\n");
    return 0;
}
