/*
 * rulecond_example.cpp -- alerts over a log whose rules say WHERE a string must stand and which strings must NOT occur: "starts with ERROR, contains
 * payment, does not contain retry"; Snort's content:"GET"; depth:3; content:"/admin"; content:!"Host: intranet".  A rule is a list of
 * PFACX_rule_member_t -- a pattern id, PFACX_RULE_NOT / PFACX_RULE_FROM_END, offset and depth -- opened by PFACX_rulesOpenEx; everything behind the
 * open is the ordinary rules call (include/pfac_ext.h; rules_example.cpp has the plain form with rule files).
 *
 *   rulecond_example                   built-in rules and records, checked against a loop over the rules
 *
 * The records are the lines of the text: a window is measured from a record's first (or last) byte.  With a GPU the device form runs; without one
 * the host form on a host-only handle.
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
    unsigned int flags, offset, depth;
};
struct Rule {
    std::string name;
    std::vector<Member> members;
};

/* the contract's test, by hand: does `record` make the member hold? */
static bool holds(const Member &m, const std::string &record)
{
    const unsigned long long n = record.size(), len = m.pattern.size();
    bool some = false;
    for (size_t s = record.find(m.pattern); s != std::string::npos && !some; s = record.find(m.pattern, s + 1)) {
        const unsigned long long a = (m.flags & PFACX_RULE_FROM_END) ? n - s - len : s;
        some = a >= m.offset && (m.depth == 0 || a + len <= (unsigned long long)m.offset + m.depth);
    }
    return some != ((m.flags & PFACX_RULE_NOT) != 0);
}

int main()
{
    const std::vector<Rule> rules = {
        {"payment-error", {{"ERROR", 0, 0, 5}, {"payment", 0, 0, 0}, {"retry", PFACX_RULE_NOT, 0, 0}}},       /* starts with, contains, does not contain */
        {"admin-from-outside", {{"GET", 0, 0, 3}, {"/admin", 0, 4, 0}, {"Host: intranet", PFACX_RULE_NOT, 0, 0}}},
        {"ends-in-401", {{"401", PFACX_RULE_FROM_END, 0, 3}}},                                                   /* endswith */
        {"get-not-first", {{"GET", 0, 1, 0}, {"GET", PFACX_RULE_NOT, 0, 3}}}};                                  /* the same pattern, two windows */
    const std::string text =
        "ERROR payment timeout\nERROR payment timeout, retry 2\nwarn: ERROR payment\nGET /admin/config 401\nGET /admin Host: intranet\n"
        "POST /x then GET /admin 401 later\nGET /index 401\n";

    /* the pattern set: every distinct pattern once, id = its line; the rules as offsets into one list of members */
    std::map<std::string, int> idOf;
    std::string patterns;
    std::vector<int> ruleOff = {0};
    std::vector<PFACX_rule_member_t> members;
    for (const Rule &r : rules) {
        for (const Member &m : r.members) {
            auto it = idOf.find(m.pattern);
            if (it == idOf.end()) {
                it = idOf.emplace(m.pattern, (int)idOf.size() + 1).first;
                patterns += m.pattern + "\n";
            }
            members.push_back(PFACX_rule_member_t{it->second, m.flags, m.offset, m.depth});
        }
        ruleOff.push_back((int)members.size());
    }
    /* the records: the lines without their newlines, back to back, and where each starts -- so a window from the end is measured from a record's
     * last character, not from a newline behind it */
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
    CHECK(PFACX_rulesOpenEx(handle, ruleOff.data(), members.data(), rules.size(), &set));

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

    /* self-check: every member of every rule over every record, by hand */
    std::vector<int> wantSeg, wantRule;
    for (size_t k = 0; k < records; k++) {
        const std::string record = body.substr(offsets[k], offsets[k + 1] - offsets[k]);
        for (size_t r = 0; r < rules.size(); r++) {
            bool all = true;
            for (const Member &m : rules[r].members) all = all && holds(m, record);
            if (all) { wantSeg.push_back((int)k); wantRule.push_back((int)r); }
        }
    }
    if (seg != wantSeg || rule != wantRule || fired == 0) {
        fprintf(stderr, "self-check FAILED: want %zu fired\n", wantSeg.size());
        return 1;
    }
    printf("self-check passed\n");
    return 0;
}
