/*
 * rules_example.cpp -- alerts over a log: a rule is a name and a few strings that must ALL occur in one record ("ERROR" and "payment-service" in the
 * same line).  The records are the segments of one batch; PFACX_rulesMatch* returns the (record, rule) pairs that fired (include/pfac_ext.h).
 *
 *   rules_example                      built-in rules and log, checked against a loop over the rules
 *   rules_example RULES [LOG]          RULES: one rule per line, its name followed by TAB-separated patterns; LOG: one record per line, a file, else stdin
 *
 * The pattern set is the distinct patterns of all rules.  No pattern contains '\n', so the line starts taken as offsets give per-line rules.
 * With a GPU the device form runs; without one the host form on a host-only handle.
 */
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
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

struct Rule {
    std::string name;
    std::vector<std::string> patterns;
};

int main(int argc, char **argv)
{
    std::vector<Rule> rules = {{"payment-down", {"ERROR", "payment-service"}},
                               {"admin-probe", {"GET", "/admin"}},
                               {"any-get", {"GET"}},
                               {"admin-config", {"GET /admin", "config", "401"}}};
    std::string text = "GET /index 200\nERROR timeout in payment-service\npayment-service ok\nGET /admin/config 401\nERROR disk\nPOST /admin 403\n";
    const bool builtin = argc < 2;
    if (!builtin) {
        rules.clear();
        std::ifstream rf(argv[1], std::ios::binary);
        if (!rf) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
        for (std::string line; std::getline(rf, line);) {
            Rule r;
            size_t at = line.find('\t');
            r.name = line.substr(0, at);
            while (at != std::string::npos) {
                const size_t next = line.find('\t', at + 1);
                const std::string p = line.substr(at + 1, next == std::string::npos ? next : next - at - 1);
                if (!p.empty()) r.patterns.push_back(p);
                at = next;
            }
            if (!r.patterns.empty()) rules.push_back(r);
        }
        if (argc > 2) {
            std::ifstream tf(argv[2], std::ios::binary);
            if (!tf) { fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
            text.assign(std::istreambuf_iterator<char>(tf), std::istreambuf_iterator<char>());
        } else {
            text.assign(std::istreambuf_iterator<char>(std::cin), std::istreambuf_iterator<char>());
        }
    }
    if (rules.empty()) { fprintf(stderr, "no rules\n"); return 1; }

    /* the pattern set: every distinct pattern once, id = its line; the rules as offsets into one list of ids */
    std::map<std::string, int> idOf;
    std::string patterns;
    std::vector<int> ruleOff = {0}, rulePatterns;
    for (const Rule &r : rules) {
        for (const std::string &p : r.patterns) {
            auto it = idOf.find(p);
            if (it == idOf.end()) {
                it = idOf.emplace(p, (int)idOf.size() + 1).first;
                patterns += p + "\n";
            }
            rulePatterns.push_back(it->second);
        }
        ruleOff.push_back((int)rulePatterns.size());
    }
    /* the records: the line starts as offsets, the end of the text behind the last */
    const size_t n = text.size();
    std::vector<size_t> offsets = {0};
    for (size_t i = 0; i < n; i++)
        if (text[i] == '\n' && i + 1 < n) offsets.push_back(i + 1);
    offsets.push_back(n);
    const size_t records = offsets.size() - 1;

    int devices = 0;
    const bool gpu = hipGetDeviceCount(&devices) == hipSuccess && devices > 0;
    PFAC_handle_t handle = nullptr;
    if (gpu) CHECK(PFAC_create(&handle));
    else CHECK(PFACX_createHostOnly(&handle));
    CHECK(PFACX_readPatternFromMemory(handle, patterns.data(), patterns.size()));
    PFACX_rules_t set = nullptr;
    CHECK(PFACX_rulesOpen(handle, ruleOff.data(), rulePatterns.data(), rules.size(), &set));

    size_t fired = 0;
    std::vector<int> seg, rule;
    if (n == 0) {
        /* nothing to match */
    } else if (gpu) {
        char *d_text = nullptr;
        size_t *d_offsets = nullptr;
        int *d_seg = nullptr, *d_rule = nullptr;
        HIP(hipMalloc(reinterpret_cast<void **>(&d_text), n));
        HIP(hipMalloc(reinterpret_cast<void **>(&d_offsets), offsets.size() * sizeof(size_t)));
        HIP(hipMemcpy(d_text, text.data(), n, hipMemcpyHostToDevice));
        HIP(hipMemcpy(d_offsets, offsets.data(), offsets.size() * sizeof(size_t), hipMemcpyHostToDevice));
        /* the count query, then the list */
        const PFAC_status_t q = PFACX_rulesMatchFromDevice(set, d_text, n, d_offsets, records, nullptr, nullptr, 0, nullptr, &fired);
        if (q != PFAC_STATUS_SUCCESS && q != PFACX_STATUS_OUTPUT_TRUNCATED) { fprintf(stderr, "count query: %s\n", PFAC_getErrorString(q)); return 1; }
        seg.resize(fired);
        rule.resize(fired);
        if (fired) {
            HIP(hipMalloc(reinterpret_cast<void **>(&d_seg), fired * sizeof(int)));
            HIP(hipMalloc(reinterpret_cast<void **>(&d_rule), fired * sizeof(int)));
            CHECK(PFACX_rulesMatchFromDevice(set, d_text, n, d_offsets, records, d_seg, d_rule, fired, nullptr, &fired));
            HIP(hipMemcpy(seg.data(), d_seg, fired * sizeof(int), hipMemcpyDeviceToHost));
            HIP(hipMemcpy(rule.data(), d_rule, fired * sizeof(int), hipMemcpyDeviceToHost));
        }
        for (void *p : {(void *)d_text, (void *)d_offsets, (void *)d_seg, (void *)d_rule}) (void)hipFree(p);
    } else {
        std::string copy = text;                                           /* (the call takes a char *; it does not write) */
        const PFAC_status_t q = PFACX_rulesMatchFromHost(set, &copy[0], n, offsets.data(), records, nullptr, nullptr, 0, nullptr, &fired);
        if (q != PFAC_STATUS_SUCCESS && q != PFACX_STATUS_OUTPUT_TRUNCATED) { fprintf(stderr, "count query: %s\n", PFAC_getErrorString(q)); return 1; }
        seg.resize(fired);
        rule.resize(fired);
        if (fired) CHECK(PFACX_rulesMatchFromHost(set, &copy[0], n, offsets.data(), records, seg.data(), rule.data(), fired, nullptr, &fired));
    }
    CHECK(PFACX_rulesClose(set));
    CHECK(PFAC_destroy(handle));

    for (size_t i = 0; i < fired; i++) printf("record %d: rule %s\n", seg[i], rules[(size_t)rule[i]].name.c_str());
    if (!builtin) return 0;
    printf("%zu records, %zu rules, %zu fired (%s form)\n", records, rules.size(), fired, gpu ? "device" : "host");

    /* self-check: every rule over every record, by hand */
    std::vector<int> wantSeg, wantRule;
    for (size_t k = 0; k < records; k++) {
        const std::string record = text.substr(offsets[k], offsets[k + 1] - offsets[k]);
        for (size_t r = 0; r < rules.size(); r++) {
            bool all = true;
            for (const std::string &p : rules[r].patterns) all = all && record.find(p) != std::string::npos;
            if (all) { wantSeg.push_back((int)k); wantRule.push_back((int)r); }
        }
    }
    if (seg != wantSeg || rule != wantRule) {
        fprintf(stderr, "self-check FAILED: want %zu fired\n", wantSeg.size());
        return 1;
    }
    printf("self-check passed\n");
    return 0;
}
