/*
 * count_example.cpp -- hit counts per rule on the GPU: load a few rules, count every occurrence of every rule in a log
 * (PFACX_countFromDevice), list the rules that fired with their hits (PFACX_countNonzeroFromDevice), and check both against what a loop over
 * the rules says (include/pfac_ext.h).
 */
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
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

int main()
{
    /* "GET /admin" holds "GET", "/admin/config" holds "/admin": the longest match hides them, the counts do not */
    const std::vector<std::string> rules = {"GET", "GET /admin", "/admin", "/admin/config", "POST", "passwd", "never seen"};
    const std::string text = "GET /index GET /admin/config POST /login passwd GET /admin POST /admin/config passwd passwd";
    std::string patterns;
    for (const std::string &r : rules) patterns += r + "\n";
    const size_t n = text.size(), numCounts = rules.size() + 1;            /* counts are indexed by pattern id: 1 .. F */

    PFAC_handle_t handle = nullptr;
    CHECK(PFAC_create(&handle));
    CHECK(PFACX_readPatternFromMemory(handle, patterns.data(), patterns.size()));

    char *d_text = nullptr;
    unsigned long long *d_counts = nullptr, *d_hits = nullptr;
    int *d_ids = nullptr;
    HIP(hipMalloc(reinterpret_cast<void **>(&d_text), n));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_counts), numCounts * sizeof(unsigned long long)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_hits), numCounts * sizeof(unsigned long long)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_ids), numCounts * sizeof(int)));
    HIP(hipMemcpy(d_text, text.data(), n, hipMemcpyHostToDevice));

    size_t occurrences = 0, fired = 0;
    unsigned long long sum = 0;
    CHECK(PFACX_countFromDevice(handle, d_text, n, 0, d_counts, numCounts, &occurrences));
    CHECK(PFACX_countNonzeroFromDevice(handle, d_counts, numCounts, d_ids, d_hits, numCounts, &fired, &sum));
    std::vector<int> ids(fired);
    std::vector<unsigned long long> hits(fired);
    if (fired) {
        HIP(hipMemcpy(ids.data(), d_ids, fired * sizeof(int), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(hits.data(), d_hits, fired * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }

    printf("%s\nrule, hits\n", text.c_str());
    for (size_t i = 0; i < fired; i++) printf("%s, %llu\n", rules[(size_t)ids[i] - 1].c_str(), hits[i]);
    printf("%zu rules fired, %zu occurrences\n", fired, occurrences);

    /* self-check: every occurrence of every rule, counted by hand */
    std::vector<unsigned long long> want(numCounts, 0);
    size_t wantFired = 0, wantAll = 0;
    for (size_t r = 0; r < rules.size(); r++) {
        for (size_t at = text.find(rules[r]); at != std::string::npos; at = text.find(rules[r], at + 1)) want[r + 1]++;
        wantFired += want[r + 1] != 0;
        wantAll += want[r + 1];
    }
    bool ok = fired == wantFired && occurrences == wantAll && sum == wantAll;
    for (size_t i = 0; ok && i < fired; i++) ok = ids[i] >= 1 && (size_t)ids[i] < numCounts && hits[i] == want[(size_t)ids[i]] && (i == 0 || ids[i] > ids[i - 1]);
    if (!ok) {
        fprintf(stderr, "self-check FAILED: want %zu rules, %zu occurrences\n", wantFired, wantAll);
        return 1;
    }
    printf("self-check passed\n");

    (void)hipFree(d_text);
    (void)hipFree(d_counts);
    (void)hipFree(d_hits);
    (void)hipFree(d_ids);
    CHECK(PFAC_destroy(handle));
    return 0;
}
