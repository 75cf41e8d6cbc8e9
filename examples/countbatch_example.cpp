/*
 * countbatch_example.cpp -- keyword counts per line of a small log on the GPU: load a few keywords, cut the log at its newlines, count every
 * occurrence of every keyword in every line with one call (PFACX_countBatchFromDevice: the count query first, then arrays of exactly that length),
 * print `line: id x count ...`, and check the list against what a loop over the lines and the keywords says (include/pfac_ext.h).
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
    /* "timeout" holds "time", "error: disk" holds "error": the longest match hides them, the counts do not */
    const std::vector<std::string> keywords = {"error", "error: disk", "time", "timeout", "retry", "never seen"};
    const std::string log =
        "boot ok\n"
        "error: disk full, retry retry retry\n"
        "\n"
        "timeout after some time, error\n"
        "retry at time 12: timeout timeout\n";
    std::string patterns;
    for (const std::string &k : keywords) patterns += k + "\n";
    std::vector<size_t> offsets = {0};                                      /* a line is a segment, its newline included */
    for (size_t i = 0; i < log.size(); i++)
        if (log[i] == '\n') offsets.push_back(i + 1);
    if (offsets.back() != log.size()) offsets.push_back(log.size());
    const size_t n = log.size(), lines = offsets.size() - 1;

    PFAC_handle_t handle = nullptr;
    CHECK(PFAC_create(&handle));
    CHECK(PFACX_readPatternFromMemory(handle, patterns.data(), patterns.size()));

    char *d_log = nullptr;
    size_t *d_offsets = nullptr, *d_first = nullptr;
    HIP(hipMalloc(reinterpret_cast<void **>(&d_log), n));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_offsets), (lines + 1) * sizeof(size_t)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_first), (lines + 1) * sizeof(size_t)));
    HIP(hipMemcpy(d_log, log.data(), n, hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_offsets, offsets.data(), (lines + 1) * sizeof(size_t), hipMemcpyHostToDevice));

    size_t entries = 0;
    unsigned long long occurrences = 0;
    PFAC_status_t st = PFACX_countBatchFromDevice(handle, d_log, n, d_offsets, lines, 0, nullptr, nullptr, 0, d_first, &entries, &occurrences);
    if (st != PFAC_STATUS_SUCCESS && st != PFACX_STATUS_OUTPUT_TRUNCATED) CHECK(st);                 /* the count query: how long is the list? */
    int *d_ids = nullptr;
    unsigned int *d_counts = nullptr;
    HIP(hipMalloc(reinterpret_cast<void **>(&d_ids), (entries + 1) * sizeof(int)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_counts), (entries + 1) * sizeof(unsigned int)));
    CHECK(PFACX_countBatchFromDevice(handle, d_log, n, d_offsets, lines, 0, d_ids, d_counts, entries, d_first, &entries, &occurrences));
    std::vector<int> ids(entries);
    std::vector<unsigned int> counts(entries);
    std::vector<size_t> first(lines + 1);
    if (entries) {
        HIP(hipMemcpy(ids.data(), d_ids, entries * sizeof(int), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(counts.data(), d_counts, entries * sizeof(unsigned int), hipMemcpyDeviceToHost));
    }
    HIP(hipMemcpy(first.data(), d_first, (lines + 1) * sizeof(size_t), hipMemcpyDeviceToHost));

    for (size_t k = 0; k < lines; k++) {
        printf("%zu:", k + 1);
        for (size_t i = first[k]; i < first[k + 1]; i++) printf(" %d\xc3\x97%u", ids[i], counts[i]);
        printf("\n");
    }
    printf("%zu entries, %llu occurrences in %zu lines\n", entries, occurrences, lines);

    /* self-check: every occurrence of every keyword inside every line, counted by hand */
    bool ok = first[0] == 0 && first[lines] == entries;
    size_t at = 0;
    unsigned long long wantAll = 0;
    for (size_t k = 0; ok && k < lines; k++) {
        const std::string line = log.substr(offsets[k], offsets[k + 1] - offsets[k]);
        for (size_t id = 1; ok && id <= keywords.size(); id++) {
            unsigned int want = 0;
            for (size_t p = line.find(keywords[id - 1]); p != std::string::npos; p = line.find(keywords[id - 1], p + 1)) want++;
            if (want == 0) continue;
            ok = at < first[k + 1] && at >= first[k] && ids[at] == (int)id && counts[at] == want;
            wantAll += want;
            at++;
        }
        ok = ok && at == first[k + 1];
    }
    ok = ok && at == entries && occurrences == wantAll;
    if (!ok) {
        fprintf(stderr, "self-check FAILED\n");
        return 1;
    }
    printf("self-check passed\n");

    (void)hipFree(d_log);
    (void)hipFree(d_offsets);
    (void)hipFree(d_first);
    (void)hipFree(d_ids);
    (void)hipFree(d_counts);
    CHECK(PFAC_destroy(handle));
    return 0;
}
