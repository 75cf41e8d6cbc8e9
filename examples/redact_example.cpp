/*
 * redact_example.cpp -- scrub keywords out of a log line on the GPU: load a few keywords, print the spans of the text that belong to a match
 * (PFACX_matchSpansFromDevice), print the text with those bytes overwritten (PFACX_redactSpansFromDevice), and check both against what a
 * loop over the keywords says (include/pfac_ext.h).
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
    const std::vector<std::string> keywords = {"password=", "hunter2", "token", "tokens", "4111-1111"};
    const std::string text = "login ok user=ann password=hunter2 tokens=2 card 4111-1111-1111 token token";
    std::string patterns;
    for (const std::string &k : keywords) patterns += k + "\n";
    const size_t n = text.size();

    PFAC_handle_t handle = nullptr;
    CHECK(PFAC_create(&handle));
    CHECK(PFACX_readPatternFromMemory(handle, patterns.data(), patterns.size()));

    char *d_text = nullptr, *d_out = nullptr;
    int *d_start = nullptr, *d_len = nullptr;
    HIP(hipMalloc(reinterpret_cast<void **>(&d_text), n));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_out), n));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_start), n * sizeof(int)));           /* capacity >= size: the arrays double as the scan's pair list */
    HIP(hipMalloc(reinterpret_cast<void **>(&d_len), n * sizeof(int)));
    HIP(hipMemcpy(d_text, text.data(), n, hipMemcpyHostToDevice));

    size_t numSpans = 0, covered = 0;
    CHECK(PFACX_matchSpansFromDevice(handle, d_text, n, d_start, d_len, n, &numSpans, &covered));
    CHECK(PFACX_redactSpansFromDevice(handle, d_text, n, d_start, d_len, numSpans, '#', d_out));     /* asynchronous; the copies below wait for it */
    std::vector<int> start(numSpans), len(numSpans);
    std::string out(n, '\0');
    if (numSpans) {
        HIP(hipMemcpy(start.data(), d_start, numSpans * sizeof(int), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(len.data(), d_len, numSpans * sizeof(int), hipMemcpyDeviceToHost));
    }
    HIP(hipMemcpy(&out[0], d_out, n, hipMemcpyDeviceToHost));

    printf("%s\n", text.c_str());
    for (size_t i = 0; i < numSpans; i++) printf("span %zu: [%d, %d) \"%s\"\n", i, start[i], start[i] + len[i], text.substr(start[i], len[i]).c_str());
    printf("%s\n%zu spans, %zu bytes covered\n", out.c_str(), numSpans, covered);

    /* self-check: every occurrence of every keyword, painted by hand */
    std::string want = text;
    for (const std::string &k : keywords)
        for (size_t at = text.find(k); at != std::string::npos; at = text.find(k, at + 1)) want.replace(at, k.size(), std::string(k.size(), '#'));
    size_t wantCovered = 0, wantSpans = 0, sum = 0;
    for (size_t b = 0; b < n; b++) {
        wantCovered += want[b] != text[b];
        wantSpans += want[b] != text[b] && (b == 0 || want[b - 1] == text[b - 1]);
    }
    for (size_t i = 0; i < numSpans; i++) sum += (size_t)len[i];
    if (out != want || covered != wantCovered || numSpans != wantSpans || sum != covered) {
        fprintf(stderr, "self-check FAILED: want %zu spans, %zu bytes:\n%s\n", wantSpans, wantCovered, want.c_str());
        return 1;
    }
    printf("self-check passed\n");

    (void)hipFree(d_text);
    (void)hipFree(d_out);
    (void)hipFree(d_start);
    (void)hipFree(d_len);
    CHECK(PFAC_destroy(handle));
    return 0;
}
