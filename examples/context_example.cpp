/*
 * context_example.cpp -- grep -n -C 1 -F -f PATTERNS over a small log on the GPU: the lines that contain a pattern with one line of context on
 * either side, the matching lines marked ':', the context '-', and "--" between groups of lines that are not adjacent.
 * PFACX_matchLinesContextFromDevice selects the lines and tags them (include/pfac_ext.h): lineTag = group << 1 | (1: the line matches).
 */
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
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
    const char patterns[] = "ERROR\ntimeout\n";
    const char log[] =
        "10:00:01 GET /index.html 200\n"
        "10:00:02 GET /api/items 200\n"
        "10:00:03 upstream timeout after 30 s\n"
        "10:00:03 ERROR GET /api/items 504\n"
        "10:00:04 GET /favicon.ico 404\n"
        "10:00:05 GET /index.html 200\n"
        "10:00:06 GET /about.html 200\n"
        "10:00:07 POST /login 302\n"
        "10:00:08 ERROR session store unreachable\n"
        "10:00:09 GET /index.html 200\n";
    const size_t n = sizeof log - 1;

    PFAC_handle_t handle = nullptr;
    CHECK(PFAC_create(&handle));
    CHECK(PFACX_readPatternFromMemory(handle, patterns, sizeof patterns - 1));

    char *d_log = nullptr;
    int *d_start = nullptr, *d_len = nullptr, *d_index = nullptr, *d_tag = nullptr;
    HIP(hipMalloc(reinterpret_cast<void **>(&d_log), n));
    for (int **p : {&d_start, &d_len, &d_index, &d_tag}) HIP(hipMalloc(reinterpret_cast<void **>(p), n * sizeof(int)));   /* capacity >= size */
    HIP(hipMemcpy(d_log, log, n, hipMemcpyHostToDevice));

    size_t numLines = 0, numSelected = 0, numMatching = 0, numGroups = 0;
    CHECK(PFACX_matchLinesContextFromDevice(handle, d_log, n, 0, /* before */ 1, /* after */ 1, d_start, d_len, d_index, d_tag, n, &numLines, &numSelected,
                                            &numMatching, &numGroups));
    std::vector<int> start(numSelected), len(numSelected), index(numSelected), tag(numSelected);
    if (numSelected) {
        HIP(hipMemcpy(start.data(), d_start, numSelected * sizeof(int), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(len.data(), d_len, numSelected * sizeof(int), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(index.data(), d_index, numSelected * sizeof(int), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(tag.data(), d_tag, numSelected * sizeof(int), hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < numSelected; i++) {
        if (i > 0 && (tag[i] >> 1) != (tag[i - 1] >> 1)) puts("--");              /* the group changes: the line numbers jump */
        printf("%d%c%.*s\n", index[i] + 1, (tag[i] & 1) ? ':' : '-', len[i], log + start[i]);
    }
    fprintf(stderr, "%zu of %zu lines in %zu groups, %zu of them match\n", numSelected, numLines, numGroups, numMatching);

    (void)hipFree(d_log);
    for (int *p : {d_start, d_len, d_index, d_tag}) (void)hipFree(p);
    CHECK(PFAC_destroy(handle));
    return 0;
}
