/*
 * capture_example.cpp -- "the patterns are keys, give me the values" over an HTTP-like text that lies in device memory:
 *
 *     capture_example          (no arguments: a small text of its own)
 *
 * PFACX_matchCapturedFromDevice scans the text for three header keys and gives every match the (start, length) of the value behind it -- blanks
 * skipped (S = {' ', '\t'}), ended by the line's end (D = {'\r', '\n'}) -- and PFACX_gatherLinesFromDevice writes the values as text, one per line:
 * two calls, no host round trip; only the text of the values comes back.  Checks itself against a host loop and exits non-zero on a mismatch.
 * Without a GPU (PFAC_create fails) the host form runs on a host-only handle and the values are cut out on the host (include/pfac_ext.h).
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

static const char kPatterns[] = "Host:\nContent-Length:\nUser-Agent:\n";
static const char kText[] =
    "GET /a HTTP/1.1\r\nHost: one.example\r\nUser-Agent:\tcurl/8.5\r\nAccept: */*\r\n\r\n"
    "POST /b HTTP/1.1\r\nHost:    two.example\r\nContent-Length: 11\r\nUser-Agent:\r\n\r\nhello world"
    "GET /c HTTP/1.1\nHost:three.example\n\n";

static void setClass(unsigned int *cls, const char *members)
{
    std::memset(cls, 0, 8 * sizeof(unsigned int));
    for (const char *m = members; *m; m++) cls[(unsigned char)*m >> 5] |= 1u << ((unsigned char)*m & 31u);
}

int main()
{
    const std::string text = kText;
    const size_t n = text.size();
    unsigned int skip[8], stop[8];
    setClass(skip, " \t");
    setClass(stop, "\r\n");

    PFAC_handle_t handle = nullptr;
    const bool onDevice = PFAC_create(&handle) == PFAC_STATUS_SUCCESS;
    if (!onDevice) CHECK(PFACX_createHostOnly(&handle));
    CHECK(PFACX_readPatternFromMemory(handle, kPatterns, sizeof(kPatterns) - 1));

    int found = 0;
    std::vector<int> ids(n), pos(n), valStart(n), valLen(n);
    std::string values;
    if (!onDevice) {
        /* no GPU: the host form, the same call */
        std::string copy = text;
        CHECK(PFACX_matchCapturedFromHost(handle, &copy[0], n, skip, stop, 0, 0, ids.data(), pos.data(), valStart.data(), valLen.data(), n, &found));
        for (int i = 0; i < found; i++) values += text.substr((size_t)valStart[i], (size_t)valLen[i]) + "\n";
    } else {
        char *d_text = nullptr, *d_values = nullptr;
        int *d_out = nullptr;                                                                       /* ids, positions, starts, lengths: n entries each */
        HIP(hipMalloc(reinterpret_cast<void **>(&d_text), n));
        HIP(hipMalloc(reinterpret_cast<void **>(&d_values), 2 * n + 1));
        HIP(hipMalloc(reinterpret_cast<void **>(&d_out), 4 * n * sizeof(int)));
        HIP(hipMemcpy(d_text, text.data(), n, hipMemcpyHostToDevice));                              /* the one upload */
        CHECK(PFACX_matchCapturedFromDevice(handle, d_text, n, skip, stop, 0, 0, d_out, d_out + n, d_out + 2 * n, d_out + 3 * n, n, &found));
        size_t bytes = 0;
        CHECK(PFACX_gatherLinesFromDevice(handle, d_text, n, d_out + 2 * n, d_out + 3 * n, (size_t)found, d_values, 2 * n + 1, &bytes));
        values.resize(bytes);
        if (bytes) HIP(hipMemcpy(&values[0], d_values, bytes, hipMemcpyDeviceToHost));              /* the one download */
        if (found) {
            HIP(hipMemcpy(ids.data(), d_out, (size_t)found * sizeof(int), hipMemcpyDeviceToHost));  /* ... and, for the check below, the pairs */
            HIP(hipMemcpy(pos.data(), d_out + n, (size_t)found * sizeof(int), hipMemcpyDeviceToHost));
        }
        (void)hipFree(d_text);
        (void)hipFree(d_values);
        (void)hipFree(d_out);
    }
    fputs(values.c_str(), stdout);

    /* the check: the same values by a host loop over the text */
    static const char *const keys[] = {"Host:", "Content-Length:", "User-Agent:"};
    std::string want;
    int wantFound = 0;
    for (size_t p = 0; p < n; p++) {
        for (const char *key : keys) {
            const size_t len = std::strlen(key);
            if (text.compare(p, len, key) != 0) continue;
            size_t s = p + len;
            while (s < n && (text[s] == ' ' || text[s] == '\t')) s++;
            size_t e = s;
            while (e < n && text[e] != '\r' && text[e] != '\n') e++;
            want += text.substr(s, e - s) + "\n";
            if (wantFound < found && (pos[(size_t)wantFound] != (int)p || std::strcmp(keys[ids[(size_t)wantFound] - 1], key) != 0)) wantFound = -(int)n - 1;
            wantFound++;
        }
    }
    CHECK(PFAC_destroy(handle));
    if (wantFound != found || want != values) {
        fprintf(stderr, "MISMATCH: %d values (want %d)\n%s--- want ---\n%s", found, wantFound, values.c_str(), want.c_str());
        return 1;
    }
    return 0;
}
