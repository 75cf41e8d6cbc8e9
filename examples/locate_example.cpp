/*
 * locate_example.cpp -- `grep -n -b -o -F -f PATTERN_FILE` over a text that lies in device memory:
 *
 *     locate_example [PATTERN_FILE [TEXT_FILE]]      (no TEXT_FILE: the text is read from stdin; no argument at all: a small text of its own)
 *
 * PFACX_matchLocatedFromDevice scans the text and gives every match its line and its column where the text lies; only the four result arrays come
 * back.  Prints `line:col:pattern` for every match, both counted from 1 as grep counts lines (the library counts from 0).  Without a GPU
 * (PFAC_create fails) the host form runs on a host-only handle (include/pfac_ext.h).
 */
#include <hip/hip_runtime_api.h>

#include <cstdio>
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

static const char kPatterns[] = "ERROR\ntimeout\nuser=\n";
static const char kText[] = "10:00 INFO start user=ann\n10:01 ERROR timeout after 30s user=bob\n\n10:02 INFO done\n10:03 ERROR disk full";

int main(int argc, char **argv)
{
    if (argc > 3) {
        fprintf(stderr, "usage: %s [PATTERN_FILE [TEXT_FILE]]\n", argv[0]);
        return 2;
    }
    std::string text;
    if (argc == 1) {
        text = kText;
    } else {
        FILE *in = argc == 3 ? fopen(argv[2], "rb") : stdin;
        if (!in) {
            fprintf(stderr, "cannot open %s\n", argv[2]);
            return 1;
        }
        char piece[1 << 16];
        for (size_t got; (got = fread(piece, 1, sizeof(piece), in)) > 0;) text.append(piece, got);
        if (in != stdin) fclose(in);
    }
    const size_t n = text.size();
    if (n == 0) return 0;

    PFAC_handle_t handle = nullptr;
    const bool onDevice = PFAC_create(&handle) == PFAC_STATUS_SUCCESS;
    if (!onDevice) CHECK(PFACX_createHostOnly(&handle));
    if (argc == 1) CHECK(PFACX_readPatternFromMemory(handle, kPatterns, sizeof(kPatterns) - 1));
    else CHECK(PFAC_readPatternFromFile(handle, argv[1]));

    int found = 0;
    std::vector<int> ids(n), pos(n), line(n), col(n);
    if (!onDevice) {
        /* no GPU: the host form, the same call */
        CHECK(PFACX_matchLocatedFromHost(handle, &text[0], n, nullptr, 0, ids.data(), pos.data(), line.data(), col.data(), n, &found));
    } else {
        char *d_text = nullptr;
        int *d_out = nullptr;                                                                       /* ids, positions, lines, columns: n entries each */
        HIP(hipMalloc(reinterpret_cast<void **>(&d_text), n));
        HIP(hipMalloc(reinterpret_cast<void **>(&d_out), 4 * n * sizeof(int)));
        HIP(hipMemcpy(d_text, text.data(), n, hipMemcpyHostToDevice));                              /* the one upload */
        CHECK(PFACX_matchLocatedFromDevice(handle, d_text, n, nullptr, 0, d_out, d_out + n, d_out + 2 * n, d_out + 3 * n, n, &found));
        if (found) {
            const size_t bytes = (size_t)found * sizeof(int);
            HIP(hipMemcpy(ids.data(), d_out, bytes, hipMemcpyDeviceToHost));
            HIP(hipMemcpy(line.data(), d_out + 2 * n, bytes, hipMemcpyDeviceToHost));
            HIP(hipMemcpy(col.data(), d_out + 3 * n, bytes, hipMemcpyDeviceToHost));
        }
        (void)hipFree(d_text);
        (void)hipFree(d_out);
    }
    for (int i = 0; i < found; i++) printf("%d:%d:pattern %d\n", line[i] + 1, col[i] + 1, ids[i]);
    CHECK(PFAC_destroy(handle));
    return 0;
}
