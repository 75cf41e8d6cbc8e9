/*
 * lines_example.cpp -- grep -F -f PATTERNS TEXT on the GPU: print the lines of TEXT that contain a pattern of PATTERNS.
 *   lines_example [-v] [-i] PATTERNS TEXT      -v: the lines that contain none; -i: ignore ASCII case
 * PFACX_matchLinesFromDevice selects the lines, PFACX_gatherLinesFromDevice turns them into text (include/pfac_ext.h).
 */
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
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

int main(int argc, char **argv)
{
    unsigned int lineFlags = 0, readFlags = 0;
    int arg = 1;
    for (; arg < argc && argv[arg][0] == '-'; arg++) {
        if (!strcmp(argv[arg], "-v")) lineFlags |= PFACX_LINES_INVERT;
        else if (!strcmp(argv[arg], "-i")) readFlags |= PFACX_READ_NOCASE;
        else break;
    }
    if (argc - arg != 2) {
        fprintf(stderr, "usage: %s [-v] [-i] PATTERNS TEXT\n", argv[0]);
        return 2;
    }
    std::ifstream f(argv[arg + 1], std::ios::binary);
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[arg + 1]);
        return 2;
    }
    std::vector<char> text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const size_t n = text.size();

    PFAC_handle_t handle = nullptr;
    CHECK(PFAC_create(&handle));
    CHECK(PFACX_readPatternFromFileEx(handle, argv[arg], readFlags));
    if (n == 0) return PFAC_destroy(handle) == PFAC_STATUS_SUCCESS ? 0 : 1;

    char *d_text = nullptr, *d_out = nullptr;
    int *d_start = nullptr, *d_len = nullptr;
    HIP(hipMalloc(reinterpret_cast<void **>(&d_text), n));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_start), n * sizeof(int)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_len), n * sizeof(int)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_out), n + 1));                     /* the text of the selected lines is at most size + 1 bytes */
    HIP(hipMemcpy(d_text, text.data(), n, hipMemcpyHostToDevice));

    size_t numLines = 0, numSelected = 0, outBytes = 0;
    CHECK(PFACX_matchLinesFromDevice(handle, d_text, n, lineFlags, d_start, d_len, nullptr, n, &numLines, &numSelected));
    CHECK(PFACX_gatherLinesFromDevice(handle, d_text, n, d_start, d_len, numSelected, d_out, n + 1, &outBytes));
    std::vector<char> out(outBytes);
    if (outBytes) HIP(hipMemcpy(out.data(), d_out, outBytes, hipMemcpyDeviceToHost));
    fwrite(out.data(), 1, out.size(), stdout);
    fprintf(stderr, "%zu of %zu lines\n", numSelected, numLines);

    (void)hipFree(d_text);
    (void)hipFree(d_start);
    (void)hipFree(d_len);
    (void)hipFree(d_out);
    CHECK(PFAC_destroy(handle));
    return 0;
}
