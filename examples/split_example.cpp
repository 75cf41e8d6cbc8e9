/*
 * split_example.cpp -- keyword counts per line of a log that lies in device memory, with no copy back and no kernel of the caller's:
 *
 *     split_example PATTERN_FILE [LOG_FILE]          (no LOG_FILE: the log is read from stdin)
 *
 * The log is uploaded once.  PFACX_splitFromDevice cuts it at its newlines -- the count query first, then an array of exactly numSegments + 1
 * offsets --, and PFACX_countBatchFromDevice takes those offsets as they lie on the device.  Prints `line N: pattern x count ...` for every line
 * with an occurrence.  Without a GPU (PFAC_create fails) the same two steps run through the host forms on a host-only handle
 * (include/pfac_ext.h).
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
#define QUERY(call)                                                                            \
    do {                                                                                       \
        const PFAC_status_t st_ = (call);                                                      \
        if (st_ != PFAC_STATUS_SUCCESS && st_ != PFACX_STATUS_OUTPUT_TRUNCATED) {              \
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

static void print(const std::vector<size_t> &first, const std::vector<int> &ids, const std::vector<unsigned int> &counts, size_t lines, size_t longest,
                  unsigned long long occurrences)
{
    for (size_t k = 0; k < lines; k++) {
        if (first[k] == first[k + 1]) continue;
        printf("line %zu:", k + 1);
        for (size_t i = first[k]; i < first[k + 1]; i++) printf(" %d\xc3\x97%u", ids[i], counts[i]);
        printf("\n");
    }
    printf("%zu lines, the longest %zu bytes, %llu occurrences\n", lines, longest, occurrences);
}

int main(int argc, char **argv)
{
    if (argc < 2 || argc > 3) {
        fprintf(stderr, "usage: %s PATTERN_FILE [LOG_FILE]\n", argv[0]);
        return 2;
    }
    std::string log;
    FILE *in = argc == 3 ? fopen(argv[2], "rb") : stdin;
    if (!in) {
        fprintf(stderr, "cannot open %s\n", argv[2]);
        return 1;
    }
    char piece[1 << 16];
    for (size_t got; (got = fread(piece, 1, sizeof(piece), in)) > 0;) log.append(piece, got);
    if (in != stdin) fclose(in);
    const size_t n = log.size();
    if (n == 0) {
        printf("0 lines\n");
        return 0;
    }

    size_t lines = 0, longest = 0, entries = 0;
    unsigned long long occurrences = 0;
    std::vector<size_t> first;
    std::vector<int> ids;
    std::vector<unsigned int> counts;

    PFAC_handle_t handle = nullptr;
    if (PFAC_create(&handle) != PFAC_STATUS_SUCCESS) {
        /* no GPU: the host forms, the same two steps */
        CHECK(PFACX_createHostOnly(&handle));
        CHECK(PFAC_readPatternFromFile(handle, argv[1]));
        QUERY(PFACX_splitFromHost(handle, log.data(), n, nullptr, 0, nullptr, 0, &lines, &longest));
        std::vector<size_t> offsets(lines + 1);
        CHECK(PFACX_splitFromHost(handle, log.data(), n, nullptr, 0, offsets.data(), offsets.size(), &lines, &longest));
        first.resize(lines + 1);
        QUERY(PFACX_countBatchFromHost(handle, &log[0], n, offsets.data(), lines, 0, nullptr, nullptr, 0, first.data(), &entries, &occurrences));
        ids.resize(entries + 1);
        counts.resize(entries + 1);
        CHECK(PFACX_countBatchFromHost(handle, &log[0], n, offsets.data(), lines, 0, ids.data(), counts.data(), entries, first.data(), &entries, &occurrences));
        print(first, ids, counts, lines, longest, occurrences);
        CHECK(PFAC_destroy(handle));
        return 0;
    }
    CHECK(PFAC_readPatternFromFile(handle, argv[1]));

    char *d_log = nullptr;
    HIP(hipMalloc(reinterpret_cast<void **>(&d_log), n));
    HIP(hipMemcpy(d_log, log.data(), n, hipMemcpyHostToDevice));                                    /* the one upload */

    /* the lines: how many, then their offsets -- they never leave the device */
    QUERY(PFACX_splitFromDevice(handle, d_log, n, nullptr, 0, nullptr, 0, &lines, &longest));
    size_t *d_offsets = nullptr, *d_first = nullptr;
    HIP(hipMalloc(reinterpret_cast<void **>(&d_offsets), (lines + 1) * sizeof(size_t)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_first), (lines + 1) * sizeof(size_t)));
    CHECK(PFACX_splitFromDevice(handle, d_log, n, nullptr, 0, d_offsets, lines + 1, &lines, &longest));

    /* the counts of every pattern in every line: the count query, then arrays of exactly that length */
    QUERY(PFACX_countBatchFromDevice(handle, d_log, n, d_offsets, lines, 0, nullptr, nullptr, 0, d_first, &entries, &occurrences));
    int *d_ids = nullptr;
    unsigned int *d_counts = nullptr;
    HIP(hipMalloc(reinterpret_cast<void **>(&d_ids), (entries + 1) * sizeof(int)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_counts), (entries + 1) * sizeof(unsigned int)));
    CHECK(PFACX_countBatchFromDevice(handle, d_log, n, d_offsets, lines, 0, d_ids, d_counts, entries, d_first, &entries, &occurrences));

    first.resize(lines + 1);
    ids.resize(entries + 1);
    counts.resize(entries + 1);
    HIP(hipMemcpy(first.data(), d_first, (lines + 1) * sizeof(size_t), hipMemcpyDeviceToHost));
    if (entries) {
        HIP(hipMemcpy(ids.data(), d_ids, entries * sizeof(int), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(counts.data(), d_counts, entries * sizeof(unsigned int), hipMemcpyDeviceToHost));
    }
    print(first, ids, counts, lines, longest, occurrences);

    (void)hipFree(d_log);
    (void)hipFree(d_offsets);
    (void)hipFree(d_first);
    (void)hipFree(d_ids);
    (void)hipFree(d_counts);
    CHECK(PFAC_destroy(handle));
    return 0;
}
