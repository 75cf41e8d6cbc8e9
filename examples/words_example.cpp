/*
 * words_example.cpp -- whole-word term frequencies on the GPU: every occurrence of a keyword that is a word of its own
 * (PFACX_matchWordsFromDevice with PFACX_WORDS_ALL: `the` does not count inside `other`, `then` or `bathe`), counted per keyword
 * (PFACX_countPairsFromDevice with PFACX_COUNT_LONGEST over the list), and checked against what a loop over the keywords says
 * (include/pfac_ext.h).
 */
#include <hip/hip_runtime_api.h>

#include <cctype>
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

static bool wordByte(char c) { return std::isalnum((unsigned char)c) || c == '_'; }

int main()
{
    /* "the end" holds "the": both are whole words there, and PFACX_WORDS_ALL reports both */
    const std::vector<std::string> words = {"the", "then", "other", "he", "the end", "never seen"};
    const std::string text = "the other then bathe the, then the end he said: the-end of the other";
    std::string patterns;
    for (const std::string &w : words) patterns += w + "\n";
    const size_t n = text.size(), numCounts = words.size() + 1;            /* counts are indexed by pattern id: 1 .. F */

    PFAC_handle_t handle = nullptr;
    CHECK(PFAC_create(&handle));
    CHECK(PFACX_readPatternFromMemory(handle, patterns.data(), patterns.size()));

    char *d_text = nullptr;
    int *d_ids = nullptr, *d_pos = nullptr;
    unsigned long long *d_counts = nullptr;
    const size_t capacity = 2 * n;                                          /* >= size; a longer list is reported, not written */
    HIP(hipMalloc(reinterpret_cast<void **>(&d_text), n));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_ids), capacity * sizeof(int)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_pos), capacity * sizeof(int)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_counts), numCounts * sizeof(unsigned long long)));
    HIP(hipMemcpy(d_text, text.data(), n, hipMemcpyHostToDevice));

    size_t listed = 0;
    CHECK(PFACX_matchWordsFromDevice(handle, d_text, n, nullptr /* [0-9A-Za-z_] */, PFACX_WORDS_ALL, d_ids, d_pos, capacity, &listed));
    CHECK(PFACX_countPairsFromDevice(handle, d_ids, listed, PFACX_COUNT_LONGEST, d_counts, numCounts));
    std::vector<int> ids(listed), pos(listed);
    std::vector<unsigned long long> counts(numCounts);
    if (listed) {
        HIP(hipMemcpy(ids.data(), d_ids, listed * sizeof(int), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(pos.data(), d_pos, listed * sizeof(int), hipMemcpyDeviceToHost));
    }
    HIP(hipMemcpy(counts.data(), d_counts, numCounts * sizeof(unsigned long long), hipMemcpyDeviceToHost));   /* (waits for the count) */

    printf("%s\n", text.c_str());
    for (size_t i = 0; i < listed; i++) printf("%3d  %s\n", pos[i], words[(size_t)ids[i] - 1].c_str());
    printf("word, whole-word occurrences\n");
    for (size_t w = 0; w < words.size(); w++) printf("%s, %llu\n", words[w].c_str(), counts[w + 1]);

    /* self-check: every occurrence of every keyword with no word byte on either side, counted by hand */
    std::vector<unsigned long long> want(numCounts, 0);
    size_t wantAll = 0;
    for (size_t w = 0; w < words.size(); w++)
        for (size_t at = text.find(words[w]); at != std::string::npos; at = text.find(words[w], at + 1)) {
            const size_t end = at + words[w].size();
            if ((at == 0 || !wordByte(text[at - 1])) && (end == n || !wordByte(text[end]))) { want[w + 1]++; wantAll++; }
        }
    bool ok = listed == wantAll && want[1] == 5 && want[2] == 2;           /* `the`: five whole words of the ten places it occurs in */
    for (size_t id = 1; ok && id < numCounts; id++) ok = counts[id] == want[id];
    for (size_t i = 1; ok && i < listed; i++) ok = pos[i] >= pos[i - 1];
    if (!ok) {
        fprintf(stderr, "self-check FAILED: want %zu whole-word occurrences, got %zu\n", wantAll, listed);
        return 1;
    }
    printf("self-check passed\n");

    (void)hipFree(d_text);
    (void)hipFree(d_ids);
    (void)hipFree(d_pos);
    (void)hipFree(d_counts);
    CHECK(PFAC_destroy(handle));
    return 0;
}
