/*
 * replace_example.cpp -- an anonymiser: every rule is a pattern and the string that takes its place ("alice@example.com" -> "<EMAIL>").  The text is
 * tokenised into disjoint leftmost-longest matches (PFACX_matchDisjoint*) and printed with every match replaced (PFACX_replace*), include/pfac_ext.h.
 *
 *   replace_example                      built-in rules and text, checked against a loop over the rules
 *   replace_example RULES [TEXT]         RULES: one "pattern<TAB>replacement" per line (no tab: the match is deleted); TEXT: a file, else stdin
 *
 * With a GPU the device forms run; without one the host forms on a host-only handle.
 */
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <utility>
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

template <class T>
static T *deviceCopy(const T *src, size_t count)
{
    T *d = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&d), (count ? count : 1) * sizeof(T)) != hipSuccess) return nullptr;
    if (count && src && hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
}

int main(int argc, char **argv)
{
    std::vector<std::pair<std::string, std::string>> rules = {
        {"alice@example.com", "<EMAIL>"}, {"bob@example.org", "<EMAIL>"}, {"10.0.0.7", "<IP>"}, {"10.0.0.77", "<IP>"},
        {"hunter2", ""}, {"password=", "pw="}, {"word=h", "!"}};
    std::string text = "login alice@example.com from 10.0.0.77 password=hunter2; cc bob@example.org via 10.0.0.7.";
    const bool builtin = argc < 2;
    if (!builtin) {
        rules.clear();
        std::ifstream rf(argv[1], std::ios::binary);
        if (!rf) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
        for (std::string line; std::getline(rf, line);) {
            if (line.empty()) continue;
            const size_t tab = line.find('\t');
            rules.emplace_back(line.substr(0, tab), tab == std::string::npos ? std::string() : line.substr(tab + 1));
        }
        if (argc > 2) {
            std::ifstream tf(argv[2], std::ios::binary);
            if (!tf) { fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
            text.assign(std::istreambuf_iterator<char>(tf), std::istreambuf_iterator<char>());
        } else {
            text.assign(std::istreambuf_iterator<char>(std::cin), std::istreambuf_iterator<char>());
        }
    }
    /* pattern k + 1 is rule k; the replacement of pattern id is replBytes[replOff[id], replOff[id + 1]): F + 2 offsets, entry 0 unused */
    std::string patterns, replBytes;
    std::vector<int> replOff = {0, 0};
    for (const auto &r : rules) {
        patterns += r.first + "\n";
        replBytes += r.second;
        replOff.push_back((int)replBytes.size());
    }
    const size_t n = text.size();

    int devices = 0;
    const bool gpu = hipGetDeviceCount(&devices) == hipSuccess && devices > 0;
    PFAC_handle_t handle = nullptr;
    if (gpu) CHECK(PFAC_create(&handle));
    else CHECK(PFACX_createHostOnly(&handle));
    CHECK(PFACX_readPatternFromMemory(handle, patterns.data(), patterns.size()));

    std::vector<int> ids(n ? n : 1), pos(n ? n : 1);                      /* capacity >= size: the arrays double as the scan's pair list */
    size_t numTokens = 0, covered = 0, outBytes = 0;
    std::string out;
    if (gpu) {
        char *d_text = deviceCopy(text.data(), n), *d_repl = deviceCopy(replBytes.data(), replBytes.size());
        int *d_ids = deviceCopy<int>(nullptr, n), *d_pos = deviceCopy<int>(nullptr, n), *d_off = deviceCopy(replOff.data(), replOff.size());
        if (!d_text || !d_repl || !d_ids || !d_pos || !d_off) { fprintf(stderr, "device memory\n"); return 1; }
        CHECK(PFACX_matchDisjointFromDevice(handle, d_text, n, d_ids, d_pos, n, &numTokens, &covered));
        /* the size query, then the text */
        const PFAC_status_t q = PFACX_replaceFromDevice(handle, d_text, n, d_ids, d_pos, numTokens, d_off, replOff.size(), d_repl, replBytes.size(),
                                                        nullptr, 0, &outBytes);
        if (q != PFAC_STATUS_SUCCESS && q != PFACX_STATUS_OUTPUT_TRUNCATED) { fprintf(stderr, "size query: %s\n", PFAC_getErrorString(q)); return 1; }
        char *d_out = deviceCopy<char>(nullptr, outBytes);
        if (!d_out) { fprintf(stderr, "device memory\n"); return 1; }
        CHECK(PFACX_replaceFromDevice(handle, d_text, n, d_ids, d_pos, numTokens, d_off, replOff.size(), d_repl, replBytes.size(), d_out, outBytes,
                                      &outBytes));
        out.resize(outBytes);
        if (numTokens) {
            HIP(hipMemcpy(ids.data(), d_ids, numTokens * sizeof(int), hipMemcpyDeviceToHost));
            HIP(hipMemcpy(pos.data(), d_pos, numTokens * sizeof(int), hipMemcpyDeviceToHost));
        }
        if (outBytes) HIP(hipMemcpy(&out[0], d_out, outBytes, hipMemcpyDeviceToHost));
        for (void *p : {(void *)d_text, (void *)d_repl, (void *)d_ids, (void *)d_pos, (void *)d_off, (void *)d_out}) (void)hipFree(p);
    } else {
        std::string copy = text;                                           /* (the call takes a char *; it does not write) */
        CHECK(PFACX_matchDisjointFromHost(handle, &copy[0], n, ids.data(), pos.data(), ids.size(), &numTokens, &covered));
        const PFAC_status_t q = PFACX_replaceFromHost(handle, text.data(), n, ids.data(), pos.data(), numTokens, replOff.data(), replOff.size(),
                                                      replBytes.data(), replBytes.size(), nullptr, 0, &outBytes);
        if (q != PFAC_STATUS_SUCCESS && q != PFACX_STATUS_OUTPUT_TRUNCATED) { fprintf(stderr, "size query: %s\n", PFAC_getErrorString(q)); return 1; }
        out.resize(outBytes);
        CHECK(PFACX_replaceFromHost(handle, text.data(), n, ids.data(), pos.data(), numTokens, replOff.data(), replOff.size(), replBytes.data(),
                                    replBytes.size(), outBytes ? &out[0] : nullptr, outBytes, &outBytes));
    }
    CHECK(PFAC_destroy(handle));

    fwrite(out.data(), 1, out.size(), stdout);
    if (!builtin) return 0;
    printf("\n%zu tokens, %zu bytes covered, %zu -> %zu bytes (%s forms)\n", numTokens, covered, n, outBytes, gpu ? "device" : "host");
    for (size_t k = 0; k < numTokens; k++)
        printf("token %zu: \"%s\" at %d -> \"%s\"\n", k, rules[ids[k] - 1].first.c_str(), pos[k], rules[ids[k] - 1].second.c_str());

    /* self-check: at every position the longest rule that matches there, by hand */
    std::string want;
    size_t wantTokens = 0, wantCovered = 0;
    for (size_t p = 0; p < n;) {
        size_t best = rules.size();
        for (size_t k = 0; k < rules.size(); k++)
            if (text.compare(p, rules[k].first.size(), rules[k].first) == 0 && (best == rules.size() || rules[k].first.size() > rules[best].first.size())) best = k;
        if (best == rules.size()) { want += text[p++]; continue; }
        want += rules[best].second;
        p += rules[best].first.size();
        wantTokens++;
        wantCovered += rules[best].first.size();
    }
    if (out != want || numTokens != wantTokens || covered != wantCovered) {
        fprintf(stderr, "self-check FAILED: want %zu tokens, %zu bytes:\n%s\n", wantTokens, wantCovered, want.c_str());
        return 1;
    }
    printf("self-check passed\n");
    return 0;
}
