/*
 * approx_example.cpp -- patterns matched within k mismatches (PFACX_approxOpen / PFACX_approxGetPieces / PFACX_approxMatchFromDevice,
 * include/pfac_ext.h): a dozen keywords, each allowed one wrong letter, over a short text with typos.  The library cuts every keyword into
 * k + 1 parts, scans for the heads of the parts and counts the differing bytes of every keyword around every occurrence of a piece; the list
 * holds (keyword id, start) and the distance.
 */
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <tuple>
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
    const std::vector<std::string> keywords = {"password", "username", "passport", "creditcard", "security", "firewall",
                                               "download", "attachment", "database", "encryption", "malicious", "certificate"};
    const std::string input =
        "Your pasword (a letter is missing: not found) and usernane were sent; the passp0rt scan is an attachnent. The firevall blocked a downlaod (two letters swapped: not "
        "found) from a maliciou5 host, the databa5e keeps its encrypt1on and the certifikate is fine; password, once more, spelled right.";
    const size_t n = input.size(), S = keywords.size();

    std::string bytes;
    std::vector<size_t> patOff(1, 0);
    for (const std::string &k : keywords) {
        bytes += k;
        patOff.push_back(bytes.size());
    }
    const std::vector<int> budget(S, 1);                                    /* one substitution each */

    PFAC_handle_t handle = nullptr;
    CHECK(PFAC_create(&handle));
    PFACX_approx_t approx = nullptr;
    int badPattern = 0;
    CHECK(PFACX_approxOpen(handle, reinterpret_cast<const unsigned char *>(bytes.data()), patOff.data(), budget.data(), S, 0, 0, &approx,
                           &badPattern));                                   /* loads the pieces into the handle */
    std::vector<size_t> pieceOff(S + 2);
    CHECK(PFACX_approxGetPieces(approx, pieceOff.data(), nullptr, nullptr, nullptr, 0));
    const size_t pieces = pieceOff[S + 1];
    std::vector<int> pieceId(pieces), pieceStart(pieces), pieceLen(pieces);
    CHECK(PFACX_approxGetPieces(approx, nullptr, pieceId.data(), pieceStart.data(), pieceLen.data(), pieces));
    for (size_t i = 1; i <= S; i++) {
        printf("keyword %2zu  %-12s pieces:", i, keywords[i - 1].c_str());
        for (size_t e = pieceOff[i]; e < pieceOff[i + 1]; e++)
            printf("  %s (pattern %d)", keywords[i - 1].substr((size_t)pieceStart[e], (size_t)pieceLen[e]).c_str(), pieceId[e]);
        printf("\n");
    }

    char *d_input = nullptr;
    int *d_ids = nullptr, *d_pos = nullptr, *d_mis = nullptr;
    const size_t capacity = n;                                              /* the device form wants capacity >= size */
    HIP(hipMalloc(reinterpret_cast<void **>(&d_input), n));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_ids), capacity * sizeof(int)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_pos), capacity * sizeof(int)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_mis), capacity * sizeof(int)));
    HIP(hipMemcpy(d_input, input.data(), n, hipMemcpyHostToDevice));

    size_t listed = 0;
    CHECK(PFACX_approxMatchFromDevice(approx, d_input, n, d_ids, d_pos, d_mis, capacity, &listed));
    std::vector<int> ids(listed), pos(listed), mis(listed);
    if (listed) {
        HIP(hipMemcpy(ids.data(), d_ids, listed * sizeof(int), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(pos.data(), d_pos, listed * sizeof(int), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(mis.data(), d_mis, listed * sizeof(int), hipMemcpyDeviceToHost));
    }
    std::vector<std::tuple<int, int, int>> got, want;
    printf("occurrences, in the order of their candidate positions:\n");
    for (size_t i = 0; i < listed; i++) {
        const std::string &k = keywords[(size_t)ids[i] - 1];
        printf("  %-12s at %3d as \"%s\" (%d wrong)\n", k.c_str(), pos[i], input.substr((size_t)pos[i], k.size()).c_str(), mis[i]);
        got.emplace_back(pos[i], ids[i], mis[i]);
    }

    /* self-check: the definition, byte by byte -- every keyword at every start with at most one differing byte */
    for (size_t i = 0; i < S; i++)
        for (size_t s = 0; s + keywords[i].size() <= n; s++) {
            int d = 0;
            for (size_t t = 0; t < keywords[i].size(); t++) d += input[s + t] != keywords[i][t];
            if (d <= budget[i]) want.emplace_back((int)s, (int)i + 1, d);
        }
    std::sort(got.begin(), got.end());
    std::sort(want.begin(), want.end());
    if (got != want || want.size() != 9 || pieces != 2 * S) {
        fprintf(stderr, "self-check FAILED: %zu listed, %zu by the definition\n", got.size(), want.size());
        return 1;
    }
    printf("self-check passed\n");

    (void)hipFree(d_input);
    (void)hipFree(d_ids);
    (void)hipFree(d_pos);
    (void)hipFree(d_mis);
    CHECK(PFACX_approxClose(approx));
    CHECK(PFAC_destroy(handle));
    return 0;
}
