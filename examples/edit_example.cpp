/*
 * edit_example.cpp -- keywords found within one edit, indels included (PFACX_edit*, include/pfac_ext.h): `pasword` (a letter dropped),
 * `passsword` (a letter doubled) and `passw0rd` (a letter replaced) are all found, with PFACX_EDIT_BEST_ENDS one entry per place.
 * The self-check compares the list with Sellers' recurrence over the whole input, written out below.
 *
 * Build: make -C examples edit_example        Run: examples/edit_example
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
    const std::vector<std::string> keywords = {"password", "username", "firewall", "download", "attachment", "certificate"};
    const std::string input =
        "Your pasword and your usernamee were sent; the passsword list is an atachment. The firevall blocked a downlaod (two letters swapped: "
        "two edits, not found) and the certifcate is fine; passw0rd, password.";
    const size_t n = input.size(), S = keywords.size();

    std::string bytes;
    std::vector<size_t> patOff(1, 0);
    for (const std::string &k : keywords) {
        bytes += k;
        patOff.push_back(bytes.size());
    }
    const std::vector<int> budget(S, 1);                                    /* one edit each */

    PFAC_handle_t handle = nullptr;
    CHECK(PFAC_create(&handle));
    PFACX_edit_t edit = nullptr;
    int badPattern = 0;
    CHECK(PFACX_editOpen(handle, reinterpret_cast<const unsigned char *>(bytes.data()), patOff.data(), budget.data(), S, 0, 0, PFACX_EDIT_BEST_ENDS,
                         &edit, &badPattern));                              /* loads the pieces into the handle */

    char *d_input = nullptr;
    int *d_ids = nullptr, *d_pos = nullptr, *d_end = nullptr, *d_dist = nullptr;
    const size_t capacity = n;                                              /* the device form wants capacity >= size */
    HIP(hipMalloc(reinterpret_cast<void **>(&d_input), n));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_ids), capacity * sizeof(int)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_pos), capacity * sizeof(int)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_end), capacity * sizeof(int)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_dist), capacity * sizeof(int)));
    HIP(hipMemcpy(d_input, input.data(), n, hipMemcpyHostToDevice));

    size_t listed = 0;
    CHECK(PFACX_editMatchFromDevice(edit, d_input, n, d_ids, d_pos, d_end, d_dist, capacity, &listed));
    std::vector<int> ids(listed), pos(listed), end(listed), dist(listed);
    if (listed) {
        HIP(hipMemcpy(ids.data(), d_ids, listed * sizeof(int), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(pos.data(), d_pos, listed * sizeof(int), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(end.data(), d_end, listed * sizeof(int), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(dist.data(), d_dist, listed * sizeof(int), hipMemcpyDeviceToHost));
    }
    std::vector<std::tuple<int, int, int, int>> got, want;
    printf("occurrences, in the order of their candidate positions:\n");
    for (size_t i = 0; i < listed; i++) {
        printf("  %-12s [%3d, %3d) as \"%s\" (%d edit%s)\n", keywords[(size_t)ids[i] - 1].c_str(), pos[i], end[i],
               input.substr((size_t)pos[i], (size_t)(end[i] - pos[i])).c_str(), dist[i], dist[i] == 1 ? "" : "s");
        got.emplace_back(ids[i], pos[i], end[i], dist[i]);
    }

    /* self-check: Sellers' recurrence, a column per end; a cell is (cost, start), the lower cost first, then the larger start */
    for (size_t i = 0; i < S; i++) {
        const std::string &pat = keywords[i];
        const size_t L = pat.size();
        std::vector<std::pair<int, int>> D(n + 1);
        std::vector<std::pair<int, int>> above(L + 1), here(L + 1);
        const auto less = [](const std::pair<int, int> &a, const std::pair<int, int> &b) { return a.first != b.first ? a.first < b.first : a.second > b.second; };
        for (size_t c = 0; c <= n; c++) {
            here[0] = {0, (int)c};
            for (size_t r = 1; r <= L; r++) {
                std::pair<int, int> best = {here[r - 1].first + 1, here[r - 1].second};
                if (c > 0) {
                    const std::pair<int, int> diag = {above[r - 1].first + (pat[r - 1] != input[c - 1]), above[r - 1].second};
                    const std::pair<int, int> left = {above[r].first + 1, above[r].second};
                    if (less(diag, best)) best = diag;
                    if (less(left, best)) best = left;
                }
                here[r] = best;
            }
            D[c] = here[L];
            above = here;
        }
        for (size_t e = 1; e <= n; e++)
            if (D[e].first <= budget[i] && D[e - 1].first > D[e].first && (e == n || D[e + 1].first >= D[e].first))
                want.emplace_back((int)i + 1, D[e].second, (int)e, D[e].first);
    }
    std::sort(got.begin(), got.end());
    std::sort(want.begin(), want.end());
    if (got != want || want.size() != 8) {
        fprintf(stderr, "self-check FAILED: %zu listed, %zu by the definition\n", got.size(), want.size());
        return 1;
    }
    printf("self-check passed\n");

    (void)hipFree(d_input);
    (void)hipFree(d_ids);
    (void)hipFree(d_pos);
    (void)hipFree(d_end);
    (void)hipFree(d_dist);
    CHECK(PFACX_editClose(edit));
    CHECK(PFAC_destroy(handle));
    return 0;
}
