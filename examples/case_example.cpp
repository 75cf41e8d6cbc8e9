/*
 * case_example.cpp -- `nocase` as a property of each pattern, as in a Snort rule's `content:`: one caseless handle, one scan, and per pattern
 * the choice between "in any case" and "exactly as written" (PFACX_caseOpen / PFACX_caseMatchFromDevice, include/pfac_ext.h).  A sensitive `GET`,
 * a sensitive `get` and a caseless `Get` are three patterns over the same folded text; `Host: ` matches in any case, `AKIA` only as written.
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

int main()
{
    const std::vector<std::string> lines = {"GET", "get", "Get", "Host: ", "AKIA"};
    const unsigned char sensitive[] = {0, 1, 1, 0, 0, 1};                   /* by id, entry 0 unused: `Get` and `Host: ` in any case */
    const std::string text = "GET get gEt Get HOST: akia AKIA";
    std::string patterns;
    for (const std::string &l : lines) patterns += l + "\n";
    const size_t n = text.size();

    PFAC_handle_t handle = nullptr;
    CHECK(PFAC_create(&handle));
    CHECK(PFACX_readPatternFromMemoryEx(handle, patterns.data(), patterns.size(), PFACX_READ_NOCASE));
    PFACX_case_t cs = nullptr;
    int most = 0;
    CHECK(PFACX_caseOpen(handle, patterns.data(), patterns.size(), 0, sensitive, lines.size() + 1, &cs, &most));

    char *d_text = nullptr;
    int *d_ids = nullptr, *d_pos = nullptr;
    const size_t capacity = n * (size_t)most;                               /* never truncates; the device form wants capacity >= size */
    HIP(hipMalloc(reinterpret_cast<void **>(&d_text), n));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_ids), capacity * sizeof(int)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_pos), capacity * sizeof(int)));
    HIP(hipMemcpy(d_text, text.data(), n, hipMemcpyHostToDevice));

    printf("%s\n", text.c_str());
    std::vector<std::vector<int>> got(2);
    for (unsigned int flags : {0u, PFACX_CASE_ALL}) {
        size_t listed = 0;
        CHECK(PFACX_caseMatchFromDevice(cs, d_text, n, flags, d_ids, d_pos, capacity, &listed));
        std::vector<int> ids(listed), pos(listed);
        if (listed) {
            HIP(hipMemcpy(ids.data(), d_ids, listed * sizeof(int), hipMemcpyDeviceToHost));
            HIP(hipMemcpy(pos.data(), d_pos, listed * sizeof(int), hipMemcpyDeviceToHost));
        }
        printf(flags ? "every pattern at each position (PFACX_CASE_ALL):\n" : "the longest pattern at each position, the highest id on a tie:\n");
        for (size_t i = 0; i < listed; i++) {
            printf("%3d  line %d  %-6s %s\n", pos[i], ids[i], lines[(size_t)ids[i] - 1].c_str(), sensitive[ids[i]] ? "exact" : "any case");
            got[flags ? 1 : 0].push_back(pos[i] * 16 + ids[i]);
        }
    }

    /* self-check: the three variants over `GET get gEt Get`, `Host: ` in another case, `AKIA` only as written */
    const std::vector<int> list = {0 * 16 + 3, 4 * 16 + 3, 8 * 16 + 3, 12 * 16 + 3, 16 * 16 + 4, 27 * 16 + 5};
    const std::vector<int> all = {0 * 16 + 3, 0 * 16 + 1, 4 * 16 + 3, 4 * 16 + 2, 8 * 16 + 3, 12 * 16 + 3, 16 * 16 + 4, 27 * 16 + 5};
    if (got[0] != list || got[1] != all || most != 3) {
        fprintf(stderr, "self-check FAILED\n");
        return 1;
    }
    printf("self-check passed\n");

    (void)hipFree(d_text);
    (void)hipFree(d_ids);
    (void)hipFree(d_pos);
    CHECK(PFACX_caseClose(cs));
    CHECK(PFAC_destroy(handle));
    return 0;
}
