/*
 * gapsig_example.cpp -- signatures with bounded gaps between parts (PFACX_gapsigOpenText / PFACX_gapsigGetAnchors /
 * PFACX_gapsigMatchFromDevice, include/pfac_ext.h): hex signatures of the ClamAV kind with `{n-m}` and `[n-m]` between their parts.  The library
 * picks one fully specified run inside one part of each signature as its anchor, scans for the anchors and searches over the gap widths around
 * every anchor occurrence; the list holds (signature id, start) and the smallest end, every occurrence once.
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
    const std::vector<std::string> lines = {
        "4D 5A {2-6} 50 45 00 00",          /* 1: MZ, two to six bytes, PE\0\0 */
        "E8 ?? ?? ?? ?? [0-8] 5? C3",       /* 2: call rel32; up to eight bytes; pop reg; ret */
        "69 64 3D {1-4} 3B {0-2} 6F 6B",    /* 3: id=, one to four bytes, ;, up to two bytes, ok */
    };
    std::string signatures;
    for (const std::string &l : lines) signatures += l + "\n";
    const char raw[] = "..MZ\x90\x00\x03PE\x00\x00..id=1234; ok.\xe8\x10\x20\x30\x40\x90\x90\x5d\xc3.id=12345;ok.MZ.PE\x00\x00";
    const std::string input(raw, sizeof(raw) - 1);
    const size_t n = input.size();

    PFAC_handle_t handle = nullptr;
    CHECK(PFAC_create(&handle));
    PFACX_gapsig_t sig = nullptr;
    int badLine = 0;
    CHECK(PFACX_gapsigOpenText(handle, signatures.data(), signatures.size(), 0, &sig, &badLine));   /* loads the anchors into the handle */
    const size_t S = lines.size();
    std::vector<int> anchorId(S + 1), anchorPart(S + 1), anchorOff(S + 1), anchorLen(S + 1);
    CHECK(PFACX_gapsigGetAnchors(sig, anchorId.data(), anchorPart.data(), anchorOff.data(), anchorLen.data(), S + 1));
    for (size_t i = 1; i <= S; i++)
        printf("signature %zu  %-30s anchor: pattern %d, part %d, bytes [%d, %d)\n", i, lines[i - 1].c_str(), anchorId[i], anchorPart[i], anchorOff[i],
               anchorOff[i] + anchorLen[i]);

    char *d_input = nullptr;
    int *d_ids = nullptr, *d_pos = nullptr, *d_end = nullptr;
    const size_t capacity = n;                                              /* the device form wants capacity >= size */
    HIP(hipMalloc(reinterpret_cast<void **>(&d_input), n));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_ids), capacity * sizeof(int)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_pos), capacity * sizeof(int)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_end), capacity * sizeof(int)));
    HIP(hipMemcpy(d_input, input.data(), n, hipMemcpyHostToDevice));

    size_t listed = 0;
    CHECK(PFACX_gapsigMatchFromDevice(sig, d_input, n, d_ids, d_pos, d_end, capacity, &listed));
    std::vector<int> ids(listed), pos(listed), end(listed), got;
    if (listed) {
        HIP(hipMemcpy(ids.data(), d_ids, listed * sizeof(int), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(pos.data(), d_pos, listed * sizeof(int), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(end.data(), d_end, listed * sizeof(int), hipMemcpyDeviceToHost));
    }
    printf("occurrences, in the order of their anchors:\n");
    for (size_t i = 0; i < listed; i++) {
        printf("  signature %d covers [%d, %d)\n", ids[i], pos[i], end[i]);
        got.push_back((pos[i] * 64 + end[i]) * 4 + ids[i]);
    }

    /* self-check: the header at 2 with a gap of three (the one at the end has a gap of one), the first rule at 13 (the second has five bytes),
     * the stub at 25 with two bytes in its gap */
    const std::vector<int> want = {(2 * 64 + 11) * 4 + 1, (13 * 64 + 24) * 4 + 3, (25 * 64 + 34) * 4 + 2};
    if (got != want || anchorPart[1] != 1 || anchorLen[1] != 4 || anchorPart[2] != 0 || anchorPart[3] != 0 || anchorLen[3] != 3) {
        fprintf(stderr, "self-check FAILED\n");
        return 1;
    }
    printf("self-check passed\n");

    (void)hipFree(d_input);
    (void)hipFree(d_ids);
    (void)hipFree(d_pos);
    (void)hipFree(d_end);
    CHECK(PFACX_gapsigClose(sig));
    CHECK(PFAC_destroy(handle));
    return 0;
}
