/*
 * sig_example.cpp -- masked byte signatures with wildcards (PFACX_sigOpenText / PFACX_sigGetAnchors / PFACX_sigMatchFromDevice,
 * include/pfac_ext.h): hex signatures of the ClamAV kind next to a text rule.  The library picks one fully specified run of each signature as
 * its anchor, scans for the anchors and verifies every signature around every anchor occurrence; the list holds (signature id, start).
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
        "4D 5A ?? ?? 50 45 00 00",          /* 1: MZ, any two bytes, PE\0\0 */
        "E8 ?? ?? ?? ?? 5? C3",             /* 2: call rel32; pop reg; ret */
        "69 64 3D ?? ?? ?? ?? 3B",          /* 3: id=, any four bytes, ; */
    };
    std::string signatures;
    for (const std::string &l : lines) signatures += l + "\n";
    const char raw[] = "..MZ\x90\x00PE\x00\x00..id=1234;.\xe8\x10\x20\x30\x40\x5d\xc3.id=12345;.\xe8\x10\x20\x30\x40\x6d\xc3";
    const std::string input(raw, sizeof(raw) - 1);
    const size_t n = input.size();

    PFAC_handle_t handle = nullptr;
    CHECK(PFAC_create(&handle));
    PFACX_sig_t sig = nullptr;
    int badLine = 0;
    CHECK(PFACX_sigOpenText(handle, signatures.data(), signatures.size(), 0, &sig, &badLine));   /* loads the anchors into the handle */
    std::vector<int> anchorId(lines.size() + 1), anchorOff(lines.size() + 1), anchorLen(lines.size() + 1);
    CHECK(PFACX_sigGetAnchors(sig, anchorId.data(), anchorOff.data(), anchorLen.data(), lines.size() + 1));
    for (size_t i = 1; i <= lines.size(); i++)
        printf("signature %zu  %-26s anchor: pattern %d, bytes [%d, %d)\n", i, lines[i - 1].c_str(), anchorId[i], anchorOff[i], anchorOff[i] + anchorLen[i]);

    char *d_input = nullptr;
    int *d_ids = nullptr, *d_pos = nullptr;
    const size_t capacity = n;                                              /* the device form wants capacity >= size */
    HIP(hipMalloc(reinterpret_cast<void **>(&d_input), n));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_ids), capacity * sizeof(int)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_pos), capacity * sizeof(int)));
    HIP(hipMemcpy(d_input, input.data(), n, hipMemcpyHostToDevice));

    size_t listed = 0;
    CHECK(PFACX_sigMatchFromDevice(sig, d_input, n, d_ids, d_pos, capacity, &listed));
    std::vector<int> ids(listed), pos(listed), got;
    if (listed) {
        HIP(hipMemcpy(ids.data(), d_ids, listed * sizeof(int), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(pos.data(), d_pos, listed * sizeof(int), hipMemcpyDeviceToHost));
    }
    printf("occurrences, in the order of their anchors:\n");
    for (size_t i = 0; i < listed; i++) {
        printf("  signature %d starts at %d\n", ids[i], pos[i]);
        got.push_back(pos[i] * 16 + ids[i]);
    }

    /* self-check: the header at 2, the first rule at 12 (the second one has five bytes), the first stub at 21 (the second pops nothing) */
    const std::vector<int> want = {2 * 16 + 1, 12 * 16 + 3, 21 * 16 + 2};
    if (got != want || anchorOff[1] != 4 || anchorLen[1] != 4 || anchorOff[2] != 0 || anchorLen[3] != 3) {
        fprintf(stderr, "self-check FAILED\n");
        return 1;
    }
    printf("self-check passed\n");

    (void)hipFree(d_input);
    (void)hipFree(d_ids);
    (void)hipFree(d_pos);
    CHECK(PFACX_sigClose(sig));
    CHECK(PFAC_destroy(handle));
    return 0;
}
