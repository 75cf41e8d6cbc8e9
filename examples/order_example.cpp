/*
 * order_example.cpp -- from token rules to `line:column rule` without sorting on the host (PFACX_clsigOpenText / PFACX_clsigMatchFromDevice /
 * PFACX_orderHitsFromDevice / PFACX_locatePairsFromDevice, include/pfac_ext.h).  The class-signature call lists (rule, start, end) by owning
 * anchor, not by start; the locate call wants positions non-decreasing; the order call in between permutes the three columns in place.  Without
 * a device the three host forms do the same.
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
    const std::string rules =
        "[a-z0-9=]{2,12}@corp\n"                                 /* 1: a mail name: it starts up to 12 bytes in front of its anchor `@corp` */
        "(?<![0-9])[0-9]{3}-[0-9]{2}-[0-9]{4}(?![0-9])\n"        /* 2: a social security number */
        "id=[0-9]{1,6}\n";                                       /* 3: an id */
    std::string text =
        "from bob@corp id=7\n"
        "ssn 123-45-6789 to xid=4al@corp\n"
        "nothing here\n"
        "id=9001 carol@corp 987-65-4321\n";
    const size_t n = text.size();

    int devices = 0;
    const bool gpu = hipGetDeviceCount(&devices) == hipSuccess && devices > 0;
    PFAC_handle_t handle = nullptr;
    if (gpu) CHECK(PFAC_create(&handle));
    else CHECK(PFACX_createHostOnly(&handle));
    PFACX_clsig_t sig = nullptr;
    int badLine = 0;
    CHECK(PFACX_clsigOpenText(handle, rules.data(), rules.size(), 0, 0, &sig, &badLine));

    size_t listed = 0;
    int wasOrdered = -1;
    std::vector<int> ids(n), pos(n), end(n), record(n), column(n);
    if (gpu) {
        char *d_text = nullptr;
        int *d_ids = nullptr, *d_pos = nullptr, *d_end = nullptr, *d_record = nullptr, *d_column = nullptr;
        HIP(hipMalloc(reinterpret_cast<void **>(&d_text), n));
        for (int **p : {&d_ids, &d_pos, &d_end, &d_record, &d_column}) HIP(hipMalloc(reinterpret_cast<void **>(p), n * sizeof(int)));
        HIP(hipMemcpy(d_text, text.data(), n, hipMemcpyHostToDevice));
        CHECK(PFACX_clsigMatchFromDevice(sig, d_text, n, d_ids, d_pos, d_end, n, &listed));
        /* by start, rules of one start by id; the three columns move together */
        CHECK(PFACX_orderHitsFromDevice(handle, d_pos, d_ids, d_end, nullptr, listed, PFACX_ORDER_TIES_BY_ID, nullptr, &wasOrdered));
        CHECK(PFACX_locatePairsFromDevice(handle, d_text, n, nullptr, 0, d_pos, listed, d_record, d_column, nullptr));
        const size_t bytes = listed * sizeof(int);
        if (listed) {
            HIP(hipMemcpy(ids.data(), d_ids, bytes, hipMemcpyDeviceToHost));
            HIP(hipMemcpy(pos.data(), d_pos, bytes, hipMemcpyDeviceToHost));
            HIP(hipMemcpy(end.data(), d_end, bytes, hipMemcpyDeviceToHost));
            HIP(hipMemcpy(record.data(), d_record, bytes, hipMemcpyDeviceToHost));
            HIP(hipMemcpy(column.data(), d_column, bytes, hipMemcpyDeviceToHost));
        }
        for (void *p : {(void *)d_text, (void *)d_ids, (void *)d_pos, (void *)d_end, (void *)d_record, (void *)d_column}) (void)hipFree(p);
    } else {
        CHECK(PFAC_setPlatform(handle, PFAC_PLATFORM_CPU));
        CHECK(PFACX_clsigMatchFromHost(sig, &text[0], n, ids.data(), pos.data(), end.data(), n, &listed));
        CHECK(PFACX_orderHitsFromHost(handle, pos.data(), ids.data(), end.data(), nullptr, listed, PFACX_ORDER_TIES_BY_ID, nullptr, &wasOrdered));
        CHECK(PFACX_locatePairsFromHost(handle, text.data(), n, nullptr, 0, pos.data(), listed, record.data(), column.data(), nullptr));
    }

    std::string got;
    for (size_t k = 0; k < listed; k++) {
        char line[160];
        snprintf(line, sizeof line, "%d:%d rule %d %.*s\n", record[k] + 1, column[k] + 1, ids[k], end[k] - pos[k], text.c_str() + pos[k]);
        got += line;
    }
    printf("%s%zu hits, the list was %s in start order (%s forms)\n", got.c_str(), listed, wasOrdered ? "already" : "not", gpu ? "device" : "host");

    /* self-check: every start of a mail name is a hit (the largest end each), so `bob@corp` lists `bob` and `ob`; `id=4` is listed in front of
     * `xid=4al@corp` by its anchor and comes out behind it, and behind rule 1 at its own start */
    const std::string want =
        "1:6 rule 1 bob@corp\n1:7 rule 1 ob@corp\n1:15 rule 3 id=7\n"
        "2:5 rule 2 123-45-6789\n2:20 rule 1 xid=4al@corp\n2:21 rule 1 id=4al@corp\n2:21 rule 3 id=4\n2:22 rule 1 d=4al@corp\n2:23 rule 1 =4al@corp\n"
        "2:24 rule 1 4al@corp\n2:25 rule 1 al@corp\n"
        "4:1 rule 3 id=9001\n4:9 rule 1 carol@corp\n4:10 rule 1 arol@corp\n4:11 rule 1 rol@corp\n4:12 rule 1 ol@corp\n4:20 rule 2 987-65-4321\n";
    if (got != want || wasOrdered != 0) {
        fprintf(stderr, "self-check FAILED\n");
        return 1;
    }
    printf("self-check passed\n");
    CHECK(PFACX_clsigClose(sig));
    CHECK(PFAC_destroy(handle));
    return 0;
}
