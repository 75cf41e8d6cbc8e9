/*
 * groups_example.cpp -- port groups over a handful of packets on the GPU: one pattern set that holds the strings of the HTTP group, the SMB group
 * and the "any" group, one mask per pattern and per packet, one call (PFACX_groupsMatchFromDevice: the count query with the groups that hit first,
 * then arrays of exactly that length), print the matches of every packet, and check the list against a loop over the packets and the patterns of
 * their groups (include/pfac_ext.h).
 */
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
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
    const unsigned long long HTTP = 1ull << 0, SMB = 1ull << 1, ANY = 1ull << 2;
    struct Pattern { std::string bytes; unsigned long long groups; };
    /* "GET /admin" hides "GET " where both are enabled; "cmd.exe" is on two lines, once for each group that wants it */
    const std::vector<Pattern> patterns = {{"GET ", HTTP}, {"GET /admin", SMB}, {"cmd.exe", HTTP}, {"\\PIPE\\", SMB}, {"cmd.exe", SMB}, {"passwd", ANY}};
    struct Packet { std::string bytes; unsigned long long groups; };
    const std::vector<Packet> packets = {{"GET /admin/passwd HTTP/1.1", HTTP | ANY},           /* port 80 */
                                         {"\\PIPE\\srvsvc cmd.exe GET /admin", SMB | ANY},      /* port 445 */
                                         {"GET /cmd.exe", ANY},                                /* another port: the any group alone */
                                         {"", HTTP | ANY},
                                         {"run cmd.exe, read passwd", HTTP | SMB | ANY}};
    std::string file, input;
    std::vector<unsigned long long> masks = {0};                            /* by pattern id: ids count from 1 */
    for (const Pattern &p : patterns) { file += p.bytes + "\n"; masks.push_back(p.groups); }
    std::vector<size_t> offsets = {0};
    std::vector<unsigned long long> segMasks;
    for (const Packet &p : packets) { input += p.bytes; offsets.push_back(input.size()); segMasks.push_back(p.groups); }
    const size_t n = input.size(), count = packets.size();

    PFAC_handle_t handle = nullptr;
    PFACX_groups_t groups = nullptr;
    CHECK(PFAC_create(&handle));
    CHECK(PFACX_readPatternFromMemory(handle, file.data(), file.size()));
    CHECK(PFACX_groupsOpen(handle, masks.data(), masks.size(), &groups));

    char *d_input = nullptr;
    size_t *d_offsets = nullptr, *d_first = nullptr;
    unsigned long long *d_segMasks = nullptr, *d_hit = nullptr;
    HIP(hipMalloc(reinterpret_cast<void **>(&d_input), n));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_offsets), (count + 1) * sizeof(size_t)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_first), (count + 1) * sizeof(size_t)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_segMasks), count * sizeof(unsigned long long)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_hit), count * sizeof(unsigned long long)));
    HIP(hipMemcpy(d_input, input.data(), n, hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_offsets, offsets.data(), (count + 1) * sizeof(size_t), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_segMasks, segMasks.data(), count * sizeof(unsigned long long), hipMemcpyHostToDevice));

    size_t listed = 0;                                                      /* the count query: how long is the list, which groups hit where? */
    PFAC_status_t st = PFACX_groupsMatchFromDevice(groups, d_input, n, d_offsets, count, d_segMasks, 0, nullptr, nullptr, 0, nullptr, d_hit, &listed);
    if (st != PFAC_STATUS_SUCCESS && st != PFACX_STATUS_OUTPUT_TRUNCATED) CHECK(st);
    int *d_ids = nullptr, *d_pos = nullptr;
    HIP(hipMalloc(reinterpret_cast<void **>(&d_ids), (listed + 1) * sizeof(int)));
    HIP(hipMalloc(reinterpret_cast<void **>(&d_pos), (listed + 1) * sizeof(int)));
    CHECK(PFACX_groupsMatchFromDevice(groups, d_input, n, d_offsets, count, d_segMasks, 0, d_ids, d_pos, listed, d_first, nullptr, &listed));
    std::vector<int> ids(listed), pos(listed);
    std::vector<size_t> first(count + 1);
    std::vector<unsigned long long> hit(count);
    if (listed) {
        HIP(hipMemcpy(ids.data(), d_ids, listed * sizeof(int), hipMemcpyDeviceToHost));
        HIP(hipMemcpy(pos.data(), d_pos, listed * sizeof(int), hipMemcpyDeviceToHost));
    }
    HIP(hipMemcpy(first.data(), d_first, (count + 1) * sizeof(size_t), hipMemcpyDeviceToHost));
    HIP(hipMemcpy(hit.data(), d_hit, count * sizeof(unsigned long long), hipMemcpyDeviceToHost));

    for (size_t k = 0; k < count; k++) {
        printf("packet %zu (groups %llx, hit %llx):", k, segMasks[k], hit[k]);
        for (size_t i = first[k]; i < first[k + 1]; i++) printf(" %d@%zu", ids[i], (size_t)pos[i] - offsets[k]);
        printf("\n");
    }

    /* self-check: per position of every packet the longest pattern of the packet's groups; of equal strings the last line reports, for all of them */
    bool ok = first[0] == 0 && first[count] == listed;
    size_t at = 0;
    for (size_t k = 0; ok && k < count; k++) {
        const std::string &bytes = packets[k].bytes;
        unsigned long long wantHit = 0;
        for (size_t p = 0; ok && p < bytes.size(); p++) {
            int best = 0;
            for (size_t id = 1; id <= patterns.size(); id++) {
                const std::string &s = patterns[id - 1].bytes;
                if (bytes.compare(p, s.size(), s) != 0 || p + s.size() > bytes.size()) continue;
                unsigned long long m = 0;
                int reported = 0;
                for (size_t j = 1; j <= patterns.size(); j++)
                    if (patterns[j - 1].bytes == s) { m |= patterns[j - 1].groups; reported = (int)j; }
                if (!(m & packets[k].groups)) continue;
                wantHit |= m & packets[k].groups;
                if (best == 0 || s.size() > patterns[(size_t)best - 1].bytes.size()) best = reported;
            }
            if (best == 0) continue;
            ok = at < first[k + 1] && at >= first[k] && ids[at] == best && (size_t)pos[at] == offsets[k] + p;
            at++;
        }
        ok = ok && at == first[k + 1] && hit[k] == wantHit;
    }
    if (!ok || at != listed) {
        fprintf(stderr, "self-check FAILED\n");
        return 1;
    }
    printf("self-check passed: %zu matches in %zu packets\n", listed, count);

    (void)hipFree(d_input);
    (void)hipFree(d_offsets);
    (void)hipFree(d_first);
    (void)hipFree(d_segMasks);
    (void)hipFree(d_hit);
    (void)hipFree(d_ids);
    (void)hipFree(d_pos);
    CHECK(PFACX_groupsClose(groups));
    CHECK(PFAC_destroy(handle));
    return 0;
}
