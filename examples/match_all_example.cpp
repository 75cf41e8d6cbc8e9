// match_all_example.cpp -- every pattern at a position, not only the longest (include/pfac_ext.h: PFACX_matchAll*).
// Two rules whose patterns nest: rule A "GET" and rule B "GET /admin".  The longest-match calls report B alone at
// position 0; PFACX_matchAllFromDevice reports B and then A there.  Prints one line per (position, rule).
//
//   make -C examples match_all_example && ./examples/match_all_example
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "PFAC.h"
#include "pfac_ext.h"

static void check(const char *what, PFAC_status_t st)
{
    if (st == PFAC_STATUS_SUCCESS) return;
    std::fprintf(stderr, "%s: %s\n", what, PFAC_getErrorString(st));
    std::exit(1);
}

static void hipCheck(const char *what, hipError_t e)
{
    if (e == hipSuccess) return;
    std::fprintf(stderr, "%s: %s\n", what, hipGetErrorString(e));
    std::exit(1);
}

int main()
{
    const char *rules[] = {"", "rule A (GET)", "rule B (GET /admin)"};      // pattern id 1 = line 1, id 2 = line 2
    const char patterns[] = "GET\nGET /admin\n";
    const char input[] = "GET /admin HTTP/1.1\r\nHost: example\r\n\r\nGET /index.html";
    const size_t n = std::strlen(input);

    PFAC_handle_t handle;
    check("PFAC_create", PFAC_create(&handle));
    check("PFACX_readPatternFromMemory", PFACX_readPatternFromMemory(handle, patterns, std::strlen(patterns)));
    PFACX_info_t info;
    std::memset(&info, 0, sizeof(info));
    info.structSize = sizeof(info);
    check("PFACX_getInfo", PFACX_getInfo(handle, &info));
    const size_t capacity = n * (size_t)info.maxMatchesPerPosition;     // never truncates

    char *d_input = nullptr;
    int *d_ids = nullptr, *d_pos = nullptr;
    hipCheck("hipMalloc", hipMalloc(reinterpret_cast<void **>(&d_input), n));
    hipCheck("hipMalloc", hipMalloc(reinterpret_cast<void **>(&d_ids), capacity * sizeof(int)));
    hipCheck("hipMalloc", hipMalloc(reinterpret_cast<void **>(&d_pos), capacity * sizeof(int)));
    hipCheck("hipMemcpy", hipMemcpy(d_input, input, n, hipMemcpyHostToDevice));

    size_t count = 0;
    check("PFACX_matchAllFromDevice", PFACX_matchAllFromDevice(handle, d_input, n, d_ids, d_pos, capacity, &count));
    std::vector<int> ids(count), pos(count);
    hipCheck("hipMemcpy", hipMemcpy(ids.data(), d_ids, count * sizeof(int), hipMemcpyDeviceToHost));
    hipCheck("hipMemcpy", hipMemcpy(pos.data(), d_pos, count * sizeof(int), hipMemcpyDeviceToHost));
    std::printf("maxMatchesPerPosition = %d, number of matches = %zu\n", info.maxMatchesPerPosition, count);
    for (size_t i = 0; i < count; i++) std::printf("position %d: %s\n", pos[i], rules[ids[i]]);

    (void)hipFree(d_input);
    (void)hipFree(d_ids);
    (void)hipFree(d_pos);
    check("PFAC_destroy", PFAC_destroy(handle));
    return 0;
}
