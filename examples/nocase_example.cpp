// nocase_example.cpp -- a caseless pattern set (include/pfac_ext.h: PFACX_READ_NOCASE), as Snort's `nocase` or grep -iF.
// The rules are written in any case; the input is matched whatever its case, on the GPU, and is left as it was.  Prints one
// line per match and the input afterwards.
//
//   make -C examples nocase_example && ./examples/nocase_example
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
    const char *rules[] = {"", "rule 1 (select)", "rule 2 (Union Select)", "rule 3 (/ETC/passwd)"};   // pattern id = line
    const char patterns[] = "select\nUnion Select\n/ETC/passwd\n";
    const char input[] = "GET /?q=1 UNION SELECT pw FROM users; cat /etc/PASSWD; SeLeCt";
    const size_t n = std::strlen(input);

    PFAC_handle_t handle;
    check("PFAC_create", PFAC_create(&handle));
    check("PFACX_readPatternFromMemoryEx", PFACX_readPatternFromMemoryEx(handle, patterns, std::strlen(patterns), PFACX_READ_NOCASE));
    PFACX_info_t info;
    std::memset(&info, 0, sizeof(info));
    info.structSize = sizeof(info);
    check("PFACX_getInfo", PFACX_getInfo(handle, &info));

    char *d_input = nullptr;
    int *d_result = nullptr;
    hipCheck("hipMalloc", hipMalloc(reinterpret_cast<void **>(&d_input), n));
    hipCheck("hipMalloc", hipMalloc(reinterpret_cast<void **>(&d_result), n * sizeof(int)));
    hipCheck("hipMemcpy", hipMemcpy(d_input, input, n, hipMemcpyHostToDevice));
    check("PFAC_matchFromDevice", PFAC_matchFromDevice(handle, d_input, n, d_result));

    std::vector<int> result(n);
    std::vector<char> after(n + 1, 0);
    hipCheck("hipMemcpy", hipMemcpy(result.data(), d_result, n * sizeof(int), hipMemcpyDeviceToHost));
    hipCheck("hipMemcpy", hipMemcpy(after.data(), d_input, n, hipMemcpyDeviceToHost));
    std::printf("caseInsensitive = %d\n", info.caseInsensitive);
    for (size_t i = 0; i < n; i++)
        if (result[i] > 0) std::printf("position %zu: %s\n", i, rules[result[i]]);
    std::printf("input after the call: %s\n", after.data());

    (void)hipFree(d_input);
    (void)hipFree(d_result);
    check("PFAC_destroy", PFAC_destroy(handle));
    return 0;
}
