// stream_example.cpp -- input that arrives in pieces (include/pfac_ext.h: PFACX_stream*), as a reassembled TCP flow does.
// The pattern "passwd" straddles the two pieces; the stream finds it once, at its position in the flow.  One plain call per
// piece would miss it.  Prints one line per match.
//
//   make -C examples stream_example && ./examples/stream_example
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

static void report(const char *call, const std::vector<int> &ids, const std::vector<int> &pos, int count, unsigned long long base, const char *const *names)
{
    for (int k = 0; k < count; k++)
        std::printf("%s: stream position %llu (%d from the piece's first byte): %s\n", call, base + (long long)pos[k], pos[k], names[ids[k]]);
}

int main()
{
    const char *names[] = {"", "GET", "passwd", "pass"};             // pattern id = line
    const char patterns[] = "GET\npasswd\npass\n";
    const char *pieces[] = {"GET /etc/pas", "swd HTTP/1.1 pass"};      // "passwd" is cut after "pas"

    PFAC_handle_t handle;
    check("PFAC_create", PFAC_create(&handle));
    check("PFACX_readPatternFromMemory", PFACX_readPatternFromMemory(handle, patterns, std::strlen(patterns)));
    PFACX_info_t info;
    std::memset(&info, 0, sizeof(info));
    info.structSize = sizeof(info);
    check("PFACX_getInfo", PFACX_getInfo(handle, &info));
    const size_t capacity = 64 + (size_t)info.maxPatternLen;          // >= piece size + maxPatternLen

    char *d_piece = nullptr;
    int *d_ids = nullptr, *d_pos = nullptr;
    hipCheck("hipMalloc", hipMalloc(reinterpret_cast<void **>(&d_piece), 64));
    hipCheck("hipMalloc", hipMalloc(reinterpret_cast<void **>(&d_ids), capacity * sizeof(int)));
    hipCheck("hipMalloc", hipMalloc(reinterpret_cast<void **>(&d_pos), capacity * sizeof(int)));
    std::vector<int> ids(capacity), pos(capacity);

    PFACX_stream_t stream;
    check("PFACX_streamOpen", PFACX_streamOpen(handle, &stream));
    unsigned long long total = 0;
    int found = 0;
    for (const char *piece : pieces) {
        const size_t n = std::strlen(piece);
        int count = 0;
        unsigned long long offset = 0;
        hipCheck("hipMemcpy", hipMemcpy(d_piece, piece, n, hipMemcpyHostToDevice));
        check("PFACX_streamMatchFromDevice", PFACX_streamMatchFromDevice(stream, d_piece, n, d_ids, d_pos, capacity, &count, &offset));
        hipCheck("hipMemcpy", hipMemcpy(ids.data(), d_ids, count * sizeof(int), hipMemcpyDeviceToHost));
        hipCheck("hipMemcpy", hipMemcpy(pos.data(), d_pos, count * sizeof(int), hipMemcpyDeviceToHost));
        report("piece", ids, pos, count, offset, names);
        total = offset + n;
        found += count;
    }
    int count = 0;
    check("PFACX_streamFlush", PFACX_streamFlush(stream, d_ids, d_pos, capacity, &count));      // the end of the flow
    hipCheck("hipMemcpy", hipMemcpy(ids.data(), d_ids, count * sizeof(int), hipMemcpyDeviceToHost));
    hipCheck("hipMemcpy", hipMemcpy(pos.data(), d_pos, count * sizeof(int), hipMemcpyDeviceToHost));
    report("flush", ids, pos, count, total, names);
    found += count;
    std::printf("%d matches in %llu bytes\n", found, total);

    check("PFACX_streamClose", PFACX_streamClose(stream));
    (void)hipFree(d_piece);
    (void)hipFree(d_ids);
    (void)hipFree(d_pos);
    check("PFAC_destroy", PFAC_destroy(handle));
    return found == 3 ? 0 : 1;
}
