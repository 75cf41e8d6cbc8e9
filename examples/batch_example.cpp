/*
 * batch_example.cpp -- many independent packets in one call (include/pfac_ext.h: PFACX_matchBatch*).
 *
 * A capture of packets is one buffer: a pcap-like record header (16 bytes: seconds, microseconds, captured length, original
 * length) in front of every packet's bytes.  The payloads are copied into one contiguous buffer and cut by an offsets array,
 * so that no match runs from the end of one packet into the next.  The program matches the whole capture with one device call,
 * checks it against one PFAC_matchFromDevice call per packet, and prints the matches per packet from the compacted form.
 *
 *     make -C examples && ./examples/batch_example [pattern_file]
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "PFAC.h"
#include "pfac_ext.h"

#define CHECK(call)                                                                             \
    do {                                                                                        \
        PFAC_status_t st_ = (call);                                                             \
        if (st_ != PFAC_STATUS_SUCCESS) {                                                       \
            std::fprintf(stderr, "%s failed: %s\n", #call, PFAC_getErrorString(st_));           \
            return 1;                                                                           \
        }                                                                                       \
    } while (0)
#define HIP_CHECK(call)                                                                         \
    do {                                                                                        \
        if ((call) != hipSuccess) { std::fprintf(stderr, "%s failed\n", #call); return 1; }     \
    } while (0)

struct RecordHeader { uint32_t sec, usec, capLen, origLen; };

/* a small capture: request lines whose patterns would straddle packets if the payloads were matched as one stream */
static std::vector<unsigned char> makeCapture(int packets)
{
    const char *payloads[] = {"GET /index.html HTTP/1.1\r\nHost: example.com\r\n\r\nGET /", "admin.php HTTP/1.1\r\n\r\n",
                              "POST /login HTTP/1.1\r\nContent-Length: 9\r\n\r\nuser=root", "HTTP/1.1 200 OK\r\n\r\n<html>", ""};
    std::vector<unsigned char> cap;
    for (int i = 0; i < packets; i++) {
        const std::string p = payloads[i % 5];
        const RecordHeader h = {1700000000u + (uint32_t)i, 0, (uint32_t)p.size(), (uint32_t)p.size()};
        const unsigned char *hb = reinterpret_cast<const unsigned char *>(&h);
        cap.insert(cap.end(), hb, hb + sizeof(h));
        cap.insert(cap.end(), p.begin(), p.end());
    }
    return cap;
}

int main(int argc, char **argv)
{
    const char *patternFile = argc > 1 ? argv[1] : nullptr;
    const std::string defaultPatterns = "GET /admin\nGET /\nadmin.php\nroot\n<html>\nHTTP/1.1 200\n";

    /* the capture's payloads, back to back, and where each packet starts */
    const std::vector<unsigned char> capture = makeCapture(1000);
    std::vector<char> payload;
    std::vector<size_t> offsets(1, 0);
    for (size_t at = 0; at + sizeof(RecordHeader) <= capture.size();) {
        RecordHeader h;
        std::memcpy(&h, &capture[at], sizeof(h));
        at += sizeof(h);
        payload.insert(payload.end(), capture.begin() + (long)at, capture.begin() + (long)(at + h.capLen));
        at += h.capLen;
        offsets.push_back(payload.size());
    }
    const size_t n = payload.size(), packets = offsets.size() - 1;

    PFAC_handle_t handle;
    CHECK(PFAC_create(&handle));
    if (patternFile) CHECK(PFAC_readPatternFromFile(handle, const_cast<char *>(patternFile)));
    else CHECK(PFACX_readPatternFromMemory(handle, defaultPatterns.data(), defaultPatterns.size()));

    char *d_in = nullptr;
    size_t *d_offsets = nullptr;
    int *d_result = nullptr, *d_single = nullptr, *d_pos = nullptr, *d_segFirst = nullptr;
    HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d_in), n));
    HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d_offsets), offsets.size() * sizeof(size_t)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d_result), n * sizeof(int)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d_single), n * sizeof(int)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d_pos), n * sizeof(int)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d_segFirst), offsets.size() * sizeof(int)));
    HIP_CHECK(hipMemcpy(d_in, payload.data(), n, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_offsets, offsets.data(), offsets.size() * sizeof(size_t), hipMemcpyHostToDevice));

    /* one call for the whole capture ... */
    CHECK(PFACX_matchBatchFromDevice(handle, d_in, n, d_offsets, packets, d_result));
    /* ... against one call per packet */
    for (size_t k = 0; k < packets; k++)
        if (offsets[k + 1] > offsets[k])
            CHECK(PFAC_matchFromDevice(handle, d_in + offsets[k], offsets[k + 1] - offsets[k], d_single + offsets[k]));
    std::vector<int> batch(n), single(n);
    HIP_CHECK(hipMemcpy(batch.data(), d_result, n * sizeof(int), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(single.data(), d_single, n * sizeof(int), hipMemcpyDeviceToHost));
    size_t differ = 0, matches = 0;
    for (size_t i = 0; i < n; i++) { differ += batch[i] != single[i]; matches += batch[i] != 0; }

    /* the compacted form: (id, position) pairs, and where each packet's pairs begin */
    int pairs = 0;
    CHECK(PFACX_matchBatchFromDeviceReduce(handle, d_in, n, d_offsets, packets, d_result, d_pos, d_segFirst, &pairs));
    std::vector<int> ids((size_t)pairs), pos((size_t)pairs), first(offsets.size());
    if (pairs) {
        HIP_CHECK(hipMemcpy(ids.data(), d_result, (size_t)pairs * sizeof(int), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(pos.data(), d_pos, (size_t)pairs * sizeof(int), hipMemcpyDeviceToHost));
    }
    HIP_CHECK(hipMemcpy(first.data(), d_segFirst, first.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < 5 && k < packets; k++) {
        std::printf("packet %zu (%zu bytes):", k, offsets[k + 1] - offsets[k]);
        for (int j = first[k]; j < first[k + 1]; j++) std::printf(" id %d at %zu", ids[(size_t)j], (size_t)pos[(size_t)j] - offsets[k]);
        std::printf("\n");
    }
    std::printf("%zu packets, %zu bytes: %zu matches (%d pairs), %zu positions differ from one call per packet\n", packets, n, matches, pairs,
                differ);

    (void)hipFree(d_in); (void)hipFree(d_offsets); (void)hipFree(d_result); (void)hipFree(d_single); (void)hipFree(d_pos);
    (void)hipFree(d_segFirst);
    PFAC_destroy(handle);
    return differ == 0 && (size_t)pairs == matches ? 0 : 1;
}
