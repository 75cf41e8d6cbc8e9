// flows_example.cpp -- packets of several reassembled flows matched in ONE call per batch (include/pfac_ext.h: PFACX_flows*).
// Three flows, their packets interleaved in two batches; "passwd" of flow 1 is cut after "pas" BETWEEN the batches and is found once,
// at its position in the flow (a batch call without flows would miss it).  Prints one line per match.
//
//   make -C examples flows_example && ./examples/flows_example
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

struct Packet { unsigned int flow; const char *bytes; };

int main()
{
    const char *names[] = {"", "GET", "passwd", "pass", "cmd.exe"};   // pattern id = line
    const char patterns[] = "GET\npasswd\npass\ncmd.exe\n";
    // one piece per flow and batch: packets of one flow that arrive in one batch are laid adjacent and passed as one piece
    const std::vector<std::vector<Packet>> batches = {
        {{1, "GET /etc/pas"}, {0, "POST /a cmd."}, {2, "GET /index"}},
        {{2, ".html pass"}, {1, "swd HTTP/1.1"}, {0, "exe GET"}},
    };
    const size_t numFlows = 3;

    PFAC_handle_t handle;
    check("PFAC_create", PFAC_create(&handle));
    check("PFACX_readPatternFromMemory", PFACX_readPatternFromMemory(handle, patterns, std::strlen(patterns)));
    PFACX_info_t info;
    std::memset(&info, 0, sizeof(info));
    info.structSize = sizeof(info);
    check("PFACX_getInfo", PFACX_getInfo(handle, &info));
    const size_t M = (size_t)info.maxPatternLen;
    const size_t room = 256, capacity = room + numFlows * (M - 1);    // >= batch size + pieces * (maxPatternLen - 1)

    char *d_input = nullptr;
    int *d_ids = nullptr, *d_pos = nullptr, *d_first = nullptr;
    hipCheck("hipMalloc", hipMalloc(reinterpret_cast<void **>(&d_input), room));
    hipCheck("hipMalloc", hipMalloc(reinterpret_cast<void **>(&d_ids), capacity * sizeof(int)));
    hipCheck("hipMalloc", hipMalloc(reinterpret_cast<void **>(&d_pos), capacity * sizeof(int)));
    hipCheck("hipMalloc", hipMalloc(reinterpret_cast<void **>(&d_first), (numFlows + 1) * sizeof(int)));
    std::vector<int> ids(capacity), pos(capacity), first(numFlows + 1);

    PFACX_flows_t flows;
    check("PFACX_flowsOpen", PFACX_flowsOpen(handle, numFlows, &flows));
    for (size_t b = 0; b < batches.size(); b++) {
        std::string buffer;
        std::vector<size_t> offsets(1, 0);
        std::vector<unsigned int> flowIds;
        for (const Packet &p : batches[b]) {
            buffer += p.bytes;
            offsets.push_back(buffer.size());
            flowIds.push_back(p.flow);
        }
        const size_t pieces = flowIds.size();
        std::vector<unsigned long long> pieceOffsets(pieces);
        int count = 0;
        hipCheck("hipMemcpy", hipMemcpy(d_input, buffer.data(), buffer.size(), hipMemcpyHostToDevice));
        check("PFACX_flowsMatchFromDevice", PFACX_flowsMatchFromDevice(flows, d_input, buffer.size(), offsets.data(), flowIds.data(), pieces, d_ids, d_pos,
                                                                        capacity, d_first, pieceOffsets.data(), &count));
        hipCheck("hipMemcpy", hipMemcpy(ids.data(), d_ids, count * sizeof(int), hipMemcpyDeviceToHost));
        hipCheck("hipMemcpy", hipMemcpy(pos.data(), d_pos, count * sizeof(int), hipMemcpyDeviceToHost));
        hipCheck("hipMemcpy", hipMemcpy(first.data(), d_first, (pieces + 1) * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < pieces; k++)
            for (int z = first[k]; z < first[k + 1]; z++)
                std::printf("batch %zu, flow %u: flow position %llu (%d from the piece's first byte): %s\n", b, flowIds[k],
                            pieceOffsets[k] + (long long)pos[z], pos[z], names[ids[z]]);
    }
    // the end of every flow: what was still pending
    const unsigned int all[] = {0, 1, 2};
    int count = 0;
    check("PFACX_flowsFlush", PFACX_flowsFlush(flows, all, numFlows, d_ids, d_pos, capacity, d_first, &count));
    hipCheck("hipMemcpy", hipMemcpy(ids.data(), d_ids, count * sizeof(int), hipMemcpyDeviceToHost));
    hipCheck("hipMemcpy", hipMemcpy(pos.data(), d_pos, count * sizeof(int), hipMemcpyDeviceToHost));
    hipCheck("hipMemcpy", hipMemcpy(first.data(), d_first, (numFlows + 1) * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < numFlows; k++)
        for (int z = first[k]; z < first[k + 1]; z++)
            std::printf("flush, flow %u: %d from the flow's end: %s\n", all[k], pos[z], names[ids[z]]);

    check("PFACX_flowsClose", PFACX_flowsClose(flows));
    (void)hipFree(d_input);
    (void)hipFree(d_ids);
    (void)hipFree(d_pos);
    (void)hipFree(d_first);
    check("PFAC_destroy", PFAC_destroy(handle));
    return 0;
}
