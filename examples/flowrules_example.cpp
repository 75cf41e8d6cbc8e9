// flowrules_example.cpp -- rules whose patterns arrive in different packets of a flow (include/pfac_ext.h: PFACX_flowRules*).
// Three flows, their packets interleaved in three batches.  Flow 1 sends `User-Agent:` cut between batch 0 and 1 and `sqlmap` cut between batch
// 1 and 2: the rule {User-Agent:, sqlmap} fires once, in batch 2.  Every batch goes through PFACX_flowsMatchFromDevice, and the ids and
// pieceFirst it leaves on the device go straight into PFACX_flowRulesPairsFromDevice: no pair is copied to the host.  Prints one line per fired
// rule.  With --host the same through a host-only handle and the two host forms.
//
//   make -C examples flowrules_example && ./examples/flowrules_example
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

int main(int argc, char **argv)
{
    const bool onHost = argc > 1 && std::strcmp(argv[1], "--host") == 0;
    const char patterns[] = "User-Agent:\nsqlmap\nGET\nGET /admin\npasswd\n";            // pattern id = line
    const int ruleOff[] = {0, 2, 4, 5};
    const int rulePatterns[] = {1, 2, /**/ 3, 5, /**/ 4};
    const char *ruleNames[] = {"sqlmap scanner", "GET and passwd", "admin page"};
    const size_t numRules = 3, numFlows = 3;
    // one piece per flow and batch
    const std::vector<std::vector<Packet>> batches = {
        {{1, "GET /admin HTTP/1.1\r\nUser-Ag"}, {0, "POST /login\r\nUser-Agent: curl"}},
        {{1, "ent: sql"}, {2, "GET /etc/pas"}},
        {{1, "map/1.7\r\n"}, {2, "swd\r\n"}, {0, " sqlmap"}},
    };

    PFAC_handle_t handle;
    check("PFAC_create", onHost ? PFACX_createHostOnly(&handle) : PFAC_create(&handle));
    check("PFACX_readPatternFromMemory", PFACX_readPatternFromMemory(handle, patterns, std::strlen(patterns)));
    PFACX_info_t info;
    std::memset(&info, 0, sizeof(info));
    info.structSize = sizeof(info);
    check("PFACX_getInfo", PFACX_getInfo(handle, &info));
    const size_t M = (size_t)info.maxPatternLen;
    const size_t room = 256, capacity = room + numFlows * (M - 1);    // >= batch size + pieces * (maxPatternLen - 1)
    const size_t firedCapacity = numFlows * numRules;                 // a (flow, rule) fires once: never more in one call

    // the arrays of both calls: on the device, or (--host) on the host
    std::vector<char> h_input(room);
    std::vector<int> h_ids(capacity), h_pos(capacity), h_first(numFlows + 1), h_firedPiece(firedCapacity), h_firedRule(firedCapacity);
    char *input = h_input.data();
    int *ids = h_ids.data(), *pos = h_pos.data(), *first = h_first.data(), *firedPiece = h_firedPiece.data(), *firedRule = h_firedRule.data();
    if (!onHost) {
        hipCheck("hipMalloc", hipMalloc(reinterpret_cast<void **>(&input), room));
        hipCheck("hipMalloc", hipMalloc(reinterpret_cast<void **>(&ids), capacity * sizeof(int)));
        hipCheck("hipMalloc", hipMalloc(reinterpret_cast<void **>(&pos), capacity * sizeof(int)));
        hipCheck("hipMalloc", hipMalloc(reinterpret_cast<void **>(&first), (numFlows + 1) * sizeof(int)));
        hipCheck("hipMalloc", hipMalloc(reinterpret_cast<void **>(&firedPiece), firedCapacity * sizeof(int)));
        hipCheck("hipMalloc", hipMalloc(reinterpret_cast<void **>(&firedRule), firedCapacity * sizeof(int)));
    }

    PFACX_flows_t flows;
    PFACX_flowRules_t rules;
    check("PFACX_flowsOpen", PFACX_flowsOpen(handle, numFlows, &flows));
    check("PFACX_flowRulesOpen", PFACX_flowRulesOpen(handle, ruleOff, rulePatterns, numRules, numFlows, &rules));

    // the pairs of one flows call (or flush) into the rules, and what fired out
    const auto fire = [&](const char *when, const unsigned int *flowIds, size_t pieces, int count) {
        size_t fired = 0;
        check("PFACX_flowRulesPairs", (onHost ? PFACX_flowRulesPairsFromHost : PFACX_flowRulesPairsFromDevice)(
                                          rules, ids, (size_t)count, first, flowIds, pieces, firedPiece, firedRule, firedCapacity, nullptr, &fired));
        if (!onHost) {
            hipCheck("hipMemcpy", hipMemcpy(h_firedPiece.data(), firedPiece, fired * sizeof(int), hipMemcpyDeviceToHost));
            hipCheck("hipMemcpy", hipMemcpy(h_firedRule.data(), firedRule, fired * sizeof(int), hipMemcpyDeviceToHost));
        }
        for (size_t i = 0; i < fired; i++)
            std::printf("%s, flow %u: rule %d fired (%s)\n", when, flowIds[h_firedPiece[i]], h_firedRule[i], ruleNames[h_firedRule[i]]);
    };

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
        if (onHost) {
            std::memcpy(input, buffer.data(), buffer.size());
            check("PFACX_flowsMatchFromHost", PFACX_flowsMatchFromHost(flows, input, buffer.size(), offsets.data(), flowIds.data(), pieces, ids, pos, capacity,
                                                                        first, pieceOffsets.data(), &count));
        } else {
            hipCheck("hipMemcpy", hipMemcpy(input, buffer.data(), buffer.size(), hipMemcpyHostToDevice));
            check("PFACX_flowsMatchFromDevice", PFACX_flowsMatchFromDevice(flows, input, buffer.size(), offsets.data(), flowIds.data(), pieces, ids, pos,
                                                                            capacity, first, pieceOffsets.data(), &count));
        }
        fire(("batch " + std::to_string(b)).c_str(), flowIds.data(), pieces, count);
    }
    // the end of every flow: what was still pending completes rules too; then the rule state of the flushed flows is reset with them
    const unsigned int all[] = {0, 1, 2};
    int count = 0;
    check("PFACX_flowsFlush", PFACX_flowsFlush(flows, all, numFlows, ids, pos, capacity, first, &count));
    fire("flush", all, numFlows, count);
    check("PFACX_flowRulesReset", PFACX_flowRulesReset(rules, all, numFlows));

    check("PFACX_flowRulesClose", PFACX_flowRulesClose(rules));
    check("PFACX_flowsClose", PFACX_flowsClose(flows));
    if (!onHost) {
        (void)hipFree(input);
        (void)hipFree(ids);
        (void)hipFree(pos);
        (void)hipFree(first);
        (void)hipFree(firedPiece);
        (void)hipFree(firedRule);
    }
    check("PFAC_destroy", PFAC_destroy(handle));
    return 0;
}
