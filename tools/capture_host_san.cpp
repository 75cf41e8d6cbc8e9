/*
 * capture_host_san.cpp -- PFACX_capturePairsFromHost and PFACX_matchCapturedFromHost under AddressSanitizer and UBSan (make -C pfac_amd/csrc san; run
 * build/capture_host_san: no arguments).
 *
 * The texts of tests/capture_ref.py's table and a few hundred random ones under several class pairs and windows, with and without
 * PFACX_CAPTURE_AT_POS, with sorted lists (duplicates, both ends outside the input, ids the set does not have) and lists that are not sorted at all;
 * the input, the ids, the positions and both outputs in heap blocks of exactly their size: a read past the input's or the list's end or a write past
 * an output's is a report.  Every entry is checked against a loop that states the six rules once more; the scan form at every capCapacity from 0 to
 * the count + 1.
 */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pfac_ext.h"

static bool inClass(const unsigned int *cls, unsigned char b) { return (cls[b >> 5] >> (b & 31u)) & 1u; }

static void classOf(const std::string &members, unsigned int *cls)
{
    std::memset(cls, 0, 8 * sizeof(unsigned int));
    for (unsigned char b : members) cls[b >> 5] |= 1u << (b & 31u);
}

static const std::vector<std::string> kKeys = {"Host:", "user=", "x=", "k="};                    /* ids 1 .. 4 */

/* the six rules of include/pfac_ext.h, byte by byte */
static void reference(const std::string &in, const unsigned int *skip, const unsigned int *stop, size_t window, unsigned int flags, int id, int p,
                      int *valStart, int *valLen)
{
    const size_t n = in.size();
    *valStart = -1;
    *valLen = 0;
    if (p < 0 || (size_t)p >= n) return;
    size_t b = (size_t)p;
    if (!(flags & PFACX_CAPTURE_AT_POS)) {
        if (id < 1 || (size_t)id > kKeys.size()) return;
        b += kKeys[(size_t)id - 1].size();
    }
    if (b > n) b = n;
    const size_t w = window == 0 || window > n - b ? n : b + window;
    size_t s = b;
    while (s < w && inClass(skip, (unsigned char)in[s]) && !inClass(stop, (unsigned char)in[s])) s++;
    size_t e = s;
    while (e < w && !inClass(stop, (unsigned char)in[e])) e++;
    *valStart = (int)s;
    *valLen = (int)(e - s);
}

static int failures = 0;

template <class T>
static T *exactly(const std::vector<T> &v)                                                      /* a heap block of exactly v's bytes */
{
    T *p = static_cast<T *>(std::malloc(v.size() ? v.size() * sizeof(T) : 1));
    if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

struct Classes { const char *skip; size_t skipSize; const char *stop; size_t stopSize; bool nullSkip, nullStop; };

static void run(PFAC_handle_t handle, const std::string &text, const Classes &c, const std::vector<int> &idList, const std::vector<int> &posList)
{
    unsigned int skip[8], stop[8];
    classOf(std::string(c.skip, c.skipSize), skip);
    classOf(std::string(c.stop, c.stopSize), stop);
    const size_t windows[] = {0, 1, 3, text.size(), text.size() + 9, (size_t)-1};
    for (unsigned int flags = 0; flags < 2; flags++) {
        for (size_t window : windows) {
            char *in = exactly(std::vector<char>(text.begin(), text.end()));
            int *ids = flags ? nullptr : exactly(idList), *pos = exactly(posList);
            int *valStart = exactly(std::vector<int>(posList.size(), -7)), *valLen = exactly(std::vector<int>(posList.size(), -7));
            const PFAC_status_t st = PFACX_capturePairsFromHost(handle, in, text.size(), c.nullSkip ? nullptr : skip, c.nullStop ? nullptr : stop, window,
                                                                flags, ids, pos, posList.size(), valStart, valLen);
            bool ok = st == PFAC_STATUS_SUCCESS;
            for (size_t k = 0; ok && !text.empty() && k < posList.size(); k++) {
                int s, l;
                reference(text, skip, stop, window, flags, idList[k], posList[k], &s, &l);
                ok = valStart[k] == s && valLen[k] == l;
            }
            for (size_t k = 0; ok && text.empty() && k < posList.size(); k++) ok = valStart[k] == -7 && valLen[k] == -7;   /* size == 0: nothing is touched */
            if (!ok) {
                failures++;
                fprintf(stderr, "MISMATCH: %zu bytes, %zu pairs, flags %u, window %zu: status %d\n", text.size(), posList.size(), flags, window, (int)st);
            }
            std::free(in); std::free(ids); std::free(pos); std::free(valStart); std::free(valLen);
        }
    }
}

/* the scan form: ids and positions of `size` entries, valStart and valLen of exactly capCapacity */
static void runScan(PFAC_handle_t handle, const std::string &text)
{
    const size_t n = text.size();
    char *in = exactly(std::vector<char>(text.begin(), text.end()));
    int *ids = exactly(std::vector<int>(n, 0)), *pos = exactly(std::vector<int>(n, 0));
    int count = -1;
    if (PFAC_matchFromHostReduce(handle, in, n, ids, pos, &count) != PFAC_STATUS_SUCCESS) failures++;
    unsigned int skip[8], stop[8];
    classOf(" \t", skip);
    classOf("\r\n", stop);
    for (size_t capacity = 0; capacity <= (size_t)count + 1; capacity++) {
        int *ids2 = exactly(std::vector<int>(n, 0)), *pos2 = exactly(std::vector<int>(n, 0));
        int *valStart = exactly(std::vector<int>(capacity, -7)), *valLen = exactly(std::vector<int>(capacity, -7));
        int found = -1;
        const PFAC_status_t st = PFACX_matchCapturedFromHost(handle, in, n, skip, stop, 0, 0, ids2, pos2, capacity ? valStart : nullptr,
                                                             capacity ? valLen : nullptr, capacity, &found);
        bool ok = found == count && st == (capacity >= (size_t)count ? PFAC_STATUS_SUCCESS : PFACX_STATUS_OUTPUT_TRUNCATED);
        for (size_t k = 0; ok && k < capacity; k++) {
            int s = -7, l = -7;
            if (k < (size_t)count) reference(text, skip, stop, 0, 0, ids[k], pos[k], &s, &l);
            ok = valStart[k] == s && valLen[k] == l && (k >= (size_t)count || (ids2[k] == ids[k] && pos2[k] == pos[k]));
        }
        if (!ok) {
            failures++;
            fprintf(stderr, "MISMATCH: the scan form at capCapacity %zu: status %d, %d pairs (want %d)\n", capacity, (int)st, found, count);
        }
        std::free(ids2); std::free(pos2); std::free(valStart); std::free(valLen);
    }
    std::free(in); std::free(ids); std::free(pos);
}

int main()
{
    PFAC_handle_t handle = nullptr;
    if (PFACX_createHostOnly(&handle) != PFAC_STATUS_SUCCESS) return 2;
    std::string patterns;
    for (const std::string &k : kKeys) patterns += k + "\n";
    if (PFACX_readPatternFromMemory(handle, patterns.data(), patterns.size()) != PFAC_STATUS_SUCCESS) return 2;
    unsigned int seed = 20261020u;
    const auto next = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    std::string every;
    for (int b = 0; b < 256; b++) every.push_back((char)b);
    const Classes classes[] = {
        {"", 0, "\n", 1, true, true}, {" \t", 2, "\r\n", 2, false, false}, {" ", 1, ";", 1, false, false}, {" \n", 2, "\n", 1, false, false},
        {every.data(), 256, "", 0, false, false}, {"", 0, "", 0, false, false}, {"ab", 2, every.data() + 56, 200, false, false},
    };
    const auto lists = [&](const std::string &text) {
        const int n = (int)text.size();
        std::vector<int> ids, pos, wild;
        for (int k = 0; k < n + n / 2 + 3; k++) {
            pos.push_back((int)(next() % (unsigned int)(n + 6)) - 3);                           /* duplicates, both ends outside */
            ids.push_back((int)(next() % 7u) - 1);                                              /* -1, 0 and F + 1 among them */
        }
        wild = pos;
        wild.push_back(-2147483647 - 1);
        wild.push_back(2147483647);
        std::sort(pos.begin(), pos.end());
        std::vector<int> wildIds = ids;
        wildIds.push_back(2147483647);
        wildIds.push_back(-2147483647 - 1);
        for (const Classes &c : classes) {
            run(handle, text, c, ids, pos);
            run(handle, text, c, wildIds, wild);
            run(handle, text, c, {}, {});
        }
    };
    const std::string table[] = {"", "x", "\n", "ab", "Host: a.b\r\nuser=bob\nx=  \n k=v", "abc=1;ab=2;", "abcdefgh\n"};
    size_t cases = 0;
    for (const std::string &t : table) {
        lists(t);
        cases++;
    }
    for (int round = 0; round < 300; round++) {
        const size_t n = next() % 90;
        std::string text;
        for (size_t k = 0; k < n; k++) text.push_back(round % 3 == 2 ? (char)next() : "ab \t\n;;x\r="[next() % 10]);
        lists(text);
        cases++;
    }
    runScan(handle, "GET / HTTP/1.1\r\nHost:   example.org\r\nuser= bob \nk=\r\nx=last");
    runScan(handle, "no key in this line");
    PFAC_destroy(handle);
    if (failures) {
        fprintf(stderr, "%d mismatches\n", failures);
        return 1;
    }
    printf("capture_host_san: %zu texts x 7 class pairs x 6 windows x 2 flag values x 3 lists, and the scan form at every capacity: ok\n", cases);
    return 0;
}
