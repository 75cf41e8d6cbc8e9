/*
 * locate_host_san.cpp -- PFACX_locatePairsFromHost and PFACX_matchLocatedFromHost under AddressSanitizer and UBSan (make -C pfac_amd/csrc san; run
 * build/locate_host_san: no arguments).
 *
 * The texts of tests/locate_ref.py's table and a few hundred random ones under all four flag combinations, with sorted lists (duplicates, both ends
 * outside the input), every position, and lists that are not sorted at all; the input, the positions and both outputs in heap blocks of exactly
 * their size: a read past the input's or the list's end or a write past an output's is a report.  Sorted lists are checked against a loop that
 * states the definition once more, position by position; the scan form at every locCapacity from 0 to the count + 1.
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

/* is position c of [1, n - 1] a cut: the definition of include/pfac_ext.h, delimiter by delimiter */
static bool cutAt(const std::string &in, const unsigned int *cls, unsigned int flags, size_t c)
{
    const size_t n = in.size();
    const size_t p = (flags & PFACX_SPLIT_BEFORE) ? c : c - 1;                                   /* the delimiter that would give the cut c */
    if (c == 0 || c >= n || !inClass(cls, (unsigned char)in[p])) return false;
    if (!(flags & PFACX_SPLIT_RUNS)) return true;
    return (flags & PFACX_SPLIT_BEFORE) ? !inClass(cls, (unsigned char)in[p - 1]) : !inClass(cls, (unsigned char)in[p + 1]);
}

static void reference(const std::string &in, const unsigned int *cls, unsigned int flags, int p, int *record, int *column)
{
    *record = *column = -1;
    if (p < 0 || (size_t)p >= in.size()) return;
    int cuts = 0, start = 0;
    for (size_t c = 1; c <= (size_t)p; c++)
        if (cutAt(in, cls, flags, c)) { cuts++; start = (int)c; }
    *record = cuts;
    *column = p - start;
}

static int failures = 0;

template <class T>
static T *exactly(const std::vector<T> &v)                                                      /* a heap block of exactly v's bytes */
{
    T *p = static_cast<T *>(std::malloc(v.size() ? v.size() * sizeof(T) : 1));
    if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

static void run(PFAC_handle_t handle, const std::string &text, const unsigned int *cls, bool defaultClass, const std::vector<int> &list, bool sorted)
{
    for (unsigned int flags = 0; flags < 4; flags++) {
        size_t records = 1;
        for (size_t c = 1; c < text.size(); c++) records += cutAt(text, cls, flags, c) ? 1 : 0;
        if (text.empty()) records = 0;
        char *in = exactly(std::vector<char>(text.begin(), text.end()));
        int *pos = exactly(list);
        for (int withColumn = 0; withColumn < 2; withColumn++) {
            int *record = exactly(std::vector<int>(list.size(), -7)), *column = withColumn ? exactly(std::vector<int>(list.size(), -7)) : nullptr;
            size_t n = (size_t)-1;
            const PFAC_status_t st = PFACX_locatePairsFromHost(handle, in, text.size(), defaultClass ? nullptr : cls, flags, pos, list.size(), record,
                                                               column, &n);
            bool ok = st == PFAC_STATUS_SUCCESS && n == records;
            for (size_t k = 0; ok && sorted && !text.empty() && k < list.size(); k++) {
                int r, c;
                reference(text, cls, flags, list[k], &r, &c);
                ok = record[k] == r && (!column || column[k] == c);
            }
            if (!ok) {
                failures++;
                fprintf(stderr, "MISMATCH: %zu bytes, %zu positions, flags %u: status %d, %zu records (want %zu)\n", text.size(), list.size(), flags,
                        (int)st, n, records);
            }
            std::free(record);
            std::free(column);
        }
        std::free(pos);
        std::free(in);
    }
}

/* the scan form: ids and positions of `size` entries, record and column of exactly locCapacity */
static void runScan(PFAC_handle_t handle, const std::string &text)
{
    const size_t n = text.size();
    char *in = exactly(std::vector<char>(text.begin(), text.end()));
    int *ids = exactly(std::vector<int>(n, 0)), *pos = exactly(std::vector<int>(n, 0));
    int count = -1;
    if (PFAC_matchFromHostReduce(handle, in, n, ids, pos, &count) != PFAC_STATUS_SUCCESS) failures++;
    unsigned int cls[8];
    classOf("\n", cls);
    for (size_t capacity = 0; capacity <= (size_t)count + 1; capacity++) {
        int *ids2 = exactly(std::vector<int>(n, 0)), *pos2 = exactly(std::vector<int>(n, 0));
        int *record = exactly(std::vector<int>(capacity, -7)), *column = exactly(std::vector<int>(capacity, -7));
        int found = -1;
        const PFAC_status_t st = PFACX_matchLocatedFromHost(handle, in, n, nullptr, 0, ids2, pos2, capacity ? record : nullptr, capacity ? column : nullptr,
                                                            capacity, &found);
        bool ok = found == count && st == (capacity >= (size_t)count ? PFAC_STATUS_SUCCESS : PFACX_STATUS_OUTPUT_TRUNCATED);
        for (size_t k = 0; ok && k < capacity; k++) {
            int r = -7, c = -7;
            if (k < (size_t)count) reference(text, cls, 0, pos[k], &r, &c);
            ok = record[k] == r && column[k] == c && (k >= (size_t)count || (ids2[k] == ids[k] && pos2[k] == pos[k]));
        }
        if (!ok) {
            failures++;
            fprintf(stderr, "MISMATCH: the scan form at locCapacity %zu: status %d, %d pairs (want %d)\n", capacity, (int)st, found, count);
        }
        std::free(ids2); std::free(pos2); std::free(record); std::free(column);
    }
    std::free(in); std::free(ids); std::free(pos);
}

int main()
{
    PFAC_handle_t handle = nullptr;
    if (PFACX_createHostOnly(&handle) != PFAC_STATUS_SUCCESS) return 2;
    unsigned int cls[8];
    unsigned int seed = 20261020u;
    const auto next = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    const auto lists = [&](const std::string &text, const unsigned int *c, bool byDefault) {
        const int n = (int)text.size();
        std::vector<int> every, some, wild;
        for (int p = 0; p < n; p++) every.push_back(p);
        for (int k = 0; k < n / 2 + 3; k++) some.push_back((int)(next() % (unsigned int)(n + 6)) - 3);       /* duplicates, both ends outside */
        wild = some;
        std::sort(some.begin(), some.end());
        wild.push_back(-2147483647 - 1);
        wild.push_back(2147483647);
        run(handle, text, c, byDefault, every, true);
        run(handle, text, c, byDefault, some, true);
        run(handle, text, c, byDefault, wild, false);
        run(handle, text, c, byDefault, {}, true);
    };
    const struct { const char *text; size_t size; const char *members; bool byDefault; } table[] = {
        {"", 0, "\n", true}, {"x", 1, "\n", true}, {"\n", 1, "\n", true}, {"ab\ncd\n\nxyz", 10, "\n", true}, {"ab\ncd\n\nxyz", 10, "", false},
        {"a\r\nbc\r\n\r\nd", 10, "\r\n", false}, {"abc\ndef\n", 8, "\n", true},
    };
    size_t cases = 0;
    for (const auto &t : table) {
        classOf(t.members, cls);
        lists(std::string(t.text, t.size), cls, t.byDefault);
        cases++;
    }
    for (unsigned int k = 0; k < 8; k++) cls[k] = 0xFFFFFFFFu;                                  /* a full class */
    lists("every byte", cls, false);
    cases++;
    for (int round = 0; round < 300; round++) {
        const size_t n = next() % 70;
        const unsigned int members = round % 3 == 0 ? 1 : (round % 3 == 1 ? 3 : 128);
        std::string cl, text;
        for (unsigned int k = 0; k < members; k++) cl.push_back((char)(members == 128 ? 2 * k : "\n;x"[k]));
        for (size_t k = 0; k < n; k++) text.push_back(members == 128 ? (char)next() : "ab\n;;x\n"[next() % 7]);
        classOf(cl, cls);
        lists(text, cls, false);
        cases++;
    }
    static const char patterns[] = "ab\nabc\nERROR\nxyz\nb\n";
    if (PFACX_readPatternFromMemory(handle, patterns, sizeof(patterns) - 1) != PFAC_STATUS_SUCCESS) return 2;
    runScan(handle, "an ab here\nERROR abc\n\nxyz ab\nlast abc b");
    runScan(handle, "no match in this line");
    PFAC_destroy(handle);
    if (failures) {
        fprintf(stderr, "%d mismatches\n", failures);
        return 1;
    }
    printf("locate_host_san: %zu texts x 4 flag combinations x 4 lists, and the scan form at every capacity: ok\n", cases);
    return 0;
}
