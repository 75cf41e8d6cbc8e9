/*
 * cover_host_san.cpp -- PFACX_coverSpansFromHost on a host-only handle, for the sanitizer build of the host library (make -C pfac_amd/csrc
 * san: build/cover_host_san links lib/san/libpfac.so; CPU only).  Lists whose spans are worked out by hand, hostile entries and seeded random
 * lists, each with ends and with lengths, at every capacity from 0 to the number of spans + 1, the interval arrays and both span arrays in
 * heap blocks of exactly their size -- a write behind an array or a read behind a list is the sanitizer's to find --; the spans are compared
 * with the ones written here, the random lists' with a byte map.  Then every refusal of the call, and the device form on a handle without a
 * device.  Exit status 0: every check held.
 */
#include <climits>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "PFAC.h"
#include "pfac_ext.h"

namespace {

struct Span { int start, len; };
struct Case {
    const char *name;
    size_t size;
    unsigned int flags;
    std::vector<int> start, second;
    std::vector<Span> want;
};

int failures = 0;

void check(bool ok, const char *name, const char *what)
{
    if (ok) return;
    failures++;
    std::fprintf(stderr, "FAILED %s: %s\n", name, what);
}

template <class T> std::unique_ptr<T[]> exact(const T *from, size_t n)
{
    if (n == 0) return nullptr;
    std::unique_ptr<T[]> block(new T[n]);
    std::memcpy(block.get(), from, n * sizeof(T));
    return block;
}

/* the spans of a list by a byte map: what the random lists are compared with */
std::vector<Span> byMap(const Case &c)
{
    std::vector<char> covered(c.size + 1, 0);
    for (size_t i = 0; i < c.start.size(); i++) {
        long long lo = c.start[i], hi = (c.flags & PFACX_COVER_LENGTHS) ? lo + c.second[i] : (long long)c.second[i];
        if (lo < 0) lo = 0;
        if (hi > (long long)c.size) hi = (long long)c.size;
        for (long long b = lo; b < hi; b++) covered[(size_t)b] = 1;
    }
    std::vector<Span> out;
    for (size_t b = 0; b < c.size; b++)
        if (covered[b]) {
            if (b > 0 && covered[b - 1]) out.back().len++;
            else out.push_back({(int)b, 1});
        }
    return out;
}

void runCase(PFAC_handle_t h, const Case &c)
{
    const size_t n = c.start.size();
    size_t coveredWant = 0;
    for (const Span &s : c.want) coveredWant += (size_t)s.len;
    for (size_t capacity = 0; capacity <= c.want.size() + 1; capacity++) {
        const auto start = exact(c.start.data(), n), second = exact(c.second.data(), n);
        std::unique_ptr<int[]> spanStart(capacity ? new int[capacity] : nullptr), spanLen(capacity ? new int[capacity] : nullptr);
        size_t spans = 99, covered = 99;
        const PFAC_status_t st = PFACX_coverSpansFromHost(h, start.get(), second.get(), n, c.size, c.flags, spanStart.get(), spanLen.get(), capacity,
                                                          &spans, &covered);
        check(st == (capacity < c.want.size() ? PFACX_STATUS_OUTPUT_TRUNCATED : PFAC_STATUS_SUCCESS), c.name, "status");
        check(spans == c.want.size() && covered == coveredWant, c.name, "counts");
        for (size_t k = 0; k < capacity && k < c.want.size(); k++)
            check(spanStart[k] == c.want[k].start && spanLen[k] == c.want[k].len, c.name, "span");
        check(n == 0 || (std::memcmp(start.get(), c.start.data(), n * sizeof(int)) == 0 && std::memcmp(second.get(), c.second.data(), n * sizeof(int)) == 0),
              c.name, "the interval arrays were modified");
    }
}

unsigned int rngState = 20261021u;
unsigned int next() { rngState = rngState * 1664525u + 1013904223u; return rngState >> 8; }

void refusals(PFAC_handle_t h)
{
    int a[2] = {1, 5}, b[2] = {3, 9}, o[4] = {-7, -7, -7, -7}, l[4] = {-7, -7, -7, -7};
    size_t ns = 77, cb = 77;
    const PFAC_status_t bad = PFAC_STATUS_INVALID_PARAMETER;
    check(PFACX_coverSpansFromHost(nullptr, a, b, 2, 10, 0, o, l, 4, &ns, &cb) == PFAC_STATUS_INVALID_HANDLE, "refusal", "null handle");
    check(PFACX_coverSpansFromHost(h, a, b, 2, 10, 0, o, l, 4, nullptr, &cb) == bad, "refusal", "null span count");
    check(PFACX_coverSpansFromHost(h, a, b, 2, 10, 0, o, l, 4, &ns, nullptr) == bad, "refusal", "null byte count");
    check(PFACX_coverSpansFromHost(h, nullptr, b, 2, 10, 0, o, l, 4, &ns, &cb) == bad, "refusal", "null starts");
    check(PFACX_coverSpansFromHost(h, a, nullptr, 2, 10, 0, o, l, 4, &ns, &cb) == bad, "refusal", "null ends");
    check(PFACX_coverSpansFromHost(h, a, b, 2, 10, 0, nullptr, l, 4, &ns, &cb) == bad, "refusal", "null span starts");
    check(PFACX_coverSpansFromHost(h, a, b, 2, 10, 0, o, nullptr, 4, &ns, &cb) == bad, "refusal", "null span lengths");
    check(PFACX_coverSpansFromHost(h, a, b, 2, (size_t)1 << 31, 0, o, l, 4, &ns, &cb) == bad, "refusal", "size 2^31");
    check(PFACX_coverSpansFromHost(h, a, b, (size_t)1 << 31, 10, 0, o, l, 4, &ns, &cb) == bad, "refusal", "2^31 intervals");
    check(PFACX_coverSpansFromHost(h, a, b, 2, 10, 2u, o, l, 4, &ns, &cb) == bad, "refusal", "an unknown flag");
    check(PFACX_coverSpansFromHost(h, a, b, 2, 10, 0x80000001u, o, l, 4, &ns, &cb) == bad, "refusal", "an unknown flag beside the known one");
    check(ns == 77 && cb == 77 && o[0] == -7 && l[0] == -7, "refusal", "a refused call wrote something");
    check(PFACX_coverSpansFromDevice(h, a, b, 2, 10, 0, o, l, 4, &ns, &cb) == PFAC_STATUS_LIB_NOT_EXIST, "refusal", "the device form without a device");
    check(PFACX_coverSpansFromDevice(h, a, b, 2, 10, 0, a, l, 4, &ns, &cb) == bad, "refusal", "the device form: a span array over an interval array");
    check(PFACX_coverSpansFromHost(h, nullptr, nullptr, 0, 10, 0, nullptr, nullptr, 0, &ns, &cb) == PFAC_STATUS_SUCCESS && ns == 0 && cb == 0, "empty",
          "no intervals");
    ns = cb = 77;
    check(PFACX_coverSpansFromHost(h, a, b, 2, 0, 0, o, l, 4, &ns, &cb) == PFAC_STATUS_SUCCESS && ns == 0 && cb == 0 && o[0] == -7, "empty", "size 0");
}

} // namespace

int main()
{
    PFAC_handle_t h = nullptr;
    if (PFACX_createHostOnly(&h) != PFAC_STATUS_SUCCESS || !h) {
        std::fprintf(stderr, "PFACX_createHostOnly failed\n");
        return 2;
    }
    const unsigned int L = PFACX_COVER_LENGTHS;
    std::vector<Case> cases = {
        {"one byte", 10, 0, {4}, {5}, {{4, 1}}},
        {"the whole range", 10, 0, {0}, {10}, {{0, 10}}},
        {"touching", 64, 0, {8, 3}, {11, 8}, {{3, 8}}},
        {"a gap of one", 64, 0, {3, 9}, {8, 11}, {{3, 5}, {9, 2}}},
        {"nested and duplicate", 64, 0, {10, 12, 10, 11}, {30, 14, 30, 29}, {{10, 20}}},
        {"unsorted", 100, 0, {40, 3, 90, 20, 3, 60, 21}, {45, 8, 99, 22, 5, 61, 30}, {{3, 5}, {20, 10}, {40, 5}, {60, 1}, {90, 9}}},
        {"clamped", 100, 0, {-5, 90, INT_MIN}, {7, 250, 2}, {{0, 7}, {90, 10}}},
        {"empty after the clamp", 100, 0, {40, 60, 100, 170, -3, INT_MAX, INT_MIN}, {40, 20, 130, 180, 0, INT_MIN, INT_MIN}, {}},
        {"INT_MIN to INT_MAX", 100, 0, {INT_MIN}, {INT_MAX}, {{0, 100}}},
        {"lengths", 100, L, {7, 1, 2}, {2, 1, 2}, {{1, 3}, {7, 2}}},
        {"a length that overflows 32 bits", 100, L, {50, INT_MAX}, {INT_MAX, INT_MAX}, {{50, 50}}},
        {"negative lengths and starts", 100, L, {50, 70, -5, -5, INT_MIN}, {-10, INT_MIN, 10, 5, INT_MAX}, {{0, 5}}},
        {"the largest size", (size_t)INT_MAX, 0, {INT_MAX - 1, 0, 5}, {INT_MAX, 1, INT_MAX - 1}, {{0, 1}, {5, INT_MAX - 5}}},
        {"alternating, odd", 7, 0, {6, 4, 2, 0}, {7, 5, 3, 1}, {{0, 1}, {2, 1}, {4, 1}, {6, 1}}},
        {"alternating, even", 6, 0, {0, 2, 4}, {1, 3, 5}, {{0, 1}, {2, 1}, {4, 1}}},
    };
    for (int r = 0; r < 60; r++) {                             /* seeded lists against the byte map, with ends and with lengths */
        Case c{"random", (size_t)(1 + next() % 300), (r & 1) ? L : 0u, {}, {}, {}};
        const int count = 1 + (int)(next() % 40);
        for (int i = 0; i < count; i++) {
            const int s = (int)(next() % (c.size + 6)) - 3, len = (int)(next() % 20) - 3;
            c.start.push_back(s);
            c.second.push_back((r & 1) ? len : s + len);
        }
        c.want = byMap(c);
        cases.push_back(c);
    }
    for (const Case &c : cases) runCase(h, c);
    refusals(h);
    PFAC_destroy(h);
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("cover_host_san: %zu lists at every capacity and every refusal: OK\n", cases.size());
    return 0;
}
