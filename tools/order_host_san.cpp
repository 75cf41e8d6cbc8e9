/*
 * order_host_san.cpp -- PFACX_orderHitsFromHost on a host-only handle, for the sanitizer build of the host library (make -C pfac_amd/csrc san:
 * build/order_host_san links lib/san/libpfac.so; CPU only).  Lists whose order is worked out by hand and seeded random lists, each with every
 * combination of the optional columns, with and without d_perm, with and without the ties flag, every array a heap block of exactly its size
 * -- a write behind an array or a read behind a list is the sanitizer's to find --; the result is compared with std::stable_sort over tuples
 * written here.  Then every refusal of the call, each pairwise overlap included, and the device form on a handle without a device.  Exit
 * status 0: every check held.
 */
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "PFAC.h"
#include "pfac_ext.h"

namespace {

int failures = 0;

void check(bool ok, const char *name, const char *what)
{
    if (ok) return;
    failures++;
    std::fprintf(stderr, "FAILED %s: %s\n", name, what);
}

std::unique_ptr<int[]> exact(const std::vector<int> &from)
{
    if (from.empty()) return nullptr;
    std::unique_ptr<int[]> block(new int[from.size()]);
    std::memcpy(block.get(), from.data(), from.size() * sizeof(int));
    return block;
}

struct Entry { int start, id, end, aux, index; };

/* columns: bit 0 ids, bit 1 ends, bit 2 aux, bit 3 perm */
void runCase(PFAC_handle_t h, const char *name, const std::vector<int> &start, const std::vector<int> &ids, bool ties, unsigned int columns)
{
    const size_t n = start.size();
    std::vector<Entry> want(n);
    std::vector<int> end(n), aux(n);
    for (size_t k = 0; k < n; k++) {
        end[k] = (int)(k * 7 + 1);
        aux[k] = (int)k;
        want[k] = {start[k], ids[k], end[k], aux[k], (int)k};
    }
    std::stable_sort(want.begin(), want.end(), [ties](const Entry &a, const Entry &b) {
        if (a.start != b.start) return a.start < b.start;
        return ties && a.id < b.id;
    });
    bool ordered = true;
    for (size_t k = 0; k < n; k++) ordered = ordered && want[k].index == (int)k;

    std::unique_ptr<int[]> s = exact(start), i = (columns & 1u) ? exact(ids) : nullptr, e = (columns & 2u) ? exact(end) : nullptr,
                           a = (columns & 4u) ? exact(aux) : nullptr, p = (columns & 8u) && n ? std::unique_ptr<int[]>(new int[n]) : nullptr;
    int was = -1;
    const PFAC_status_t st = PFACX_orderHitsFromHost(h, s.get(), i.get(), e.get(), a.get(), n, ties ? PFACX_ORDER_TIES_BY_ID : 0u, p.get(), &was);
    check(st == PFAC_STATUS_SUCCESS, name, "status");
    check(was == (ordered ? 1 : 0), name, "wasOrdered");
    for (size_t k = 0; k < n; k++) {
        check(s[k] == want[k].start, name, "start");
        if (i) check(i[k] == want[k].id, name, "id");
        if (e) check(e[k] == want[k].end, name, "end");
        if (a) check(a[k] == want[k].aux, name, "aux");
        if (p) check(p[k] == want[k].index, name, "perm");
    }
}

void runAll(PFAC_handle_t h, const char *name, const std::vector<int> &start, const std::vector<int> &ids)
{
    for (unsigned int columns = 0; columns < 16; columns++) {
        runCase(h, name, start, ids, false, columns);
        if ((columns & 1u) && !start.empty()) runCase(h, name, start, ids, true, columns);   /* (no list: no ids array, and the flag without one is refused) */
    }
}

} // namespace

int main()
{
    PFAC_handle_t h = nullptr;
    if (PFACX_createHostOnly(&h) != PFAC_STATUS_SUCCESS || !h) {
        std::fprintf(stderr, "PFACX_createHostOnly failed\n");
        return 2;
    }
    runAll(h, "empty", {}, {});
    runAll(h, "one", {INT_MIN}, {INT_MAX});
    runAll(h, "two swapped", {5, 3}, {1, 2});
    runAll(h, "ties", {4, 4, 4, 1, 1}, {9, 8, 7, 6, 5});
    runAll(h, "extremes", {INT_MAX, INT_MIN, 0, -1, 1, INT_MIN, INT_MAX}, {INT_MIN, INT_MAX, 0, -1, 1, INT_MIN, INT_MAX});
    runAll(h, "sign bit", {5, 5 + INT_MIN, 5, 5 + INT_MIN}, {1, 1, 1, 1});
    runAll(h, "all equal", {9, 9, 9, 9, 9, 9}, {6, 5, 4, 3, 2, 1});
    runAll(h, "ordered", {1, 1, 2, 3, 3, 3}, {1, 1, 1, 2, 4, 4});
    runAll(h, "ordered by start only", {1, 1, 2, 3, 3, 3}, {2, 1, 1, 2, 4, 3});
    {
        std::vector<int> down(300), ids(300);
        for (int k = 0; k < 300; k++) { down[(size_t)k] = 300 - k; ids[(size_t)k] = k % 7; }
        runAll(h, "descending", down, ids);
    }
    std::mt19937 rng(12345);
    for (int round = 0; round < 200; round++) {
        const size_t n = 1 + rng() % 500;
        std::vector<int> start(n), ids(n);
        const int spread = round % 3 == 0 ? 4 : round % 3 == 1 ? 1000 : INT_MAX;
        for (size_t k = 0; k < n; k++) {
            start[k] = (int)(rng() % (unsigned int)spread) - (round % 2 ? spread / 2 : 0);
            ids[k] = (int)(rng() % 5u) - 2;
        }
        runAll(h, "seeded", start, ids);
    }

    /* the refusals */
    {
        std::unique_ptr<int[]> block(new int[5 * 8]);
        for (int k = 0; k < 40; k++) block[(size_t)k] = 40 - k;
        int *col[5] = {block.get(), block.get() + 8, block.get() + 16, block.get() + 24, block.get() + 32};
        int was = 77;
        const auto call = [&](PFAC_handle_t hh, int *s, int *i, int *e, int *a, size_t n, unsigned int flags, int *p) {
            return PFACX_orderHitsFromHost(hh, s, i, e, a, n, flags, p, &was);
        };
        check(call(nullptr, col[0], col[1], col[2], col[3], 8, 0, col[4]) == PFAC_STATUS_INVALID_PARAMETER, "refusals", "null handle");
        check(call(h, nullptr, col[1], col[2], col[3], 8, 0, col[4]) == PFAC_STATUS_INVALID_PARAMETER, "refusals", "null starts");
        check(call(h, col[0], col[1], col[2], col[3], (size_t)1 << 31, 0, col[4]) == PFAC_STATUS_INVALID_PARAMETER, "refusals", "2^31 hits");
        check(call(h, col[0], col[1], col[2], col[3], 8, 2u, col[4]) == PFAC_STATUS_INVALID_PARAMETER, "refusals", "unknown flag");
        check(call(h, col[0], nullptr, col[2], col[3], 8, PFACX_ORDER_TIES_BY_ID, col[4]) == PFAC_STATUS_INVALID_PARAMETER, "refusals", "ties without ids");
        for (int x = 0; x < 5; x++)
            for (int y = x + 1; y < 5; y++)
                for (int shift : {0, 7, -7}) {
                    int *arg[5] = {col[0], col[1], col[2], col[3], col[4]};
                    arg[y] = arg[x] + shift;
                    check(call(h, arg[0], arg[1], arg[2], arg[3], 8, 0, arg[4]) == PFAC_STATUS_INVALID_PARAMETER, "refusals", "overlap");
                }
        check(was == 77, "refusals", "a refused call wrote wasOrdered");
        for (int k = 0; k < 40; k++) check(block[(size_t)k] == 40 - k, "refusals", "a refused call wrote an array");
        check(PFACX_orderHitsFromDevice(h, col[0], nullptr, nullptr, nullptr, 8, 0, nullptr, &was) == PFAC_STATUS_LIB_NOT_EXIST, "refusals",
              "the device form without a device");
        check(PFACX_orderHitsFromHost(h, col[0], nullptr, nullptr, nullptr, 8, 0, nullptr, nullptr) == PFAC_STATUS_SUCCESS, "no wasOrdered", "status");
        for (int k = 0; k < 8; k++) check(block[(size_t)k] == 33 + k, "no wasOrdered", "order");
    }

    PFAC_destroy(h);
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("order_host_san: every check held\n");
    return 0;
}
