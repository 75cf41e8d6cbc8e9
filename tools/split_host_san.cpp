/*
 * split_host_san.cpp -- PFACX_splitFromHost under AddressSanitizer and UBSan (make -C pfac_amd/csrc san; run build/split_host_san: no arguments).
 *
 * The texts of tests/split_ref.py's table and a few hundred random ones under all four flag combinations, each at every capacity from 0 to
 * numSegments + 2, the input and the offsets in heap blocks of exactly their size: a read past the input's end (the neighbour byte of the run
 * rule, the tail of memchr) or a write at or behind `capacity` is a report.  The result is checked against a loop that states the definition
 * once more.
 */
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

/* the definition of include/pfac_ext.h, delimiter by delimiter */
static std::vector<size_t> reference(const std::string &in, const unsigned int *cls, unsigned int flags)
{
    const size_t n = in.size();
    std::vector<size_t> off;
    if (n == 0) return off;
    off.push_back(0);
    for (size_t p = 0; p < n; p++) {
        if (!inClass(cls, (unsigned char)in[p])) continue;
        if (flags & PFACX_SPLIT_RUNS) {
            if ((flags & PFACX_SPLIT_BEFORE) ? (p > 0 && inClass(cls, (unsigned char)in[p - 1])) : (p + 1 < n && inClass(cls, (unsigned char)in[p + 1]))) continue;
        }
        if (flags & PFACX_SPLIT_BEFORE) { if (p > 0) off.push_back(p); }
        else if (p + 1 < n) off.push_back(p + 1);
    }
    off.push_back(n);
    return off;
}

static int failures = 0;

static void run(PFAC_handle_t handle, const std::string &text, const unsigned int *cls, bool defaultClass)
{
    for (unsigned int flags = 0; flags < 4; flags++) {
        const std::vector<size_t> want = reference(text, cls, flags);
        const size_t segments = want.empty() ? 0 : want.size() - 1;
        size_t longest = 0;
        for (size_t k = 0; k + 1 < want.size(); k++) longest = want[k + 1] - want[k] > longest ? want[k + 1] - want[k] : longest;
        char *in = static_cast<char *>(std::malloc(text.size() ? text.size() : 1));            /* exactly the input: no byte behind it */
        std::memcpy(in, text.data(), text.size());
        for (size_t capacity = 0; capacity <= want.size() + 2; capacity++) {
            size_t *off = capacity ? static_cast<size_t *>(std::malloc(capacity * sizeof(size_t))) : nullptr;
            for (size_t k = 0; k < capacity; k++) off[k] = (size_t)-7;
            size_t n = (size_t)-1, most = (size_t)-1;
            const PFAC_status_t st = PFACX_splitFromHost(handle, in, text.size(), defaultClass ? nullptr : cls, flags, off, capacity, &n, &most);
            const bool fits = text.empty() || capacity >= want.size();
            bool ok = st == (fits ? PFAC_STATUS_SUCCESS : PFACX_STATUS_OUTPUT_TRUNCATED) && n == segments && most == longest;
            for (size_t k = 0; ok && k < capacity; k++) ok = off[k] == (k < want.size() ? want[k] : (size_t)-7);
            if (!ok) {
                failures++;
                fprintf(stderr, "MISMATCH: %zu bytes, flags %u, capacity %zu: status %d, %zu segments (want %zu), longest %zu (want %zu)\n", text.size(),
                        flags, capacity, (int)st, n, segments, most, longest);
            }
            std::free(off);
        }
        std::free(in);
    }
}

int main()
{
    PFAC_handle_t handle = nullptr;
    if (PFACX_createHostOnly(&handle) != PFAC_STATUS_SUCCESS) return 2;
    unsigned int cls[8];
    const struct { const char *text; size_t size; const char *members; bool byDefault; } table[] = {
        {"", 0, "\n", true}, {"\n", 1, "\n", true}, {"a", 1, "\n", true}, {"a\n", 2, "\n", true}, {"\na", 2, "\n", true}, {"\n\n\n", 3, "\n", true},
        {"a\n\nb", 4, "\n", true}, {"a\r\nb\r\n", 6, "\r\n", false}, {"no cut\nanywhere\n", 16, "", false},
        {"id,name,,value\n7,x,,\n", 21, ",\n", false},
    };
    size_t cases = 0;
    for (const auto &t : table) {
        classOf(t.members, cls);
        run(handle, std::string(t.text, t.size), cls, t.byDefault);
        cases++;
    }
    for (unsigned int k = 0; k < 8; k++) cls[k] = 0xFFFFFFFFu;                                  /* a full class */
    run(handle, "every byte", cls, false);
    cases++;
    unsigned int seed = 20261020u;
    const auto next = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    for (int round = 0; round < 300; round++) {
        const size_t n = next() % 70;
        const unsigned int members = round % 3 == 0 ? 1 : (round % 3 == 1 ? 3 : 128);
        std::string cl, text;
        for (unsigned int k = 0; k < members; k++) cl.push_back((char)(members == 128 ? 2 * k : "\n;x"[k]));
        for (size_t k = 0; k < n; k++) text.push_back(members == 128 ? (char)next() : "ab\n;;x\n"[next() % 7]);
        classOf(cl, cls);
        run(handle, text, cls, false);
        cases++;
    }
    PFAC_destroy(handle);
    if (failures) {
        fprintf(stderr, "%d mismatches\n", failures);
        return 1;
    }
    printf("split_host_san: %zu texts x 4 flag combinations x every capacity: ok\n", cases);
    return 0;
}
