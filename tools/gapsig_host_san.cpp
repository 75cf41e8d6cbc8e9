/*
 * gapsig_host_san.cpp -- PFACX_gapsigOpen, PFACX_gapsigOpenText, PFACX_gapsigGetAnchors and PFACX_gapsigMatchFromHost on a host-only handle, for
 * the sanitizer build of the host library (make -C pfac_amd/csrc san: build/gapsig_host_san links lib/san/libpfac.so; CPU only).  Cases of
 * tests/gapsig_ref.py's table are opened through the text form from a heap block of exactly its size and run on both CPU platforms at every
 * capacity from 0 to the list's length + 1, with and without the end array, into arrays allocated at exactly `capacity` entries and over an
 * input in a heap block of exactly its size -- a write behind the arrays or a read behind the input is the sanitizer's to find --; the lists
 * are compared with what the table says by hand and with the full list.  The binary form is driven with CSR arrays of exactly their size, the
 * getter with arrays of exactly S + 1 entries.  Then every refusal of both open calls.  Exit status 0: every check held.
 */
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "PFAC.h"
#include "pfac_ext.h"

namespace {

struct Entry { int id, start, end; };
struct Case {
    const char *name;
    std::string text;                           /* the text form */
    std::string input;
    std::vector<Entry> want;                    /* by hand, in list order */
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
    std::unique_ptr<T[]> block(new T[n ? n : 1]);
    if (n) std::memcpy(block.get(), from, n * sizeof(T));
    return block;
}

PFACX_gapsig_t openText(PFAC_handle_t h, const std::string &text, size_t cut, int *bad, PFAC_status_t *st)
{
    const auto block = exact(text.data(), text.size());
    PFACX_gapsig_t sg = nullptr;
    *st = PFACX_gapsigOpenText(h, block.get(), text.size(), cut, &sg, bad);
    return sg;
}

void runCase(PFAC_handle_t h, const Case &c)
{
    int bad = -1;
    PFAC_status_t st;
    PFACX_gapsig_t sg = openText(h, c.text, 0, &bad, &st);
    check(st == PFAC_STATUS_SUCCESS && sg && bad == 0, c.name, "open");
    if (!sg) return;
    const auto in = exact(c.input.data(), c.input.size());
    const size_t total = c.want.size();
    for (int platform : {(int)PFAC_PLATFORM_CPU, (int)PFAC_PLATFORM_CPU_OMP}) {
        check(PFAC_setPlatform(h, (PFAC_platform_t)platform) == PFAC_STATUS_SUCCESS, c.name, "platform");
        for (size_t cap = 0; cap <= total + 1; cap++) {
            for (int withEnd = 0; withEnd < 2; withEnd++) {
                std::unique_ptr<int[]> ids(new int[cap ? cap : 1]), pos(new int[cap ? cap : 1]), end(new int[cap ? cap : 1]);
                size_t n = 777;
                st = PFACX_gapsigMatchFromHost(sg, in.get(), c.input.size(), cap ? ids.get() : nullptr, cap ? pos.get() : nullptr,
                                               cap && withEnd ? end.get() : nullptr, cap, &n);
                check(n == total, c.name, "the full length");
                check(st == (cap < total ? PFACX_STATUS_OUTPUT_TRUNCATED : PFAC_STATUS_SUCCESS), c.name, "the status");
                for (size_t k = 0; k < cap && k < total; k++)
                    check(ids[k] == c.want[k].id && pos[k] == c.want[k].start && (!withEnd || end[k] == c.want[k].end), c.name, "an entry");
            }
        }
    }
    check(PFACX_gapsigClose(sg) == PFAC_STATUS_SUCCESS, c.name, "close");
}

void refusals(PFAC_handle_t h)
{
    static const struct { const char *text; int line; } kText[] = {
        {"61 62\n{1} 61\n", 2}, {"61 {1}\n", 1}, {"61 {1} {2} 62\n", 1}, {"61 {2-1} 62\n", 1}, {"61 * 62\n", 1}, {"61 {1-} 62\n", 1},
        {"61 {65536} 62\n", 1}, {"61 {} 62\n", 1}, {"61 {-} 62\n", 1}, {"61 {1] 62\n", 1}, {"61 {1 62\n", 1}, {"61 { 1} 62\n", 1},
        {"61 {1--2} 62\n", 1}, {"61 62\n\n", 2}, {"6 {1} 62\n", 1}, {"61 62\n61 {1} 62", 2}, {"{", 1}, {"61 {1", 1}, {"61 [", 1},
        {"61 62\n61 {0-64} 62\n", 2}, {"61 {0-32} 62 {0-32} 63\n", 1}, {"0A {1} ?? {2} 4?\n", 1}, {"61 {99999999999999999999} 62\n", 1},
    };
    PFAC_status_t st;
    for (const auto &r : kText) {
        int bad = -1;
        PFACX_gapsig_t sg = openText(h, r.text, 0, &bad, &st);
        check(st == PFAC_STATUS_INVALID_PARAMETER && !sg && bad == r.line, r.text, "a text refusal");
    }
    std::string parts65;
    for (int j = 0; j < 65; j++) parts65 += j ? " {1} 61" : "61";
    int bad = -1;
    PFACX_gapsig_t sg = openText(h, "61\n" + parts65 + "\n", 0, &bad, &st);
    check(st == PFAC_STATUS_INVALID_PARAMETER && !sg && bad == 2, "65 parts", "a text refusal");

    /* the binary form: arrays of exactly their size */
    const unsigned char values[] = {'a', 'b', 'c', 'd', 'e', 'f'}, masks[] = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF};
    struct Binary { const char *name; std::vector<size_t> partOff, sigPart; std::vector<unsigned int> lo, hi; int bad; };
    const std::vector<Binary> rows = {
        {"an empty part", {0, 2, 2, 4}, {0, 1, 3}, {9, 0, 9}, {9, 1, 9}, 2},
        {"no part", {0, 2, 4}, {0, 0, 2}, {0, 9}, {1, 9}, 1},
        {"lo above hi", {0, 2, 4, 6}, {0, 1, 3}, {9, 3, 9}, {9, 2, 9}, 2},
        {"hi above 65 535", {0, 2, 4, 6}, {0, 1, 3}, {9, 0, 9}, {9, 65536, 9}, 2},
        {"slack 64", {0, 2, 4, 6}, {0, 3}, {5, 0, 9}, {37, 32, 9}, 1},
    };
    for (const Binary &r : rows) {
        const auto v = exact(values, r.partOff.back()), m = exact(masks, r.partOff.back());
        const auto po = exact(r.partOff.data(), r.partOff.size()), sp = exact(r.sigPart.data(), r.sigPart.size());
        const auto lo = exact(r.lo.data(), r.lo.size()), hi = exact(r.hi.data(), r.hi.size());
        bad = -1;
        sg = nullptr;
        st = PFACX_gapsigOpen(h, v.get(), m.get(), po.get(), sp.get(), lo.get(), hi.get(), r.sigPart.size() - 1, 0, &sg, &bad);
        check(st == PFAC_STATUS_INVALID_PARAMETER && !sg && bad == r.bad, r.name, "a binary refusal");
    }
    const size_t partOff[] = {0, 2, 4, 6}, sigPart[] = {0, 1, 3};
    const unsigned int lo[] = {9, 0, 9}, hi[] = {9, 63, 9};
    check(PFACX_gapsigOpen(h, nullptr, masks, partOff, sigPart, lo, hi, 2, 0, &sg, &bad) == PFAC_STATUS_INVALID_PARAMETER, "null", "values");
    check(PFACX_gapsigOpen(h, values, masks, partOff, sigPart, nullptr, hi, 2, 0, &sg, &bad) == PFAC_STATUS_INVALID_PARAMETER, "null", "gapLo");
    check(PFACX_gapsigOpen(h, values, masks, partOff, sigPart, lo, hi, 0, 0, &sg, &bad) == PFAC_STATUS_INVALID_PARAMETER, "null", "no signatures");
    check(PFACX_gapsigOpen(nullptr, values, masks, partOff, sigPart, lo, hi, 2, 0, &sg, &bad) == PFAC_STATUS_INVALID_HANDLE, "null", "handle");
    /* ... and the one that passes: the getter into arrays of exactly S + 1 entries, the match over an input of exactly its size */
    const auto v = exact(values, 6), m = exact(masks, 6);
    const auto po = exact(partOff, 4), sp = exact(sigPart, 3);
    const auto l = exact(lo, 3), u = exact(hi, 3);
    st = PFACX_gapsigOpen(h, v.get(), m.get(), po.get(), sp.get(), l.get(), u.get(), 2, 0, &sg, &bad);
    check(st == PFAC_STATUS_SUCCESS && sg && bad == 0, "binary", "open");
    if (!sg) return;
    std::unique_ptr<int[]> aid(new int[3]), apart(new int[3]), aoff(new int[3]), alen(new int[3]);
    check(PFACX_gapsigGetAnchors(sg, aid.get(), apart.get(), aoff.get(), alen.get(), 2) == PFAC_STATUS_INVALID_PARAMETER, "binary", "a short getter");
    check(PFACX_gapsigGetAnchors(sg, aid.get(), apart.get(), aoff.get(), alen.get(), 3) == PFAC_STATUS_SUCCESS, "binary", "the getter");
    check(aid[1] == 1 && aid[2] == 2 && apart[2] == 0 && aoff[2] == 0 && alen[1] == 2 && alen[2] == 2, "binary", "the anchors");
    std::string text = "cd";
    text += std::string(63, '.') + "ef ab cdef";
    const auto in = exact(text.data(), text.size());
    std::unique_ptr<int[]> ids(new int[3]), pos(new int[3]), end(new int[3]);
    size_t n = 0;
    st = PFACX_gapsigMatchFromHost(sg, in.get(), text.size(), ids.get(), pos.get(), end.get(), 3, &n);
    check(st == PFAC_STATUS_SUCCESS && n == 3, "binary", "the list");
    check(ids[0] == 2 && pos[0] == 0 && end[0] == 67 && ids[1] == 1 && pos[1] == 68 && end[1] == 70 && ids[2] == 2 && pos[2] == 71 && end[2] == 75,
          "binary", "the entries");
    size_t none = 5;
    check(PFACX_gapsigMatchFromHost(sg, in.get(), 0, nullptr, nullptr, nullptr, 0, &none) == PFAC_STATUS_SUCCESS && none == 0, "binary", "size 0");
    check(PFACX_gapsigMatchFromDevice(sg, in.get(), text.size(), ids.get(), pos.get(), end.get(), text.size(), &n) == PFAC_STATUS_LIB_NOT_EXIST,
          "binary", "a device form on a host-only handle");
    /* left open: PFAC_destroy closes it */
}

} // namespace

int main()
{
    PFAC_handle_t h = nullptr;
    if (PFACX_createHostOnly(&h) != PFAC_STATUS_SUCCESS) return 2;
    std::string many(64, 'a');
    many += "KL";
    std::vector<Entry> manyWant;
    for (int s = 0; s < 64; s++) manyWant.push_back({1, s, 66});
    std::string parts64 = "80 30", in64 = "\x80\x30";
    for (int j = 1; j < 64; j++) {
        char part[32];
        std::snprintf(part, sizeof part, " {0-1} %02X %02X", 0x80 + j, 0x30 + j % 10);
        parts64 += part;
        in64 += (j & 1) ? "." : "";
        in64 += std::string(1, (char)(0x80 + j)) + std::string(1, (char)(0x30 + j % 10));
    }
    const std::vector<Case> cases = {
        {"gap-0", "61 62 {0} 63 64\n", "abcd abxcd ab cd abcd", {{1, 0, 4}, {1, 17, 21}}},
        {"spellings", "61 62 {-1} 63 64\r\n61 62 [0-1] 63 64\n61 62\t[1]\t63 64\n", "abcd abxcd", {{2, 0, 4}, {1, 0, 4}, {3, 5, 10}, {2, 5, 10}, {1, 5, 10}}},
        {"identical-signatures", "61 ?? {1-2} 63 64\n61 ?? {1-2} 63 64\n", "ab.cd ab..cd abcd", {{2, 0, 5}, {1, 0, 5}, {2, 6, 12}, {1, 6, 12}}},
        {"owner-both-complete", "61 {0-2} 4B 4B {0-2} 7A\n", "aKKK.z", {{1, 0, 6}}},
        {"owner-nearer-dead", "61 {0-2} 4B 4B {0} 7A\n", "aKKKz", {{1, 0, 5}}},
        {"owner-neither", "61 {0-2} 4B 4B {0} 7A\n", "aKKK.z aKKK", {}},
        {"end-lazy-dead-end", "61 {0-1} 6? {0-1} 63 {0} 64\n", "abccd", {{1, 0, 5}}},
        {"input-end", "61 62 {0-2} 63 64 {0-2} 65\n", "ab.cd.e ab.cd..e ab..cd.", {{1, 0, 7}, {1, 8, 16}}},
        {"owner-many-starts", "61 {0-63} 4B 4C\n", many, manyWant},
        {"slack-63-over-63", parts64 + "\n", in64, {{1, 0, (int)in64.size()}}},
    };
    for (const Case &c : cases) runCase(h, c);
    refusals(h);
    if (PFAC_destroy(h) != PFAC_STATUS_SUCCESS) failures++;
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("gapsig_host_san: %zu cases, both open calls with their refusals, the getter and the host form at every capacity: all held\n", cases.size());
    return 0;
}
