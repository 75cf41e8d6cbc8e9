/*
 * clsig_host_san.cpp -- PFACX_clsigOpen, PFACX_clsigOpenText, PFACX_clsigGetAnchors and PFACX_clsigMatchFromHost on a host-only handle, for
 * the sanitizer build of the host library (make -C pfac_amd/csrc san: build/clsig_host_san links lib/san/libpfac.so; CPU only).  Cases of
 * tests/clsig_ref.py's table are opened through the text form from a heap block of exactly its size and run on both CPU platforms at every
 * capacity from 0 to the list's length + 1, with and without the end array, into arrays allocated at exactly `capacity` entries and over an
 * input in a heap block of exactly its size -- a write behind the arrays or a read behind the input is the sanitizer's to find --; the lists
 * are compared with what the table says by hand.  The binary form is driven with arrays of exactly their size, the getter with arrays of
 * exactly S + 1 entries.  Then every refusal of both open calls.  Exit status 0: every check held.
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
    unsigned int flags;
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

PFACX_clsig_t openText(PFAC_handle_t h, const std::string &text, unsigned int flags, int *bad, PFAC_status_t *st)
{
    const auto block = exact(text.data(), text.size());
    PFACX_clsig_t sg = nullptr;
    *st = PFACX_clsigOpenText(h, block.get(), text.size(), 0, flags, &sg, bad);
    return sg;
}

void runCase(PFAC_handle_t h, const Case &c)
{
    int bad = -1;
    PFAC_status_t st;
    PFACX_clsig_t sg = openText(h, c.text, c.flags, &bad, &st);
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
                st = PFACX_clsigMatchFromHost(sg, in.get(), c.input.size(), cap ? ids.get() : nullptr, cap ? pos.get() : nullptr,
                                              cap && withEnd ? end.get() : nullptr, cap, &n);
                check(n == total, c.name, "the full length");
                check(st == (cap < total ? PFACX_STATUS_OUTPUT_TRUNCATED : PFAC_STATUS_SUCCESS), c.name, "the status");
                for (size_t k = 0; k < cap && k < total; k++)
                    check(ids[k] == c.want[k].id && pos[k] == c.want[k].start && (!withEnd || end[k] == c.want[k].end), c.name, "an entry");
            }
        }
    }
    check(PFACX_clsigClose(sg) == PFAC_STATUS_SUCCESS, c.name, "close");
}

void refusals(PFAC_handle_t h)
{
    static const struct { const char *text; int line; } kText[] = {
        {"a*\n", 1}, {"a+\n", 1}, {"ab\na|b\n", 2}, {"(ab)\n", 1}, {"^ab\n", 1}, {"ab$\n", 1}, {"a{2,}\n", 1}, {"a{,2}\n", 1}, {"a{3,2}\n", 1},
        {"{2}a\n", 1}, {"?a\n", 1}, {"a{2}{3}\n", 1}, {"a{2}?\n", 1}, {"a[bc\n", 1}, {"a[]\n", 1}, {"a[^]\n", 1}, {"a[z-a]\n", 1}, {"a\\q\n", 1},
        {"a\\x4\n", 1}, {"a\\x\n", 1}, {"a\\\n", 1}, {"a{65536}\n", 1}, {"a{99999999999999999999}\n", 1}, {"ab\n\n", 2}, {"ab\nab", 2}, {"a[", 1},
        {"a{", 1}, {"a{1", 1}, {"a{1,", 1}, {"(?<![", 1}, {"(?<![a]", 1}, {"a(?![", 1}, {"a(?![b]\n", 1}, {"a(?![0-9])b\n", 1}, {"(?<![0-9])\n", 1},
        {"a[\\d-z]\n", 1}, {"a[a-\\d]\n", 1}, {"a[a-\\", 1}, {"a\\01\n", 1}, {"[0-9]{3}[a-f]{2}\n", 1}, {"ab\n\\n[0-9]\n", 2}, {"ab.{0,64}c\n", 1},
        {"a.{0,32}b.{0,32}c\n", 1}, {"a{65535}b\n", 1},
    };
    PFAC_status_t st;
    for (const auto &r : kText) {
        int bad = -1;
        PFACX_clsig_t sg = openText(h, r.text, 0, &bad, &st);
        check(st == PFAC_STATUS_INVALID_PARAMETER && !sg && bad == r.line, r.text, "a text refusal");
    }
    int bad = -1;
    PFACX_clsig_t sg = openText(h, "", 0, &bad, &st);
    check(st == PFAC_STATUS_INVALID_PARAMETER && !sg && bad == 0, "no line", "a text refusal");
    sg = openText(h, "ab[0-9]\n", 2u, &bad, &st);
    check(st == PFAC_STATUS_INVALID_PARAMETER && !sg, "flags", "an unknown flag bit");
    std::string parts65 = "a";
    for (int j = 0; j < 32; j++) parts65 += "[0-9]a";
    sg = openText(h, "ab\n" + parts65 + "\n", 0, &bad, &st);
    check(st == PFAC_STATUS_INVALID_PARAMETER && !sg && bad == 2, "65 parts", "a text refusal");

    /* the binary form: arrays of exactly their size.  Classes: 0 = {a}, 1 = {b}, 2 = [0-9], 3 = {'\n'} */
    unsigned int classes[32] = {};
    classes[0 * 8 + ('a' >> 5)] |= 1u << ('a' & 31);
    classes[1 * 8 + ('b' >> 5)] |= 1u << ('b' & 31);
    for (unsigned int b = '0'; b <= '9'; b++) classes[2 * 8 + (b >> 5)] |= 1u << (b & 31);
    classes[3 * 8] |= 1u << '\n';
    struct Binary { const char *name; std::vector<unsigned int> cls, lo, hi; std::vector<size_t> sigElem; std::vector<int> nb, na; int bad; };
    const std::vector<Binary> rows = {
        {"no element", {0, 1}, {1, 1}, {1, 1}, {0, 0, 2}, {-1, -1}, {-1, -1}, 1},
        {"lo above hi", {0, 1, 2}, {1, 1, 3}, {1, 1, 2}, {0, 1, 3}, {-1, -1}, {-1, -1}, 2},
        {"hi == 0", {0, 1, 2}, {1, 1, 0}, {1, 1, 0}, {0, 1, 3}, {-1, -1}, {-1, -1}, 2},
        {"hi above 65 535", {0, 1, 2}, {1, 1, 0}, {1, 1, 65536}, {0, 1, 3}, {-1, -1}, {-1, -1}, 2},
        {"a class outside the table", {0, 4, 2}, {1, 1, 1}, {1, 1, 1}, {0, 1, 3}, {-1, -1}, {-1, -1}, 2},
        {"notBefore outside the table", {0, 1, 2}, {1, 1, 1}, {1, 1, 1}, {0, 1, 3}, {-1, 4}, {-1, -1}, 2},
        {"notAfter below -1", {0, 1, 2}, {1, 1, 1}, {1, 1, 1}, {0, 1, 3}, {-1, -1}, {-2, -1}, 1},
        {"slack 64", {0, 2, 1, 2}, {1, 0, 1, 0}, {1, 32, 1, 32}, {0, 4}, {-1}, {-1}, 1},
        {"a literal part of 65 536 bytes", {0, 0, 1}, {1, 65535, 1}, {1, 65535, 1}, {0, 1, 3}, {-1, -1}, {-1, -1}, 2},
        {"no anchor", {0, 2, 3, 2}, {1, 1, 1, 1}, {1, 2, 1, 1}, {0, 2, 4}, {-1, -1}, {-1, -1}, 2},
    };
    for (const Binary &r : rows) {
        const auto t = exact(classes, 32);
        const auto c = exact(r.cls.data(), r.cls.size()), lo = exact(r.lo.data(), r.lo.size()), hi = exact(r.hi.data(), r.hi.size());
        const auto se = exact(r.sigElem.data(), r.sigElem.size());
        const auto nb = exact(r.nb.data(), r.nb.size()), na = exact(r.na.data(), r.na.size());
        bad = -1;
        sg = nullptr;
        st = PFACX_clsigOpen(h, t.get(), 4, c.get(), lo.get(), hi.get(), se.get(), nb.get(), na.get(), r.sigElem.size() - 1, 0, 0, &sg, &bad);
        check(st == PFAC_STATUS_INVALID_PARAMETER && !sg && bad == r.bad, r.name, "a binary refusal");
    }
    const unsigned int cls[] = {0, 1, 2, 2, 0, 1}, lo[] = {1, 1, 0, 1, 1, 1}, hi[] = {1, 1, 63, 1, 1, 1};
    const size_t sigElem[] = {0, 3, 6};
    const int nb[] = {-1, 2}, na[] = {2, -1};
    check(PFACX_clsigOpen(h, nullptr, 4, cls, lo, hi, sigElem, nb, na, 2, 0, 0, &sg, &bad) == PFAC_STATUS_INVALID_PARAMETER, "null", "classes");
    check(PFACX_clsigOpen(h, classes, 4, cls, nullptr, hi, sigElem, nb, na, 2, 0, 0, &sg, &bad) == PFAC_STATUS_INVALID_PARAMETER, "null", "elemLo");
    check(PFACX_clsigOpen(h, classes, 4, cls, lo, hi, nullptr, nb, na, 2, 0, 0, &sg, &bad) == PFAC_STATUS_INVALID_PARAMETER, "null", "sigElem");
    check(PFACX_clsigOpen(h, classes, 4, cls, lo, hi, sigElem, nb, na, 0, 0, 0, &sg, &bad) == PFAC_STATUS_INVALID_PARAMETER, "null", "no signatures");
    check(PFACX_clsigOpen(h, classes, 0, cls, lo, hi, sigElem, nb, na, 2, 0, 0, &sg, &bad) == PFAC_STATUS_INVALID_PARAMETER, "null", "no classes");
    check(PFACX_clsigOpen(h, classes, 4, cls, lo, hi, sigElem, nb, na, 2, 0, 4u, &sg, &bad) == PFAC_STATUS_INVALID_PARAMETER, "null", "flags");
    check(PFACX_clsigOpen(h, classes, 4, cls, lo, hi, sigElem, nb, na, 2, 0, 0, nullptr, &bad) == PFAC_STATUS_INVALID_PARAMETER, "null", "sig");
    check(PFACX_clsigOpen(nullptr, classes, 4, cls, lo, hi, sigElem, nb, na, 2, 0, 0, &sg, &bad) == PFAC_STATUS_INVALID_HANDLE, "null", "handle");
    unsigned int emptyClass[32];
    std::memcpy(emptyClass, classes, sizeof emptyClass);
    std::memset(emptyClass + 8, 0, 32);
    check(PFACX_clsigOpen(h, emptyClass, 4, cls, lo, hi, sigElem, nb, na, 2, 0, 0, &sg, &bad) == PFAC_STATUS_INVALID_PARAMETER && bad == 0, "null",
          "an empty class");
    /* ... and the one that passes (`ab[0-9]{0,63}(?![0-9])`, `(?<![0-9])[0-9]ab`), with NULL boundary arrays too: the getter into arrays of
     * exactly S + 1 entries, the match over an input of exactly its size */
    const auto t = exact(classes, 32);
    const auto c = exact(cls, 6), l = exact(lo, 6), u = exact(hi, 6);
    const auto se = exact(sigElem, 3);
    const auto b4 = exact(nb, 2), af = exact(na, 2);
    st = PFACX_clsigOpen(h, t.get(), 4, c.get(), l.get(), u.get(), se.get(), nullptr, nullptr, 2, 0, 0, &sg, &bad);
    check(st == PFAC_STATUS_SUCCESS && sg && bad == 0, "binary", "open without boundaries");
    check(PFACX_clsigClose(sg) == PFAC_STATUS_SUCCESS, "binary", "close");
    st = PFACX_clsigOpen(h, t.get(), 4, c.get(), l.get(), u.get(), se.get(), b4.get(), af.get(), 2, 0, 0, &sg, &bad);
    check(st == PFAC_STATUS_SUCCESS && sg && bad == 0, "binary", "open");
    if (!sg) return;
    std::unique_ptr<int[]> aid(new int[3]), apart(new int[3]), aoff(new int[3]), alen(new int[3]);
    check(PFACX_clsigGetAnchors(sg, aid.get(), apart.get(), aoff.get(), alen.get(), 2) == PFAC_STATUS_INVALID_PARAMETER, "binary", "a short getter");
    check(PFACX_clsigGetAnchors(sg, aid.get(), nullptr, aoff.get(), nullptr, 3) == PFAC_STATUS_SUCCESS, "binary", "the getter with null arrays");
    check(PFACX_clsigGetAnchors(sg, aid.get(), apart.get(), aoff.get(), alen.get(), 3) == PFAC_STATUS_SUCCESS, "binary", "the getter");
    check(aid[1] == 1 && aid[2] == 1 && apart[1] == 0 && apart[2] == 1 && aoff[2] == 0 && alen[1] == 2 && alen[2] == 2, "binary", "the anchors");
    std::string text = "ab";
    text += std::string(63, '7') + " 5ab 55ab ab1";
    const auto in = exact(text.data(), text.size());
    std::unique_ptr<int[]> ids(new int[5]), pos(new int[5]), end(new int[5]);
    size_t n = 0;
    st = PFACX_clsigMatchFromHost(sg, in.get(), text.size(), ids.get(), pos.get(), end.get(), 5, &n);
    check(st == PFAC_STATUS_SUCCESS && n == 5, "binary", "the list");
    check(ids[0] == 1 && pos[0] == 0 && end[0] == 65 && ids[1] == 2 && pos[1] == 66 && end[1] == 69 && ids[2] == 1 && pos[2] == 67 && end[2] == 69 &&
              ids[3] == 1 && pos[3] == 72 && end[3] == 74 && ids[4] == 1 && pos[4] == 75 && end[4] == 78,
          "binary", "the entries");
    size_t none = 5;
    check(PFACX_clsigMatchFromHost(sg, in.get(), 0, nullptr, nullptr, nullptr, 0, &none) == PFAC_STATUS_SUCCESS && none == 0, "binary", "size 0");
    check(PFACX_clsigMatchFromDevice(sg, in.get(), text.size(), ids.get(), pos.get(), end.get(), text.size(), &n) == PFAC_STATUS_LIB_NOT_EXIST,
          "binary", "a device form on a host-only handle");
    /* left open: PFAC_destroy closes it */
}

} // namespace

int main()
{
    PFAC_handle_t h = nullptr;
    if (PFACX_createHostOnly(&h) != PFAC_STATUS_SUCCESS) return 2;
    std::string many = "K" + std::string(62, '4') + "L";
    const std::vector<Case> cases = {
        {"class-lo-hi-cut-three-ways", "k=[0-9]{2,5}\n", 0, "k=12x k=1234567 k=1 k=123", {{1, 0, 4}, {1, 6, 13}, {1, 20, 25}}},
        {"identical-signatures", "id[0-9]{1,2};\r\nid[0-9]{1,2};\n", 0, "id1; id22; id333;", {{2, 0, 4}, {1, 0, 4}, {2, 5, 10}, {1, 5, 10}}},
        {"owner-both-complete", "a.{0,2}KK.{0,2}z\n", 0, "aKKK.z", {{1, 0, 6}}},
        {"owner-nearer-dead", "a.{0,2}KK[zZ]\n", 0, "aKKKz", {{1, 0, 5}}},
        {"owner-nearer-only-to-forbidden-ends", "a.{0,2}KK.{1,2}(?![0-9])\n", 0, "aKKK12;", {{1, 0, 6}}},
        {"end-lazy-dead-end", "a.?[`-o].?[c][dD]\n", PFACX_CLSIG_SHORTEST_END, "abccd", {{1, 0, 5}}},
        {"largest-end", "k[ab]{1,3}b[c]{0,3}\n", 0, "kabbc kabc kabbbcccc", {{1, 0, 5}, {1, 6, 10}, {1, 11, 19}}},
        {"shortest-end", "k[ab]{1,3}b[c]{0,3}\n", PFACX_CLSIG_SHORTEST_END, "kabbc kabc kabbbcccc", {{1, 0, 3}, {1, 6, 9}, {1, 11, 14}}},
        {"not-before", "(?<![0-9])[0-9]{3}-x\n", 0, "123-x 9123-x a123-x", {{1, 0, 5}, {1, 14, 19}}},
        {"not-after-at-the-input-end", "tok=[a-f]{2,4}(?![a-f])\n", 0, "tok=abcdef tok=abc", {{1, 11, 18}}},
        {"slack-63-at-the-input-end", "K[0-9]{0,62}L?\n", 0, many, {{1, 0, 64}}},
        {"a-run-cut-by-the-input-end", "K[0-9]{0,62}L?\n", 0, many.substr(0, 40), {{1, 0, 40}}},
    };
    for (const Case &c : cases) runCase(h, c);
    refusals(h);
    if (PFAC_destroy(h) != PFAC_STATUS_SUCCESS) failures++;
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("clsig_host_san: %zu cases, both open calls with their refusals, the getter and the host form at every capacity: all held\n", cases.size());
    return 0;
}
