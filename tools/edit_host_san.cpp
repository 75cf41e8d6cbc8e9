/*
 * edit_host_san.cpp -- PFACX_editOpen, PFACX_editGetPieces and PFACX_editMatchFromHost on a host-only handle over the case table of
 * tests/edit_ref.py, for the sanitizer build of the host library (make -C pfac_amd/csrc san: build/edit_host_san links lib/san/libpfac.so; CPU
 * only).  Every case is opened from heap blocks of exactly their size, with and without PFACX_EDIT_BEST_ENDS, its pieces are read into arrays of
 * exactly their size and compared with the documented cut, and it runs on both CPU platforms at every capacity from 0 to the list's length + 1,
 * into arrays allocated at exactly `capacity` entries (end and distance given, or NULL) and over an input in a heap block of exactly its size --
 * a write behind the arrays or a read outside the input is the sanitizer's to find -- and is compared, as a set, with the definition: Sellers'
 * recurrence over every column, evaluated here.  Then every refusal of the open call.  Exit status 0: every list agreed.
 */
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "PFAC.h"
#include "pfac_ext.h"

namespace {

struct Case {
    const char *name;
    std::vector<std::string> patterns;
    std::vector<int> budgets;
    size_t minPiece, maxPiece;
    std::string input;
};

int failures = 0;

void check(bool ok, const char *name, const char *what, int platform)
{
    if (ok) return;
    failures++;
    std::fprintf(stderr, "FAILED %s: %s (platform %d)\n", name, what, platform);
}

using Entry = std::tuple<int, int, int, int>;        /* id, start, end, distance */

/* the definition: per pattern a column of (cost, start) per end, the lower cost first, then the larger start; every end, or the three-point rule */
std::vector<Entry> byDefinition(const Case &c, bool bestEnds)
{
    std::vector<Entry> out;
    const std::string &in = c.input;
    const size_t n = in.size();
    using Cell = std::pair<int, int>;
    const auto less = [](const Cell &a, const Cell &b) { return a.first != b.first ? a.first < b.first : a.second > b.second; };
    for (size_t i = 0; i < c.patterns.size(); i++) {
        const std::string &p = c.patterns[i];
        const size_t L = p.size();
        std::vector<Cell> D(n + 1), above(L + 1), here(L + 1);
        for (size_t col = 0; col <= n; col++) {
            here[0] = {0, (int)col};
            for (size_t r = 1; r <= L; r++) {
                Cell best = {here[r - 1].first + 1, here[r - 1].second};
                if (col > 0) {
                    const Cell diag = {above[r - 1].first + (p[r - 1] != in[col - 1]), above[r - 1].second};
                    const Cell left = {above[r].first + 1, above[r].second};
                    if (less(diag, best)) best = diag;
                    if (less(left, best)) best = left;
                }
                here[r] = best;
            }
            D[col] = here[L];
            above = here;
        }
        for (size_t e = 0; e <= n; e++) {
            if (D[e].first > c.budgets[i]) continue;
            if (bestEnds && !(e >= 1 && D[e - 1].first > D[e].first && (e == n || D[e + 1].first >= D[e].first))) continue;
            out.emplace_back((int)i + 1, D[e].second, (int)e, D[e].first);
        }
    }
    std::sort(out.begin(), out.end());
    return out;
}

PFAC_handle_t hostHandle(int platform)
{
    PFAC_handle_t h = nullptr;
    if (PFACX_createHostOnly(&h) == PFAC_STATUS_SUCCESS && PFAC_setPlatform(h, (PFAC_platform_t)platform) == PFAC_STATUS_SUCCESS) return h;
    if (h) PFAC_destroy(h);
    return nullptr;
}

/* PFACX_editOpen from heap blocks of exactly their size; offsets that start at `lead` (the CSR form need not start at 0) */
PFAC_status_t openExact(PFAC_handle_t h, const std::vector<std::string> &patterns, const std::vector<int> &budgets, size_t minPiece, size_t maxPiece,
                        unsigned int flags, PFACX_edit_t *ed, int *bad, size_t lead = 0)
{
    size_t bytes = lead;
    for (const std::string &p : patterns) bytes += p.size();
    std::unique_ptr<unsigned char[]> blob(new unsigned char[bytes ? bytes : 1]);
    std::unique_ptr<size_t[]> off(new size_t[patterns.size() + 1]);
    std::unique_ptr<int[]> budget(new int[patterns.size() ? patterns.size() : 1]);
    std::memset(blob.get(), '.', lead);
    off[0] = lead;
    for (size_t i = 0; i < patterns.size(); i++) {
        std::memcpy(blob.get() + off[i], patterns[i].data(), patterns[i].size());
        off[i + 1] = off[i] + patterns[i].size();
        budget[i] = budgets[i];
    }
    return PFACX_editOpen(h, blob.get(), off.get(), budget.get(), patterns.size(), minPiece, maxPiece, flags, ed, bad);
}

void runPieces(const Case &c, PFACX_edit_t ed, int platform)
{
    const size_t S = c.patterns.size();
    std::unique_ptr<size_t[]> off(new size_t[S + 2]);
    check(PFACX_editGetPieces(ed, off.get(), nullptr, nullptr, nullptr, 0) == PFAC_STATUS_SUCCESS, c.name, "the piece offsets", platform);
    const size_t pieces = off[S + 1];
    std::unique_ptr<int[]> id(new int[pieces]), start(new int[pieces]), len(new int[pieces]);
    check(PFACX_editGetPieces(ed, nullptr, id.get(), start.get(), len.get(), pieces) == PFAC_STATUS_SUCCESS, c.name, "the pieces", platform);
    check(PFACX_editGetPieces(ed, nullptr, id.get(), nullptr, nullptr, pieces - 1) == PFAC_STATUS_INVALID_PARAMETER, c.name, "n too small", platform);
    size_t at = 0;
    for (size_t i = 0; i < S; i++) {
        const size_t L = c.patterns[i].size(), k = (size_t)c.budgets[i];
        check(off[i + 1] == at, c.name, "the offset of a pattern's pieces", platform);
        for (size_t j = 0; j <= k; j++, at++) {
            const size_t from = j * L / (k + 1), plen = std::min((j + 1) * L / (k + 1) - from, c.maxPiece ? c.maxPiece : (size_t)32);
            check(at < pieces && (size_t)start[at] == from && (size_t)len[at] == plen && id[at] >= 1, c.name, "a piece against the documented cut", platform);
        }
    }
    check(at == pieces, c.name, "the number of pieces", platform);
}

void runCase(const Case &c, int platform, bool bestEnds)
{
    PFAC_handle_t h = hostHandle(platform);
    PFACX_edit_t ed = nullptr;
    int bad = -1;
    if (!h || openExact(h, c.patterns, c.budgets, c.minPiece, c.maxPiece, bestEnds ? PFACX_EDIT_BEST_ENDS : 0u, &ed, &bad, 3) != PFAC_STATUS_SUCCESS ||
        bad != 0) {
        check(false, c.name, "open", platform);
        if (h) PFAC_destroy(h);
        return;
    }
    runPieces(c, ed, platform);
    const std::vector<Entry> want = byDefinition(c, bestEnds);
    const size_t n = c.input.size();
    std::unique_ptr<char[]> in(new char[n ? n : 1]);
    std::memcpy(in.get(), c.input.data(), n);
    for (size_t cap = 0; cap <= want.size() + 1; cap++)
        for (int optional = 0; optional < 2; optional++) {
            std::unique_ptr<int[]> ids(cap ? new int[cap] : nullptr), pos(cap ? new int[cap] : nullptr);
            std::unique_ptr<int[]> end(cap && optional ? new int[cap] : nullptr), dist(cap && optional ? new int[cap] : nullptr);
            size_t total = 99;
            const PFAC_status_t st = PFACX_editMatchFromHost(ed, in.get(), n, ids.get(), pos.get(), end.get(), dist.get(), cap, &total);
            check(total == want.size(), c.name, "the length of the list", platform);
            check(st == (cap < want.size() ? PFACX_STATUS_OUTPUT_TRUNCATED : PFAC_STATUS_SUCCESS), c.name, "the status", platform);
            if (!optional || cap < want.size()) continue;
            std::vector<Entry> got;
            for (size_t i = 0; i < want.size(); i++) got.emplace_back(ids[i], pos[i], end[i], dist[i]);
            std::sort(got.begin(), got.end());
            check(got == want, c.name, "the list against the definition", platform);
        }
    check(std::memcmp(in.get(), c.input.data(), n) == 0, c.name, "the input was modified", platform);
    check(PFACX_editClose(ed) == PFAC_STATUS_SUCCESS, c.name, "close", platform);
    PFAC_destroy(h);
}

void runRefusals()
{
    struct Refusal { const char *why; std::vector<std::string> patterns; std::vector<int> budgets; size_t minPiece, maxPiece; unsigned int flags; int bad; };
    const std::vector<Refusal> refusals = {
        {"an empty pattern", {"abcd", "", "efgh"}, {0, 0, 0}, 0, 0, 0u, 2},
        {"65 536 bytes", {"abcd", std::string(65536, 'x')}, {0, 0}, 0, 0, 0u, 2},
        {"a budget of 8", {"abcd", std::string(64, 'x')}, {0, 8}, 0, 0, 0u, 2},
        {"a negative budget", {std::string(64, 'x')}, {-1}, 0, 0, 0u, 1},
        {"7 bytes for two pieces of 4", {"abcdefg"}, {1}, 0, 0, 0u, 1},
        {"fewer bytes than parts", {"ab"}, {2}, 1, 0, 0u, 1},
        {"0x0A in a piece", {"abcdefgh", "abcd\nfgh"}, {1, 1}, 0, 0, 0u, 2},
        {"an unknown flag", {"abcdefgh"}, {1}, 0, 0, 2u, 0},
    };
    for (const Refusal &r : refusals) {
        PFAC_handle_t h = hostHandle(PFAC_PLATFORM_CPU);
        PFACX_edit_t ed = reinterpret_cast<PFACX_edit_t>(&failures);
        int bad = -1;
        const PFAC_status_t st = h ? openExact(h, r.patterns, r.budgets, r.minPiece, r.maxPiece, r.flags, &ed, &bad) : PFAC_STATUS_INTERNAL_ERROR;
        check(st == PFAC_STATUS_INVALID_PARAMETER && bad == r.bad && ed == nullptr, r.why, "the refusal", 0);
        if (h) PFAC_destroy(h);
    }
}

} // namespace

int main()
{
    const std::vector<Case> cases = {
        {"one-substitution", {"abcdefgh"}, {1}, 0, 0, "__abcXefgh__"},
        {"one-insertion", {"abcdefgh"}, {1}, 0, 0, "__abcdXefgh__"},
        {"one-deletion", {"abcdefgh"}, {1}, 0, 0, "__abcefgh__"},
        {"exact-copy-k2", {"abcdefghijkl"}, {2}, 0, 0, "__abcdefghijkl__"},
        {"abab", {"abababab"}, {1}, 0, 0, "__abababab__"},
        {"not-sorted-by-start", {"abcdefgh", "cdef"}, {1, 0}, 0, 0, "_aXcdefgh_"},
        {"identical-patterns", {"wxyzwxyz", "wxyzwxyz"}, {0, 1}, 0, 0, "wxyzwxyz"},
        {"starts-at-0-ends-at-n", {"mnopqrstuvwx"}, {2}, 0, 0, "nopqrstuvw"},
        {"short-pieces", {"abc", "ab"}, {2, 1}, 1, 0, "xabcxacxbx"},
        {"long-piece-first", {"abcdefgh", "abcd"}, {0, 0}, 0, 0, "..abcdefgh..abcd"},
        {"seven-edits", {"ABCDEFGHIJKLMNOPQRSTUVWXYZ012345"}, {7}, 0, 0, "..ABCEFGHIJKKLMNOPRSTUVWXYZ0l2345ABCDEFGHIJKLMNOPQRSTUVWXYZ01234"},
    };
    for (const Case &c : cases)
        for (int platform : {(int)PFAC_PLATFORM_CPU, (int)PFAC_PLATFORM_CPU_OMP})
            for (int best = 0; best < 2; best++) runCase(c, platform, best != 0);
    runRefusals();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("edit_host_san: %zu cases on 2 platforms, with and without PFACX_EDIT_BEST_ENDS, and the refusals: all agreed\n", cases.size());
    return 0;
}
