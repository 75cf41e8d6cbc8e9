/*
 * sig_host_san.cpp -- PFACX_sigOpen, PFACX_sigOpenText and PFACX_sigMatchFromHost on a host-only handle over the case table of tests/sig_ref.py,
 * for the sanitizer build of the host library (make -C pfac_amd/csrc san: build/sig_host_san links lib/san/libpfac.so; CPU only).  Every case is
 * opened through both calls from heap blocks of exactly their size, runs on both CPU platforms at every capacity from 0 to the list's length + 1,
 * into arrays allocated at exactly `capacity` entries and over an input in a heap block of exactly its size -- a write behind the arrays or a read
 * behind the input is the sanitizer's to find -- and is compared with the definition, evaluated here start by start and signature by signature and
 * ordered by what PFACX_sigGetAnchors says.  Then the refusals of both open calls.  Exit status 0: every list agreed.
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

#define LIT(s) std::string(s, sizeof(s) - 1)   /* a literal with zero bytes in it */

struct Sig { std::vector<unsigned char> v, m; };

struct Case {
    const char *name;
    std::vector<std::string> lines;             /* the text form, one signature per entry */
    std::string input;
};

int failures = 0;

void check(bool ok, const char *name, const char *what, int platform)
{
    if (ok) return;
    failures++;
    std::fprintf(stderr, "FAILED %s: %s (platform %d)\n", name, what, platform);
}

/* a line the table holds: pairs of hex digits or '?', blanks between them */
Sig parseLine(const std::string &line)
{
    const auto nib = [](char c) { return c == '?' ? 16 : c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10; };
    Sig s;
    for (size_t j = 0; j + 1 < line.size();) {
        if (line[j] == ' ') { j++; continue; }
        const int hi = nib(line[j]), lo = nib(line[j + 1]);
        s.v.push_back((unsigned char)((hi < 16 ? hi << 4 : 0) | (lo < 16 ? lo : 0)));
        s.m.push_back((unsigned char)((hi < 16 ? 0xF0 : 0) | (lo < 16 ? 0x0F : 0)));
        j += 2;
    }
    return s;
}

std::string hexLine(const Sig &s)
{
    static const char digits[] = "0123456789ABCDEF";
    std::string out;
    for (size_t k = 0; k < s.v.size(); k++) {
        if (k) out += ' ';
        out += (s.m[k] & 0xF0) ? digits[(s.v[k] & s.m[k]) >> 4] : '?';
        out += (s.m[k] & 0x0F) ? digits[s.v[k] & s.m[k] & 15] : '?';
    }
    return out;
}

/* the definition, ordered by the contract with the library's own anchors: (id, start) */
std::vector<std::pair<int, int>> byDefinition(const std::vector<Sig> &sigs, const std::string &in, const std::vector<int> &anchorOff,
                                              const std::vector<int> &anchorLen)
{
    std::vector<std::tuple<int, int, int, int>> found;          /* anchor position, -anchor length, -id, start */
    for (size_t i = 0; i < sigs.size(); i++) {
        const Sig &s = sigs[i];
        for (size_t at = 0; at + s.v.size() <= in.size(); at++) {
            size_t k = 0;
            while (k < s.v.size() && (((unsigned char)in[at + k] ^ s.v[k]) & s.m[k]) == 0) k++;
            if (k == s.v.size()) found.emplace_back((int)at + anchorOff[i + 1], -anchorLen[i + 1], -(int)(i + 1), (int)at);
        }
    }
    std::sort(found.begin(), found.end());
    std::vector<std::pair<int, int>> out;
    for (const auto &f : found) out.emplace_back(-std::get<2>(f), std::get<3>(f));
    return out;
}

PFAC_handle_t hostHandle(int platform)
{
    PFAC_handle_t h = nullptr;
    if (PFACX_createHostOnly(&h) == PFAC_STATUS_SUCCESS && PFAC_setPlatform(h, (PFAC_platform_t)platform) == PFAC_STATUS_SUCCESS) return h;
    if (h) PFAC_destroy(h);
    return nullptr;
}

void runLists(const Case &c, const std::vector<Sig> &sigs, PFACX_sig_t sg, int platform)
{
    const size_t S = sigs.size(), n = c.input.size();
    std::unique_ptr<int[]> anchorId(new int[S + 1]), anchorOff(new int[S + 1]), anchorLen(new int[S + 1]);      /* exactly S + 1 entries */
    check(PFACX_sigGetAnchors(sg, anchorId.get(), anchorOff.get(), anchorLen.get(), S + 1) == PFAC_STATUS_SUCCESS, c.name, "the getter", platform);
    check(PFACX_sigGetAnchors(sg, anchorId.get(), anchorOff.get(), anchorLen.get(), S) == PFAC_STATUS_INVALID_PARAMETER, c.name, "the getter with n = S", platform);
    const std::vector<int> off(anchorOff.get(), anchorOff.get() + S + 1), len(anchorLen.get(), anchorLen.get() + S + 1);
    for (size_t i = 1; i <= S; i++) {                            /* an anchor is a fully specified run inside its signature */
        bool ok = anchorId[i] >= 1 && off[i] >= 0 && len[i] >= 1 && (size_t)(off[i] + len[i]) <= sigs[i - 1].v.size();
        for (int k = 0; ok && k < len[i]; k++) ok = sigs[i - 1].m[(size_t)(off[i] + k)] == 0xFF && sigs[i - 1].v[(size_t)(off[i] + k)] != 0x0A;
        check(ok, c.name, "an anchor", platform);
    }
    const std::vector<std::pair<int, int>> want = byDefinition(sigs, c.input, off, len);
    check(!want.empty(), c.name, "the case has no occurrence", platform);
    for (size_t capacity = 0; capacity <= want.size() + 1; capacity++) {
        std::unique_ptr<char[]> input(new char[n]);              /* exactly n bytes */
        std::memcpy(input.get(), c.input.data(), n);
        std::unique_ptr<int[]> ids(new int[capacity]), pos(new int[capacity]);
        std::fill(ids.get(), ids.get() + capacity, -7);
        std::fill(pos.get(), pos.get() + capacity, -7);
        size_t total = 12345;
        const PFAC_status_t st = PFACX_sigMatchFromHost(sg, input.get(), n, capacity ? ids.get() : nullptr, capacity ? pos.get() : nullptr, capacity, &total);
        check(st == (want.size() > capacity ? PFACX_STATUS_OUTPUT_TRUNCATED : PFAC_STATUS_SUCCESS), c.name, "the status", platform);
        check(total == want.size(), c.name, "the length of the list", platform);
        check(std::memcmp(input.get(), c.input.data(), n) == 0, c.name, "the caller's bytes", platform);
        for (size_t k = 0; k < capacity; k++) {
            const bool listed = k < want.size();
            check(listed ? (ids[k] == want[k].first && pos[k] == want[k].second) : (ids[k] == -7 && pos[k] == -7), c.name, "an entry", platform);
        }
    }
}

void runCase(const Case &c)
{
    std::vector<Sig> sigs;
    std::string text;
    for (const std::string &line : c.lines) {
        sigs.push_back(parseLine(line));
        text += line + "\n";
    }
    for (int platform : {PFAC_PLATFORM_CPU, PFAC_PLATFORM_CPU_OMP}) {
        PFAC_handle_t h = hostHandle(platform);
        if (!h) { check(false, c.name, "the handle", platform); continue; }
        PFACX_sig_t sg = nullptr;
        int bad = -1;
        {   /* the text in a heap block of exactly its size: the open call copies what it keeps */
            std::unique_ptr<char[]> block(new char[text.size()]);
            std::memcpy(block.get(), text.data(), text.size());
            check(PFACX_sigOpenText(h, block.get(), text.size(), 0, &sg, &bad) == PFAC_STATUS_SUCCESS && sg && bad == 0, c.name, "the text open call", platform);
        }
        if (sg) {
            runLists(c, sigs, sg, platform);
            check(PFACX_sigClose(sg) == PFAC_STATUS_SUCCESS, c.name, "the close call", platform);
        }
        sg = nullptr;
        {   /* the binary form from blocks of exactly their sizes, values with stray bits outside their masks */
            size_t bytes = 0;
            for (const Sig &s : sigs) bytes += s.v.size();
            std::unique_ptr<unsigned char[]> values(new unsigned char[bytes]), masks(new unsigned char[bytes]);
            std::unique_ptr<size_t[]> off(new size_t[sigs.size() + 1]);
            off[0] = 0;
            for (size_t i = 0, at = 0; i < sigs.size(); i++) {
                for (size_t k = 0; k < sigs[i].v.size(); k++, at++) {
                    masks[at] = sigs[i].m[k];
                    values[at] = (unsigned char)(sigs[i].v[k] | (~sigs[i].m[k] & 0xA5));
                }
                off[i + 1] = at;
            }
            check(PFACX_sigOpen(h, values.get(), masks.get(), off.get(), sigs.size(), 0, &sg, &bad) == PFAC_STATUS_SUCCESS && sg && bad == 0, c.name,
                  "the binary open call", platform);
        }
        if (sg) runLists(c, sigs, sg, platform);                /* left open: PFAC_destroy closes it */
        PFAC_destroy(h);
    }
}

void runRefusals()
{
    PFAC_handle_t h = hostHandle(PFAC_PLATFORM_CPU);
    PFACX_sig_t sg = nullptr;
    int bad = -1;
    const auto text = [&](const std::string &t) {
        std::unique_ptr<char[]> block(new char[t.size() ? t.size() : 1]);
        std::memcpy(block.get(), t.data(), t.size());
        bad = -1;
        const PFAC_status_t st = PFACX_sigOpenText(h, block.get(), t.size(), 0, &sg, &bad);
        return st == PFAC_STATUS_INVALID_PARAMETER && !sg ? bad : -2;
    };
    bool ok = h != nullptr;
    ok = ok && text("41\n\n42\n") == 2 && text("41\n \t\n") == 2 && text("41 4\n") == 1 && text("41\n4 1\n") == 2 && text("41\n4G\n") == 2;
    ok = ok && text("41\r 42\n") == 1 && text("41\n42") == 2 && text("41\n42\n ") == 3 && text("41\n??\n") == 2 && text("0A\n") == 1;
    ok = ok && text("") == 0 && text("?") == 1 && text("4") == 1 && text("\n") == 1 && text("\r\n") == 1;
    const auto binary = [&](std::vector<unsigned char> v, std::vector<unsigned char> m, std::vector<size_t> off) {
        bad = -1;
        const PFAC_status_t st = PFACX_sigOpen(h, v.data(), m.data(), off.data(), off.size() - 1, 0, &sg, &bad);
        return st == PFAC_STATUS_INVALID_PARAMETER && !sg ? bad : -2;
    };
    ok = ok && binary({1, 2, 3}, {255, 255, 255}, {0, 1, 1, 3}) == 2 && binary({1, 2, 3}, {255, 255, 255}, {0, 2, 1, 3}) == 2;
    ok = ok && binary({1, 2, 3}, {255, 0xF0, 255}, {0, 1, 2, 3}) == 2 && binary({1, 0x0A, 3}, {255, 255, 255}, {0, 1, 2, 3}) == 2;
    ok = ok && binary(std::vector<unsigned char>(65537, 0x41), std::vector<unsigned char>(65537, 0xFF), {0, 1, 65537}) == 2;
    const unsigned char one[1] = {0x41}, full[1] = {0xFF};
    const size_t off[2] = {0, 1};
    ok = ok && PFACX_sigOpen(h, one, full, off, 0, 0, &sg, &bad) == PFAC_STATUS_INVALID_PARAMETER && bad == 0;
    ok = ok && PFACX_sigOpen(h, nullptr, full, off, 1, 0, &sg, nullptr) == PFAC_STATUS_INVALID_PARAMETER;
    ok = ok && PFACX_sigOpen(h, one, full, off, 1, 0, nullptr, nullptr) == PFAC_STATUS_INVALID_PARAMETER;
    ok = ok && PFACX_sigOpen(nullptr, one, full, off, 1, 0, &sg, nullptr) == PFAC_STATUS_INVALID_HANDLE;
    ok = ok && PFACX_sigOpen(h, one, full, off, 1, 0, &sg, nullptr) == PFAC_STATUS_SUCCESS && sg;
    if (ok) {                                                    /* stale after a re-read; closed by PFAC_destroy */
        char input[] = "xAxA";
        int ids[4], pos[4];
        size_t total = 0;
        ok = PFACX_sigMatchFromHost(sg, input, 4, ids, pos, 4, &total) == PFAC_STATUS_SUCCESS && total == 2 && ids[0] == 1 && pos[0] == 1 && pos[1] == 3;
        ok = ok && PFACX_sigMatchFromDevice(sg, input, 4, ids, pos, 4, &total) == PFAC_STATUS_LIB_NOT_EXIST;
        ok = ok && PFACX_readPatternFromMemory(h, "A\n", 2) == PFAC_STATUS_SUCCESS;
        ok = ok && PFACX_sigMatchFromHost(sg, input, 4, ids, pos, 4, &total) == PFAC_STATUS_INVALID_PARAMETER;
        ok = ok && PFACX_sigGetAnchors(sg, ids, pos, nullptr, 4) == PFAC_STATUS_INVALID_PARAMETER;
    }
    if (!ok) { std::fprintf(stderr, "FAILED: the refusals of the open calls or the stale object (last badSig / badLine %d)\n", bad); failures++; }
    if (h) PFAC_destroy(h);
}

/* tests/sig_ref.py: edge_signature, edge_lines, edge_input */
const int kEdgeLengths[] = {1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 64};
const int kEdges = 11;

Sig edgeSignature(int k, int kind)                              /* kind: 0 exact, 1 first, 2 last, 3 but-anchor, 4 middle, 5 halves */
{
    const int length = kEdgeLengths[k];
    Sig s;
    s.v.push_back((unsigned char)(0x41 + k));
    for (int i = 1; i < length; i++) s.v.push_back((unsigned char)(0x80 + (7 * i + 13 * k) % 0x70));
    s.m.assign((size_t)length, 0xFF);
    if (kind == 1 && length > 1) s.m[0] = 0;
    if (kind == 2 && length > 1) s.m[(size_t)length - 1] = 0;
    if (kind == 3) std::fill(s.m.begin() + 1, s.m.end(), 0);
    if (kind == 4) { std::fill(s.m.begin(), s.m.end(), 0); s.m[(size_t)length / 2] = 0xFF; }
    if (kind == 5 && length > 1) { s.m[0] = 0xF0; s.m[(size_t)length - 1] = 0x0F; }
    return s;
}

std::string bytesOf(const Sig &s) { return std::string(s.v.begin(), s.v.end()); }

std::string edgeInput()
{
    std::string out;
    for (int k = 0; k < kEdges; k++) {
        const std::string v = bytesOf(edgeSignature(k, 0));
        std::string last = v, first = v;
        last[last.size() - 1] = (char)(last[last.size() - 1] ^ 0x01);
        first[0] = (char)(first[0] ^ 0x10);
        out += v + " " + last + " " + first + " " + std::string((size_t)(k % 3), '-') + " ";
    }
    const std::string longest = bytesOf(edgeSignature(kEdges - 1, 0));
    return out + longest.substr(0, longest.size() - 1) + " " + bytesOf(edgeSignature(9, 0));
}

} // namespace

int main()
{
    std::vector<std::string> edges;
    for (int k = 0; k < kEdges; k++)
        for (int kind = 0; kind < 6; kind++) edges.push_back(hexLine(edgeSignature(k, kind)));
    const std::vector<Case> cases = {
        {"mz-pe", {"4D 5A ?? ?? 50 45 00 00"}, LIT("MZ\x90\x00PE\x00\x00 MZxyPE\x00\x01 MZPE\x00\x00 xMZ\n\nPE\x00\x00")},
        {"call-pop-ret", {"E8 ?? ?? ?? ?? 5? C3"},
         LIT("\xe8\x01\x02\x03\x04\x5b\xc3 \xe8\xe8\xe8\xe8\xe8\x5f\xc3\xc3 \xe8\x00\x00\x00\x00\x6b\xc3 \xe8\x00\x00\x00\x00\x50\xc2")},
        {"text-rule", {"69 64 3D ?? ?? ?? ?? 3B"}, "id=1234; id=12345; id=;;;;; xid=\n\r\t ;id=123;"},
        {"both-halves", {"4? ?1 41", "?1 4? 41"}, "AAA OQA QOA Oa A\x11" "A\x41\x41 \x41\x4f" "A"},
        {"anchor-in-the-middle", {"?? ?? 61 62 63 ?? ??"}, "abc..xabc..xxabc..xxxabcxxabcxxabc.abcx"},
        {"newline-outside-the-anchor", {"0A 61 62 0A", "61 62 0A 0A 63"}, "\nab\n ab\n\nc \nab \nab\n\nc xab\n"},
        {"only-newline-neighbours", {"0A 0A 41 0A"}, "\n\nA\n \n\nA \nA\n\n\nA\n"},
        {"an-anchor-is-a-prefix-of-another", {"61 62 ?? 64", "61 62 63 ??", "?? 61 62 63", "61 62 63"}, "abcd abxd abc xabc abcabcd"},
        {"identical-signatures", {"61 ?? 63", "61 ?? 63"}, "abc axc"},
        {"one-anchor-at-several-offsets", {"?? ?? 61 62", "61 62 ??", "?? 61 62"}, "xxabyab"},
        {"single-bytes", {"61", "62", "61"}, "abab"},
        {"equal-runs-the-leftmost-wins", {"61 62 ?? 63 64", "?? 63 64 ?? 61 62"}, "abxcd cdxab xcdxab abcd"},
        {"a-half-byte-splits-a-run", {"61 62 6? 64 65 66"}, "abcdef abxdef abkdef abCdef"},
        {"compare-edges", edges, edgeInput()},
    };
    for (const Case &c : cases) runCase(c);
    {   /* the list of the header that is not sorted by start */
        const std::vector<Sig> sigs = {parseLine("?? ?? 61 62"), parseLine("61 62 ??"), parseLine("?? 61 62")};
        const std::vector<std::pair<int, int>> want = {{3, 1}, {2, 2}, {1, 0}, {3, 4}, {1, 3}};
        if (byDefinition(sigs, "xxabyab", {0, 2, 0, 1}, {0, 2, 2, 2}) != want) { std::fprintf(stderr, "FAILED: the definition itself\n"); failures++; }
    }
    runRefusals();
    if (failures) return 1;
    std::printf("sig_host_san: %zu cases x 2 platforms x 2 open calls x every capacity agree with the definition; the open calls refuse what they must\n",
                cases.size());
    return 0;
}
