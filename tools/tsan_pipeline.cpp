/* tools/tsan_pipeline.cpp -- the thread protocol of a host call on the GPU platform (pfac_amd/csrc/piece_pipeline.h: runPieces, ZeroFill) under
 * ThreadSanitizer, with fake stages in place of the HIP calls (`make -C pfac_amd/csrc build/tsan_pipeline`; no library, no GPU): the order the stages
 * run in, what a failure at each of them does, and the zero fill beside a consumer.  That the program ends is the proof that every call joined its
 * threads.   tsan_pipeline [seed] */
#include <chrono>
#include <random>

#include "piece_pipeline.h"

using namespace pfac_internal;

namespace {

int g_checks = 0, g_failed = 0;
void check(bool ok, const char *what, size_t pieces, int stage, size_t at)
{
    g_checks++;
    if (ok) return;
    g_failed++;
    std::fprintf(stderr, "FAILED: %s (%zu pieces, failure at stage %d of piece %zu)\n", what, pieces, stage, at);
}

enum Stage { kNone, kInit, kUpload, kScan, kTake, kTakeThrows };
const PFAC_status_t kScanStatus = PFAC_STATUS_CUDA_ALLOC_FAILED, kTakeStatus = PFAC_STATUS_INVALID_PARAMETER;    /* a stage's own status comes back */

/* a few hundred microseconds, now and then; one generator per thread role (the uploader's stages, the caller's stages) */
struct Jitter {
    std::mt19937 rng;
    explicit Jitter(unsigned seed) : rng(seed) {}
    void operator()() { if (rng() % 3 == 0) std::this_thread::sleep_for(std::chrono::microseconds(100 + rng() % 400)); }
};

/* one call of runPieces over `pieces` fake pieces; the stage `failAt` of piece `at` fails (kNone: none does) */
void pipelineCase(size_t pieces, Stage failAt, size_t at, unsigned seed)
{
    std::atomic<int> clock{0};                                 /* sequence numbers: what happened before what */
    std::vector<int> uploadBegan(pieces, 0), scanEnded(pieces, 0), scans(pieces, 0), takes(pieces, 0);
    std::vector<size_t> uploadOrder, callerOrder;              /* written by one thread each, read after the call */
    std::thread::id uploadThread[2];                           /* of upload(0), of threadInit */
    int inits = 0, beguns = 0;
    Jitter upJitter(seed), callJitter(seed + 1);
    const PFAC_status_t st = runPieces(
        pieces,
        [&]() { inits++; uploadThread[1] = std::this_thread::get_id(); upJitter(); return failAt != kInit; },
        [&](size_t i) {
            uploadBegan[i] = ++clock;
            if (i == 0) uploadThread[0] = std::this_thread::get_id();
            uploadOrder.push_back(i);
            upJitter();
            return !(failAt == kUpload && i == at);
        },
        [&]() { beguns++; },
        [&](size_t i) {
            callJitter();
            scans[i]++;
            callerOrder.push_back(2 * i);
            callJitter();
            scanEnded[i] = ++clock;
            return failAt == kScan && i == at ? kScanStatus : PFAC_STATUS_SUCCESS;
        },
        [&](size_t i) {
            takes[i]++;
            callerOrder.push_back(2 * i + 1);
            callJitter();
            if (failAt == kTakeThrows && i == at) throw std::bad_alloc();
            return failAt == kTake && i == at ? kTakeStatus : PFAC_STATUS_SUCCESS;
        });
    auto ck = [&](bool ok, const char *what) { check(ok, what, pieces, (int)failAt, at); };
    const PFAC_status_t want = failAt == kNone ? PFAC_STATUS_SUCCESS : failAt == kInit || failAt == kUpload ? PFAC_STATUS_INTERNAL_ERROR
                             : failAt == kScan ? kScanStatus : failAt == kTake ? kTakeStatus : PFAC_STATUS_ALLOC_FAILED;
    ck(st == want, "the status that comes back");
    ck(beguns == 1, "begun() runs once");
    ck(inits == (pieces > 1 ? 1 : 0), "threadInit runs once on the uploader, never without one");
    for (size_t k = 0; k < uploadOrder.size(); k++) ck(uploadOrder[k] == k, "uploads happen in order");
    for (size_t k = 0; k < callerOrder.size(); k++) ck(callerOrder[k] == k, "scan(0), take(0), scan(1), take(1), ... in order, each once");
    for (size_t i = 2; i < pieces; i++)
        if (uploadBegan[i]) ck(scanEnded[i - 2] != 0 && scanEnded[i - 2] < uploadBegan[i], "upload(i) starts after scan(i - 2) has returned");
    if (pieces == 1) ck(uploadThread[0] == std::this_thread::get_id(), "one piece: upload(0) on the calling thread");
    else if (!uploadOrder.empty()) ck(uploadThread[0] != std::this_thread::get_id() && uploadThread[0] == uploadThread[1], "several pieces: the uploads on the thread that threadInit ran on");
    if (failAt == kNone) {
        ck(uploadOrder.size() == pieces && callerOrder.size() == 2 * pieces, "every piece uploaded, scanned and taken");
        return;
    }
    /* nothing of a later piece runs, nor the rest of the failing one */
    const size_t scansWanted = failAt == kInit ? 0 : failAt == kUpload ? at : at + 1;         /* at most (an upload fails while earlier pieces are under way) */
    const size_t takesWanted = failAt == kInit ? 0 : failAt == kUpload || failAt == kScan ? at : at + 1;
    size_t scanned = 0, taken = 0;
    for (size_t i = 0; i < pieces; i++) { scanned += (size_t)scans[i]; taken += (size_t)takes[i]; }
    if (failAt == kInit || failAt == kUpload) ck(scanned <= scansWanted && taken <= takesWanted && taken == scanned, "no scan or take at or behind a failed upload");
    else ck(scanned == scansWanted && taken == takesWanted, "no scan or take behind a failed stage");
    if (failAt == kInit) ck(uploadOrder.empty(), "no upload behind a failed threadInit");
}

/* the zero fill of a vector of n ints in `pieces` pieces with `helpers` threads, beside a consumer that writes one word of a piece once it is filled */
void zeroFillCase(size_t n, size_t pieces, unsigned helpers, unsigned seed)
{
    std::vector<int> v(n, -7);
    const PieceCut cut(n, n, (n + pieces - 1) / pieces, 0);
    auto ck = [&](bool ok, const char *what) { check(ok, what, pieces, (int)helpers, 0); };
    ck(cut.numPieces() == pieces, "the cut has the pieces asked for");
    Jitter jitter(seed);
    ZeroFill fill(v.data(), cut, helpers);
    fill.start();
    ck(fill.started() == helpers, "every helper started");
    for (size_t k = 0; k < pieces; k++) {
        jitter();
        const Piece p = cut.at(k);
        fill.waitFilled(k);
        bool zero = true;
        for (size_t i = 0; i < p.mine; i++) zero = zero && v[p.off + i] == 0;
        ck(zero, "after waitFilled(k) piece k is all zero");
        v[p.off + p.mine / 2] = 100 + (int)k;                  /* what a take scatters */
    }
    fill.finish();
    bool rest = true;
    for (size_t k = 0; k < pieces; k++) {
        const Piece p = cut.at(k);
        for (size_t i = 0; i < p.mine; i++) rest = rest && v[p.off + i] == (i == p.mine / 2 ? 100 + (int)k : 0);
    }
    ck(rest, "after finish() the scattered words survive and every other word is zero");
}

void cutCase()
{
    auto ck = [&](bool ok, const char *what) { check(ok, what, 0, 0, 0); };
    const PieceCut cut(70, 75, 32, 8);                         /* three pieces, the last ragged, 5 bytes of read-ahead behind the stream */
    const Piece a = cut.at(0), b = cut.at(1), c = cut.at(2);
    ck(cut.numPieces() == 3 && cut.stageNeed() == 40, "70 positions in pieces of 32");
    ck(a.off == 0 && a.mine == 32 && a.scanned == 40 && a.buffer == 0, "piece 0");
    ck(b.off == 32 && b.mine == 32 && b.scanned == 40 && b.buffer == 1 && b.index == 1, "piece 1");
    ck(c.off == 64 && c.mine == 6 && c.scanned == 11 && c.buffer == 0, "piece 2: the read-ahead ends with the readable bytes");
    const PieceCut whole(64, 64, 32, 8), small(5, 5, 32, 8);
    ck(whole.numPieces() == 2 && whole.at(1).mine == 32 && whole.at(1).scanned == 32, "two whole pieces: the last has no read-ahead");
    ck(small.numPieces() == 1 && small.piece == 5 && small.at(0).scanned == 5 && small.stageNeed() == 13, "a stream shorter than a piece is one piece");
}

} // namespace

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 20261018u;
    unsigned round = 0;
    cutCase();
    for (int repeat = 0; repeat < 3; repeat++)
        for (size_t pieces : {size_t(1), size_t(2), size_t(3), size_t(7)}) pipelineCase(pieces, kNone, 0, seed + 2 * round++);
    for (int repeat = 0; repeat < 2; repeat++) {
        const size_t pieces = 7, last = pieces - 1;
        pipelineCase(pieces, kInit, 0, seed + 2 * round++);
        for (size_t at : {size_t(0), size_t(1), size_t(3)}) pipelineCase(pieces, kUpload, at, seed + 2 * round++);
        for (size_t at : {size_t(0), size_t(2), last}) pipelineCase(pieces, kScan, at, seed + 2 * round++);
        pipelineCase(pieces, kTake, 1, seed + 2 * round++);
        for (size_t at : {size_t(0), size_t(4), last}) pipelineCase(pieces, kTakeThrows, at, seed + 2 * round++);
        pipelineCase(1, kUpload, 0, seed + 2 * round++);       /* the one-piece shortcut: no thread to stop */
        pipelineCase(1, kScan, 0, seed + 2 * round++);
        pipelineCase(1, kTakeThrows, 0, seed + 2 * round++);
    }
    for (unsigned helpers : {0u, 1u, 3u}) zeroFillCase(100003, 4, helpers, seed + 2 * round++);
    std::printf("tsan_pipeline: seed %u, %u cases, %d checks, %d failed\n", seed, round, g_checks, g_failed);
    return g_failed ? 1 : 0;
}
