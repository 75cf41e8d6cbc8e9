/*
 * piece_pipeline.h -- how the threads of ONE host call work together (host_pipeline.cpp: PFAC_matchFromHost and PFAC_matchFromHostReduce on the GPU
 * platform), without a word of HIP: the cut of a stream into pieces (PieceCut), the uploader thread beside the caller's scans (runPieces), the team
 * that writes the zeros of the caller's result vector meanwhile (ZeroFill), and what they wait for each other on (Progress).  Header only, so that
 * tools/tsan_pipeline.cpp drives the same protocol with fake stages under ThreadSanitizer on a machine without a GPU.
 */
#ifndef PFAC_PIECE_PIPELINE_H_
#define PFAC_PIECE_PIPELINE_H_

#include <pthread.h>
#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>

#if defined(__SSE2__)
#include <emmintrin.h>
#endif

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "PFAC.h"

namespace pfac_internal {

/* The threads of a host call wait for each other's progress -- the uploader for a scanned buffer, the caller for an upload to be queued and for
 * a piece of its vector to be filled -- on a condition variable: round 5 spun on std::this_thread::yield(), which on a host whose cores are all
 * busy (the zero fill runs up to eight threads beside the DMA engine's reads) takes the very cores the fill threads need.  Progress counters stay
 * atomics (the fast path is one acquire load); whoever advances one calls bump(). */
struct Progress {
    std::mutex m;
    std::condition_variable cv;
    void bump() { { std::lock_guard<std::mutex> g(m); } cv.notify_all(); }
    template <class Pred> void wait(Pred done)
    {
        if (done()) return;
        std::unique_lock<std::mutex> g(m);
        cv.wait(g, done);
    }
};

/* A stream of which positions [0, owned) get results and `readable` >= owned bytes may be read, in pieces of pieceSize positions (one piece of
 * `owned` if that is less).  Piece i owns `mine` positions from `off` and is scanned together with the `overlap` bytes behind it -- a walk may
 * read that far -- as far as they are readable; it goes through staging buffer i & 1. */
struct Piece { size_t index, off, mine, scanned; int buffer; };
struct PieceCut {
    size_t owned, readable, piece, overlap;
    PieceCut(size_t owned_, size_t readable_, size_t pieceSize, size_t overlap_)
        : owned(owned_), readable(readable_), piece(owned_ < pieceSize ? owned_ : pieceSize), overlap(overlap_) {}
    size_t numPieces() const { return piece ? (owned + piece - 1) / piece : 0; }
    size_t stageNeed() const { return piece + overlap; }        /* bytes of the longest piece with its read-ahead */
    Piece at(size_t i) const
    {
        const size_t off = i * piece;
        const size_t mine = owned - off < piece ? owned - off : piece;
        const size_t scanned = readable - off < mine + overlap ? readable - off : mine + overlap;
        return {i, off, mine, scanned, (int)(i & 1)};
    }
};

/*
 * The pipeline of a host call: pieces 0 .. numPieces - 1 go through two input buffers, piece i through buffer i & 1.
 *   upload(i) -> bool    queues the upload of piece i; called for i = 0, 1, ... in order by a thread of its own, which calls threadInit() -> bool
 *                        first (the uploads are queued by a thread of their own because queueing one from PAGEABLE memory does not return until
 *                        the runtime has staged the piece, and the caller's thread has the scans to launch and their pairs to fetch meanwhile).
 *                        upload(i), i >= 2, does not start before scan(i - 2) has returned: that scan read the buffer.  One piece has nothing to
 *                        overlap with: no thread, upload(0) runs on the caller's (tens of microseconds of a small call);
 *   begun()              once on the caller's thread, when the uploads are under way (the link first) and before the first piece is waited for;
 *   scan(i), take(i)     -> PFAC_status_t, on the caller's thread, once upload i is queued.  scan(i) is synchronous: when it returns its input
 *                        buffer may take piece i + 2, so the uploader goes on while take(i) fetches the pairs.
 * Nothing further is started after a failure, and the first one is what comes back: INTERNAL_ERROR for threadInit, an upload or a thread that
 * could not be started, ALLOC_FAILED for a std::bad_alloc out of scan or take, otherwise the stage's own status.  No thread of the call is left
 * running when this returns or throws.
 */
template <class Init, class Upload, class Begun, class Scan, class Take>
PFAC_status_t runPieces(size_t numPieces, Init threadInit, Upload upload, Begun begun, Scan scan, Take take)
{
    std::atomic<size_t> scansDone{0}, uploadsQueued{0};
    std::atomic<bool> uploadFailed{false}, stopUploads{false};
    Progress progress;
    std::thread uploader;
    struct JoinOnExit {
        std::atomic<bool> &stop; Progress &progress; std::thread &t;
        ~JoinOnExit() { stop.store(true); progress.bump(); if (t.joinable()) t.join(); }
    } joinOnExit{stopUploads, progress, uploader};
    if (numPieces == 1) {
        if (upload(0)) uploadsQueued.store(1); else uploadFailed.store(true);
    } else {
        try {
            uploader = std::thread([&]() {
                if (!threadInit()) { uploadFailed.store(true); progress.bump(); return; }
                for (size_t i = 0; i < numPieces; i++) {
                    if (i >= 2) progress.wait([&]() { return scansDone.load(std::memory_order_acquire) + 1 >= i || stopUploads.load(std::memory_order_relaxed); });
                    if (stopUploads.load(std::memory_order_relaxed)) return;
                    if (!upload(i)) { uploadFailed.store(true); progress.bump(); return; }
                    uploadsQueued.store(i + 1, std::memory_order_release);
                    progress.bump();
                }
            });
        } catch (...) { uploadFailed.store(true); }
    }
    begun();
    PFAC_status_t st = PFAC_STATUS_SUCCESS;
    try {
        for (size_t i = 0; i < numPieces && st == PFAC_STATUS_SUCCESS; i++) {
            progress.wait([&]() { return uploadsQueued.load(std::memory_order_acquire) > i || uploadFailed.load(std::memory_order_relaxed); });
            if (uploadFailed.load(std::memory_order_relaxed)) { st = PFAC_STATUS_INTERNAL_ERROR; break; }
            st = scan(i);
            if (st != PFAC_STATUS_SUCCESS) break;
            scansDone.store(i + 1, std::memory_order_release);
            progress.bump();
            st = take(i);
        }
    } catch (const std::bad_alloc &) { st = PFAC_STATUS_ALLOC_FAILED; }
    return st;
}

/* The NUMA node a host page lives on (-1: unknown, not faulted in yet, or no such system call): move_pages with no target only reports. */
inline int numaNodeOf(const void *p)
{
#if defined(__linux__) && defined(SYS_move_pages)
    void *page = reinterpret_cast<void *>(reinterpret_cast<uintptr_t>(p) & ~uintptr_t(4095));
    int status = -1;
    if (syscall(SYS_move_pages, 0, 1UL, &page, nullptr, &status, 0) == 0 && status >= 0) return status;
#else
    (void)p;
#endif
    return -1;
}
/* the CPUs of a NUMA node that this thread may run on (empty: unknown) */
inline bool cpusOfNumaNode(int node, cpu_set_t &out)
{
    CPU_ZERO(&out);
    char path[96];
    std::snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    FILE *f = std::fopen(path, "r");
    if (!f) return false;
    char buf[4096];
    const size_t got = std::fread(buf, 1, sizeof(buf) - 1, f);
    std::fclose(f);
    buf[got] = 0;
    cpu_set_t allowed;
    if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return false;
    int any = 0;
    for (char *q = buf; *q;) {
        char *end = nullptr;
        const long a = std::strtol(q, &end, 10);
        if (end == q) break;
        long b = a;
        if (*end == '-') { q = end + 1; b = std::strtol(q, &end, 10); }
        for (long c = a; c <= b && c < CPU_SETSIZE; c++)
            if (c >= 0 && CPU_ISSET((int)c, &allowed)) { CPU_SET((int)c, &out); any++; }
        q = (*end == ',') ? end + 1 : end;
        if (*end != ',' ) break;
    }
    return any > 0;
}

/* zeros without reading the lines first: streaming stores, 64 bytes per trip (the result vector of a 1 GiB call is 4 GiB
 * that nothing reads before the caller does) */
inline void fillZeroStreaming(int *p, size_t n)
{
#if !defined(__SSE2__)
    std::memset(p, 0, n * sizeof(int));                        /* hosts without SSE2 (aarch64, ppc64 nodes with AMD GPUs): plain stores */
    return;
#else
    static const bool plain = std::getenv("PFAC_HOST_FILL_MEMSET") != nullptr;
    if (plain) { std::memset(p, 0, n * sizeof(int)); return; }
    while (n && (reinterpret_cast<uintptr_t>(p) & 63u)) { *p++ = 0; n--; }
    const __m128i z = _mm_setzero_si128();
    for (; n >= 16; n -= 16, p += 16) {
        _mm_stream_si128(reinterpret_cast<__m128i *>(p), z);
        _mm_stream_si128(reinterpret_cast<__m128i *>(p + 4), z);
        _mm_stream_si128(reinterpret_cast<__m128i *>(p + 8), z);
        _mm_stream_si128(reinterpret_cast<__m128i *>(p + 12), z);
    }
    while (n) { *p++ = 0; n--; }
    _mm_sfence();
#endif
}

/*
 * The zero fill of a call's result vector, beside its pipeline: 4 bytes of host memory per position against 1 byte over the link, so it takes a few
 * threads (`helpers`; what the caller sizes them from: cpusAllowed(), fromEnv()) -- the fill and the link's reads share the host's memory channels,
 * and beyond eight threads the upload loses more than the fill gains (256 MiB from pinned buffers on a 2 x 64-core box, link 54 GB/s: 47.0 / 48.8 /
 * 43.8 / 43.3 / 46.4 GB/s with 4 / 8 / 12 / 16 / 24 threads; memset instead of streaming stores: 24.7) -- streaming stores, and the pieces IN ORDER,
 * every thread its share of each: the pairs of piece k are scattered as soon as they are back, while piece k + 1 uploads, not in one pass at the end.
 * With no helpers (a small call) the caller's thread fills, piece by piece, inside waitFilled().  Whatever fails -- no memory for the counters: one
 * memset; fewer threads than planned: their shares are filled by the caller's thread -- every element of the vector is written once start() was called
 * and finish() has returned.
 */
class ZeroFill {
public:
    ZeroFill(int *result, const PieceCut &cut, unsigned helpers) : result_(result), cut_(cut), numPieces_(cut.numPieces()), helpers_(helpers) { CPU_ZERO(&fillCpus_); }
    ZeroFill(const ZeroFill &) = delete;
    ZeroFill &operator=(const ZeroFill &) = delete;
    ~ZeroFill() { finish(); }

    /* the cores this thread may run on (a caller bound to a cpuset has fewer than the machine) */
    static unsigned cpusAllowed()
    {
        cpu_set_t allowed;
        if (sched_getaffinity(0, sizeof(allowed), &allowed) == 0) return (unsigned)CPU_COUNT(&allowed);
        return std::thread::hardware_concurrency();
    }
    /* PFAC_HOST_FILL_THREADS overrides the count: a measurement aid */
    static unsigned fromEnv(unsigned helpers)
    {
        if (const char *e = std::getenv("PFAC_HOST_FILL_THREADS")) { const int v = std::atoi(e); if (v >= 1 && v <= 256) return (unsigned)v; }
        return helpers;
    }

    void start()
    {
        begun_ = true;
        try {
            filled_.reset(new std::atomic<unsigned>[numPieces_]);
            for (size_t k = 0; k < numPieces_; k++) filled_[k].store(0, std::memory_order_relaxed);
            fillers_.reserve(helpers_);
            /* The fill threads run on the NUMA node the caller's result vector lives on: 4 bytes per position of streaming stores that
             * cross the sockets' link meet the link's own reads of the input there (2 x EPYC 9575F, GPU on node 0, pinned buffers
             * first-touched on node 1: p50 7.4 ms, p90 11.4 ms per 256 MiB call against 5.5 / 6.2 ms with the buffers on node 0 --
             * the driver's round-4 line: 29 GB/s median; tools/host_numa_probe.py).  PFAC_HOST_FILL_ANYWHERE=1 leaves them to the OS. */
            if (helpers_ && std::getenv("PFAC_HOST_FILL_ANYWHERE") == nullptr) {
                const int node = numaNodeOf(result_ + cut_.owned / 2);
                bindFill_ = node >= 0 && cpusOfNumaNode(node, fillCpus_);
            }
            for (unsigned t = 0; t < helpers_; t++)
                fillers_.emplace_back([this, t]() {
                    if (bindFill_) (void)pthread_setaffinity_np(pthread_self(), sizeof(fillCpus_), &fillCpus_);
                    for (size_t k = 0; k < numPieces_; k++) {
                        size_t lo, hi;
                        share(k, t, helpers_, lo, hi);
                        fillZeroStreaming(result_ + lo, hi - lo);
                        filled_[k].fetch_add(1, std::memory_order_release);
                        progress_.bump();
                    }
                });
        } catch (...) { /* no memory, or fewer threads than planned: the shares nobody started are filled by the caller's thread, in waitFilled() */ }
        if (!filled_) {                                            /* not even the counters: no helper was started */
            std::memset(result_, 0, cut_.owned * sizeof(int));
            helpers_ = 0;
        }
        started_ = (unsigned)fillers_.size();
    }
    unsigned started() const { return started_; }                  /* threads that run, of the helpers planned */

    /* piece k of the caller's vector is all zeros when this returns */
    void waitFilled(size_t k)
    {
        if (!filled_) return;
        if (helpers_ == 0) {                                       /* a small call: this thread fills, piece by piece */
            size_t lo, hi;
            share(k, 0, 1, lo, hi);
            if (filled_[k].load(std::memory_order_relaxed) == 0) { std::memset(result_ + lo, 0, (hi - lo) * sizeof(int)); filled_[k].store(1, std::memory_order_relaxed); }
            return;
        }
        if (filled_[k].load(std::memory_order_acquire) < helpers_) {        /* acquire: the pairs are scattered onto words the fillers wrote */
            for (unsigned t = started_; t < helpers_; t++) {            /* the shares of threads that could not be started */
                size_t lo, hi;
                share(k, t, helpers_, lo, hi);
                fillZeroStreaming(result_ + lo, hi - lo);
            }
            progress_.wait([&]() { return filled_[k].load(std::memory_order_acquire) >= started_; });
            filled_[k].store(helpers_, std::memory_order_relaxed);
        }
    }

    /* every piece filled, every thread joined (nothing if start() was never called) */
    void finish()
    {
        if (!begun_) return;
        for (size_t k = 0; k < numPieces_; k++) waitFilled(k);
        for (std::thread &t : fillers_) if (t.joinable()) t.join();
    }

private:
    void share(size_t k, unsigned t, unsigned of, size_t &lo, size_t &hi) const          /* thread t's part of piece k */
    {
        const Piece p = cut_.at(k);
        lo = p.off + p.mine * t / of / 16 * 16;
        hi = t + 1 == of ? p.off + p.mine : p.off + p.mine * (t + 1) / of / 16 * 16;
    }

    int *const result_;
    const PieceCut cut_;
    const size_t numPieces_;
    unsigned helpers_, started_ = 0;
    bool begun_ = false, bindFill_ = false;
    cpu_set_t fillCpus_;
    std::unique_ptr<std::atomic<unsigned>[]> filled_;
    Progress progress_;
    std::vector<std::thread> fillers_;
};

} // namespace pfac_internal

#endif
