/*
 * pfac_ext.h -- small extension surface next to the reference-compatible ABI
 * in PFAC.h.  Nothing here exists in the reference; every function is
 * prefixed PFACX_ so a drop-in user never sees it.  The extensions exist so
 * that tests and the bench harness can (a) exercise the host-side pattern
 * compiler on a machine without a GPU, (b) compare the compiled tables
 * byte-for-byte with the oracle, (c) read the facts a multi-GPU driver needs
 * (maximum pattern length = slice overlap, reference omp_PFAC.cpp:324) and
 * (d) A/B the kernel variants.  On top of that come the features the reference
 * does not have: batches of segments (PFACX_matchBatch*), every pattern at a
 * position (PFACX_matchAll*), caseless sets (PFACX_READ_NOCASE), streams
 * (PFACX_stream*), flow sets (PFACX_flows*), the lines that contain a
 * pattern (PFACX_matchLines*, PFACX_gatherLinesFromDevice) and the lines
 * around them (PFACX_matchLinesContext*), the bytes that
 * belong to a match, with their redaction (PFACX_matchSpans*,
 * PFACX_redactSpansFromDevice), the number of occurrences of every pattern
 * (PFACX_countFromDevice / ...FromHost, PFACX_countPairsFromDevice,
 * PFACX_countNonzeroFromDevice) and the disjoint leftmost-longest matches
 * with their replacement by a string per pattern (PFACX_matchDisjoint*,
 * PFACX_replaceFromDevice / ...FromHost), rule sets (PFACX_rules*) and rule
 * sets over the pieces of a flow (PFACX_flowRules*), the
 * counts of every pattern in every segment (PFACX_countBatch*), the
 * occurrences bounded by bytes outside a class: whole words, lines and
 * fields (PFACX_matchWords*, PFACX_wordsPairsFromDevice), pattern
 * groups: each segment of a batch sees only its own patterns (PFACX_groups*),
 * the offsets that cut a buffer into the segments of a batch at the bytes
 * of a delimiter class (PFACX_splitFromDevice / ...FromHost) and the record
 * and column of every match by the same cuts (PFACX_locatePairs*,
 * PFACX_matchLocated*) and the value behind every match
 * (PFACX_capturePairs*, PFACX_matchCaptured*).
 */
#ifndef PFAC_EXT_H_
#define PFAC_EXT_H_

#include "PFAC.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Like PFAC_create() but binds no device and loads no kernel module: only
 * the host pattern compiler and the CPU platforms work.  Any GPU entry point
 * on such a handle returns PFAC_STATUS_LIB_NOT_EXIST -- there is no silent
 * CPU fallback for the GPU platform.  The platform is preset to
 * PFAC_PLATFORM_CPU. */
PFAC_status_t PFACX_createHostOnly(PFAC_handle_t *handle);

/* PFAC_readPatternFromFile (ref PFAC.cpp:653-735) for patterns that are already in memory: `patterns`
 * holds `size` bytes in the pattern-file format, one pattern per '\n'-terminated line (bytes after
 * the last '\n' are ignored, like in a file).  Same status codes, same pattern IDs; replaces a
 * previously loaded set.  The buffer is copied. */
PFAC_status_t PFACX_readPatternFromMemory(PFAC_handle_t handle, const char *patterns, size_t size);

/* The two readers with options (defined behaviour for what the reference does silently).
 *   PFACX_READ_STRICT    bytes behind the last '\n' -- a last line without a newline, which the reference drops without
 *                        a word (PFAC_reorder_Table.cpp:181-195) -- are PFAC_STATUS_INVALID_PARAMETER.  Without the flag
 *                        they are ignored as in the reference, and PFACX_getInfo reports how many there were
 *                        (trailingBytesIgnored).
 *   PFACX_READ_STRIP_CR  "\r\n" line ends: the '\r' is not part of the pattern (the reference keeps it: user guide r1.2
 *                        p.15 item 5).  A '\r' elsewhere in a line stays.
 *   PFACX_READ_NOCASE    a caseless set (Snort's nocase, grep -iF).  ASCII fold: bytes 0x41-0x5A ('A'-'Z') map to 0x61-0x7A;
 *                        every other byte is unchanged (no locale, no Latin-1, no UTF-8).
 *                        A set read with this flag is exactly the set read, without it, from the pattern bytes with the ASCII
 *                        fold applied (after PFACX_READ_STRIP_CR): pattern IDs, tables, dumps and PFACX_getInfo (but for
 *                        caseInsensitive) are those of the folded bytes.  Every match call on such a handle returns exactly
 *                        what the same call returns on that folded set over the input with the ASCII fold applied; the
 *                        caller's input buffer, host or device, is never modified.  Patterns that become equal when folded
 *                        are duplicate lines: reported under the highest of their IDs, listed once by PFACX_matchAll*.
 *                        Reading a set without the flag makes the handle case-sensitive again.  The device calls fold into a
 *                        grow-only handle scratch of `size` bytes (deviceScratchBytes; PFACX_trim frees it).
 * flags == 0 is exactly PFAC_readPatternFromFile / PFACX_readPatternFromMemory.  Bit 4 is not assigned and is refused as
 * before, like every other unknown bit. */
#define PFACX_READ_STRICT   1u
#define PFACX_READ_STRIP_CR 2u
#define PFACX_READ_NOCASE   8u
PFAC_status_t PFACX_readPatternFromFileEx(PFAC_handle_t handle, const char *filename, unsigned int flags);
PFAC_status_t PFACX_readPatternFromMemoryEx(PFAC_handle_t handle, const char *patterns, size_t size, unsigned int flags);

typedef struct {
    size_t structSize;        /* IN: sizeof(PFACX_info_t) of the caller's header; the library never writes past it (a
                                 caller built against an older, shorter struct stays safe).  OUT: bytes filled in */
    int numOfPatterns;        /* F                                             */
    int numOfStates;          /* includes the unused state 0 (ref PFAC.cpp:704) */
    int numOfFinalStates;     /* == numOfPatterns                               */
    int initialState;         /* F + 1                                          */
    int maxPatternLen;
    int numOfLeaves;
    int perfMode;             /* PFAC_perfMode_t                                */
    int textureMode;          /* PFAC_textureMode_t as currently stored         */
    int platform;             /* PFAC_platform_t                                */
    int hasDevice;            /* 0 for PFACX_createHostOnly handles             */
    size_t numOfTableEntry;   /* ref PFAC_P.h:131-133                           */
    size_t sizeOfTableEntry;
    size_t sizeOfTableInBytes;
    /* prefilter (this implementation only; see DESIGN.md "filter") */
    int filterLog2Bits;       /* 3-gram bitmap has 2^filterLog2Bits bits (two per 3-gram, in one dword) */
    int filterHasShort;       /* 1 if some pattern is shorter than 3 bytes      */
    size_t filterBitsSet;     /* population of the 3-gram bitmap                */
    int kernelVariant;        /* PFACX_KERNEL_*                                 */
    int multiProcessorCount;
    int filterLog2BitsLadder; /* prefix-ladder bitmap has 2^filterLog2BitsLadder bits (level 2 of the prefilter) */
    int filterLog2BitsFinal3; /* length-3-pattern bitmap                         */
    size_t filterBitsSetLadder;
    int chainJumpLog2;        /* PFACX_TABLE_CHAIN: log2 of its jump-table slots (0 until the table exists) */
    size_t chainSlots;        /* PFACX_TABLE_CHAIN: 16-byte units in total: slot headers, then as many extension units */
    size_t ladderStops;       /* prefix ladder: trie nodes inserted as "stop: walk from here" ...            */
    size_t ladderGoOns;       /* ... and as "go on: test the next prefix length"                             */
    int ladderThin;           /* nodes with at most this many patterns below them are stops ...             */
    int ladderExtend;         /* ... this many levels further down                                          */
    size_t trailingBytesIgnored; /* bytes behind the last '\n' of the pattern file that were ignored (0: none)  */
    size_t deviceTableBytes;  /* device memory the pattern set holds: chained table, initial row, prefilter bitmaps,
                                 launch counters; the reference-layout table only while PFACX_KERNEL_REFTABLE is selected; the carried bytes of
                                 the handle's device-fed streams (PFACX_stream*: state, not scratch) */
    size_t deviceScratchBytes; /* device memory the handle's calls have left allocated (grow-only; PFACX_trim frees it): the two staging
                                 pieces of PFAC_matchFromHost / ...Reduce (9 bytes per position of a piece), the ordering scratch of the
                                 compacted output, the list of pattern-dense chunks, what the batch calls keep (pattern lengths, offsets of a
                                 host piece, the compaction scratch of the compacted form), the folded input of a caseless set's device
                                 calls (PFACX_READ_NOCASE) */
    int streamNearMisses;      /* what the handle's last big full-result launch said about its stream (host memory the launch's last block
                                 writes; nothing is waited for): 1 = full of near misses of long patterns -> PFACX_WALKER_AUTO picks STAGE ... */
    int streamDense;           /* ... 1 = most of it pattern-dense (short patterns over text, runs of a pattern byte) -> PFACX_KERNEL_AUTO
                                 sends the next big call to the tiled kernel alone */
    int filterLadderLast;      /* deepest level of the prefix ladder: 20, or 60 when the nodes behind the 20th byte fit its bitmap too */
    size_t filterTailEntries;  /* entries of the tail table in its LDS form (PFACX_TABLE_FILTER_TAIL): sets of a few thousand patterns */
    size_t filterTailGlobalEntries; /* ... in its device-memory form (PFACX_TABLE_FILTER_TAIL_GLOBAL): sets whose bitmaps fill the LDS, or with more
                                  thin stops than the LDS form holds (Snort-scale).  A set has one form or the other (or none) */
    int filterLog2TailGlobal;  /* log2 of the buckets of that table */
    unsigned int filterLadderSalt; /* XORed into the depth-4 hash of the prefix ladder (chosen per pattern set: pfac_context.h) */
    int filterSkipTags;        /* skip tags of the prefix ladder (PFACX_TABLE_FILTER_SKIP): depth-6 nodes with a single path down to depth 20 (at most 8) */
    int maxMatchesPerPosition; /* the most patterns that can start at one position: the longest PFACX_TABLE_PREFIX_PATTERN chain plus one (1 when
                                  no pattern is a prefix of another).  PFACX_matchAll* with capacity = size * maxMatchesPerPosition never truncates */
    int caseInsensitive;       /* 1: the set was read with PFACX_READ_NOCASE (or loaded from a caseless compiled file): every match call folds its input */
} PFACX_info_t;

PFAC_status_t PFACX_getInfo(PFAC_handle_t handle, PFACX_info_t *info);

/* Host copies of the compiled tables, owned by the handle (valid until the
 * next readPatternFromFile / setPerfMode / destroy). */
typedef enum {
    PFACX_TABLE_DENSE        = 0,  /* int[numOfStates*256]           (TIME_DRIVEN)  */
    PFACX_TABLE_HASH_ROWPTR  = 1,  /* int2[numOfStates]              (SPACE_DRIVEN) */
    PFACX_TABLE_HASH_VALPTR  = 2,  /* int2[numOfTableEntry]          (SPACE_DRIVEN) */
    PFACX_TABLE_INITIAL_ROW  = 3,  /* int[256], both modes                          */
    PFACX_TABLE_FILTER_GRAM3 = 4,  /* uint32[2^filterLog2Bits / 32]                 */
    PFACX_TABLE_FILTER_SHORT = 5,  /* uint32[2048] (65536 bits)                     */
    PFACX_TABLE_FILTER_LADDER = 6, /* uint32[2^filterLog2BitsLadder / 32]           */
    PFACX_TABLE_FILTER_FINAL3 = 7, /* uint32[2^filterLog2BitsFinal3 / 32]           */
    PFACX_TABLE_FILTER_GRAM1 = 9,  /* uint32[2^19 / 32]: one-bit 3-gram bitmap of the compacted-output kernel       */
    PFACX_TABLE_FILTER_PREFIX4 = 10, /* uint32[2^17 / 32]: the 4-byte pattern prefixes, two probes (same kernel)    */
    PFACX_TABLE_FILTER_TAIL  = 11, /* uint32[3] per slot {ladder hash of a stop node, that hash rolled over the rest of the one pattern below it,
                                      bytes of that rest | depth << 8}, a power of two of slots (none: empty): the veto on a ladder stop */
    PFACX_TABLE_FILTER_TAIL_GLOBAL = 12, /* uint32[4] per bucket: two entries {ladder hash of a stop node, (that hash rolled over the rest of the one
                                      pattern below it) & ~0x7FF | depth of the first compared byte << 3 | bytes / 4 - 1}; bucket of a hash h =
                                      (h * 0x9E3779B1) >> (32 - filterLog2TailGlobal); an entry is occupied if (word1 & 0x7F8) != 0 */
    PFACX_TABLE_FILTER_SKIP  = 13, /* uint32[filterSkipTags]: ladder hashes (depth 6) whose candidates are next asked at depth 20 */
    PFACX_TABLE_PREFIX_PATTERN = 14, /* int[numOfPatterns + 1] by pattern id: the id of the longest pattern that is a proper prefix of pattern id
                                      (0: none; entry 0 is 0).  IDs that are never reported (the lower IDs of duplicate lines) have 0.  What
                                      PFACX_matchAll* follows from the longest pattern at a position */
    PFACX_TABLE_CHAIN        = 8   /* uint32[4] per 16-byte unit: the device-only chained form of the hashed table that the
                                      GPU kernels walk in both perf modes.  chainSlots / 2 slot headers -- compact buckets,
                                      breadth first; then the 256 slots of the initial state; then the 2^chainJumpLog2
                                      slots of the jump table of 4-byte prefixes; then the LONG jump table, 2^chainJumpLog2
                                      slots again (same hash, chains of up to 23 bytes) -- followed by as many extension
                                      units, unit i = chain bytes 8..22 of slot i (long slots of wide buckets and of the long
                                      jump table only).  With N = chainSlots / 2 and J = chainJumpLog2:
                                        [0, N - 256 - 2 * 2^J) buckets | [.., N - 2 * 2^J) initial state | [.., N - 2^J) jump |
                                        [.., N) long jump | [N, 2 N) extension units.
                                      Built on first use on a host-only handle.  */
} PFACX_table_t;

PFAC_status_t PFACX_getTable(PFAC_handle_t handle, PFACX_table_t which, const void **ptr,
                             size_t *bytes);

/* Kernel variants of the GPU match path. */
/* The walker of the full-result filter kernel (PFACX_setWalker).  WINDOW: a walk's input travels with its queue entry and
 * lives in registers (fastest on text); STAGE: walks read their input in place from the chunks a wave keeps staged in LDS and
 * take 24 bytes per step through long single-successor runs (fastest when the stream is full of near misses of long
 * patterns: BASELINE config 5, 19 % over WINDOW); AUTO (default): whatever the handle's previous full-result launch found its
 * stream to be -- the first launch on a handle runs WINDOW.  Results are identical.
 * A pattern set that has a TAIL TABLE (filterTailEntries of PFACX_getInfo > 0 and room in the CU's LDS: sets of a few thousand
 * patterns) is different: the prefilter puts a ladder stop to that table before it becomes a walk, near misses hardly reach a walker,
 * and AUTO and WINDOW both mean the window walker behind that veto (another 13 % on BASELINE config 5); STAGE is the stage walker
 * without it.
 * A set whose tail table lies in DEVICE memory (filterTailGlobalEntries > 0: Snort-scale sets, round 6) asks it with one gathered load per
 * stopped candidate, which text does not repay: under AUTO such a set runs the plain window walker until a launch reports a stream full of
 * near misses, and the veto kernel (not the stage walker) from then on, until a launch of that kernel reports text again; WINDOW is the
 * plain window walker, VETO the veto kernel, always. */
#define PFACX_WALKER_AUTO   0
#define PFACX_WALKER_WINDOW 1
#define PFACX_WALKER_STAGE  2
#define PFACX_WALKER_VETO   3   /* the window walker behind the tail-hash veto whatever the stream looks like (a set without a tail table of either form: WINDOW) */
PFAC_status_t PFACX_setWalker(PFAC_handle_t handle, int walker);

#define PFACX_KERNEL_FILTER 0   /* LDS prefilter + compacted walkers wherever the pointers allow it */
#define PFACX_KERNEL_NAIVE  1   /* the tiled kernel alone: one position per thread slot, tile + halo and the
                                   hottest transition rows in LDS, coalesced result lines (any alignment)   */
#define PFACX_KERNEL_AUTO   2   /* default: FILTER, except that small calls take the tiled kernel alone
                                   (lower latency: the filter kernel has a ~19 us floor).  Either way the
                                   filter kernel hands pattern-dense 2 KiB chunks (most positions pass its
                                   first level) to the tiled kernel that follows it.                      */
#define PFACX_KERNEL_REFTABLE 3 /* the reference-shaped kernel: one thread per byte through the REFERENCE-layout
                                   table of the perf mode (dense int[S][256] / hashed int2 pair), which is built
                                   and uploaded when this variant is selected (S KiB for the dense table).  An
                                   independent second implementation for cross-checks; 6-20x slower.        */

PFAC_status_t PFACX_setKernelVariant(PFAC_handle_t handle, int variant);

/* A compiled pattern set on disk: everything PFAC_readPatternFromFile derives from the pattern
 * file -- trie, hashed / chained tables, prefilter bitmaps -- with a version + layout fingerprint + checksum
 * header.  PFACX_loadCompiled replaces the handle's pattern set like PFAC_readPatternFromFile does (and sets the
 * perf mode the set was saved with); a file of another build or a damaged one is PFAC_STATUS_INVALID_PARAMETER,
 * a missing one PFAC_STATUS_FILE_OPEN_ERROR.  Works on host-only handles too.  A caseless set (PFACX_READ_NOCASE)
 * is written as format version 8 and loads as caseless; a case-sensitive one keeps version 7.  A build that knows
 * only version 7 refuses a caseless file instead of loading it as case-sensitive. */
PFAC_status_t PFACX_saveCompiled(PFAC_handle_t handle, const char *filename);
PFAC_status_t PFACX_loadCompiled(PFAC_handle_t handle, const char *filename);

/* The handle keeps its device temporaries between calls (the reference allocates and frees them per call,
 * PFAC.cpp:920-958): two staging sets of PFAC_matchFromHost (about 9 B per position of a 32 Mi-position piece), the copies
 * of PFAC_matchFromHostReduce (9 B per input byte), sort scratch.  PFACX_trim frees them; the next call that needs one
 * allocates it again.  The pattern set and its tables stay. */
PFAC_status_t PFACX_trim(PFAC_handle_t handle);

/* What the handle's FIRST PFAC_matchFromHost / PFAC_matchFromHostReduce would allocate, create and load inside the call, done ahead of it: the
 * two staging pieces (for calls of up to maxBytes input bytes; 0 or more than a piece: whole pieces of 32 Mi positions), their copy streams and
 * events, the ordering scratch, the kernels' code objects (one throwaway scan), the runtime's staging of pageable host memory (one throwaway
 * upload).  Optional: without it the first call does the same, ~100 ms instead of ~7 (256 MiB).  PFACX_trim undoes it; a handle on a CPU
 * platform has nothing to prepare (success). */
PFAC_status_t PFACX_prepare(PFAC_handle_t handle, size_t maxBytes);

/* One call shards a host stream over several GPUs of the node (reference users write this
 * themselves after PFAC/test/omp_PFAC.cpp:257-394): one worker thread and one internal handle per entry of
 * `devices` (NULL = devices 0..numDevices-1; numDevices 0 = every visible device), contiguous slices scanned
 * with a maxPatternLen read-ahead, no exchange between devices.  `handle` supplies the pattern set and modes
 * and keeps the per-device handles for the next call.  A device may be listed more than once.
 * On a handle whose platform is a CPU platform (PFAC_setPlatform, PFACX_createHostOnly) there is nothing to shard over: the call then runs
 * `numDevices` workers (0 = one) as host threads over the CPU matchers -- same slices, same read-ahead, same folding of the results; `devices`
 * is ignored.  That is a dry run of the driver on a machine without a GPU, not a fallback: the GPU platform never takes it. */
PFAC_status_t PFACX_matchFromHostMultiGPU(PFAC_handle_t handle, char *h_inputString, size_t size,
                                          int *h_matched_result, int numDevices, const int *devices);

/* ... and its compacted-output form (PFAC_matchFromHostReduce over several GPUs): the (id, position) pairs of the whole stream in ascending
 * position order, positions counted from the start of the stream; h_matched_result and h_pos hold `size` entries each (the workers use
 * them as scratch), size < 2^31.  One byte per position crosses a host link and nothing is filled on the host: this, not the
 * full-vector form, is what scales with the number of links. */
PFAC_status_t PFACX_matchFromHostReduceMultiGPU(PFAC_handle_t handle, char *h_inputString, size_t size, int *h_matched_result, int *h_pos,
                                                int *h_num_matched, int numDevices, const int *devices);

/* Counters of the most recent launch of the filter kernel on this handle (PFAC_matchFromDevice / ...Reduce of
 * 32 MiB or more; SURVEY 8d, configuration C5: walk depth, lane utilisation, early-out rate).  Waits for the default
 * stream.  All zero before the first such launch. */
typedef struct {
    size_t structSize;                    /* IN: sizeof(PFACX_scan_stats_t) of the caller's header; OUT: bytes filled in (see PFACX_info_t) */
    unsigned long long walkerRounds;      /* wave-wide walker rounds (one table step for every live walk)      */
    unsigned long long laneSteps;         /* table steps taken, summed over lanes                              */
    unsigned long long walksStarted;      /* positions that passed level 1 and the prefix ladder and were walked */
    unsigned long long level1Hits;        /* positions that passed filter level 1                              */
    int tilesPerChunk;                    /* KiB per chunk                                                     */
    int walksPerLane;                     /* independent walks per lane in THAT launch (the full-result and the compacted-
                                             output kernel differ)                                              */
    unsigned long long ladderCandidates;  /* level-1 hits whose first four bytes are a pattern prefix (or a short
                                             pattern): what the prefix ladder was asked about                  */
    unsigned long long denseChunks;       /* 2 KiB chunks in which more than half of the positions (PFAC_DENSE_HITS of 2048) passed level 1:
                                             left to the tiled kernel that follows the filter kernel (0 for a
                                             compacted-output launch, which lists none)                         */
    double filterKernelMs;                /* GPU time of that launch of the filter kernel alone (HIP events around it);
                                             -1 unless PFACX_setKernelTiming(handle, 1) was in force           */
    unsigned long long stageModeWaves;    /* full-result launch: scanning waves that ended it finding their stream full of near misses
                                             (STAGE walker: in stage mode, two chunks staged, walking out of LDS; WINDOW walker:
                                             fetching extension units ahead); a majority makes PFACX_WALKER_AUTO give the handle's
                                             next launch the STAGE walker                                          */
    int walker;                           /* PFACX_WALKER_WINDOW / PFACX_WALKER_STAGE: what that launch ran with */
    int veto;                             /* ... and whether the window walker stood behind the tail-hash veto: 0 = no, 1 = tail table in LDS, 2 = in device
                                             memory (the kernel PFACX_WALKER_VETO asks for) */
} PFACX_scan_stats_t;

PFAC_status_t PFACX_getScanStats(PFAC_handle_t handle, PFACX_scan_stats_t *stats);

/* Measurement aid: with `on` != 0 every launch of the filter kernel on this handle is bracketed by two HIP events on
 * the default stream (a few microseconds per call); PFACX_getScanStats then reports the kernel's own time -- inside
 * PFAC_matchFromDeviceReduce, say, whose other launches a caller's events cannot tell apart. */
PFAC_status_t PFACX_setKernelTiming(PFAC_handle_t handle, int on);

/* Batch matching: one input buffer of `size` bytes cut into numSegments independent segments (packets, records) by
 * numSegments + 1 offsets -- offsets[0] == 0, offsets[numSegments] == size, never decreasing (empty segments are allowed).
 * No match runs from one segment into the next: the result at a position p of segment k is what PFAC_matchFromHost on a CPU
 * platform returns at p - offsets[k] for segment k alone, so the result is the concatenation of the per-segment results (a
 * batch of one segment is the plain call).  One call costs about what the plain call over the same bytes costs (DESIGN.md
 * "batch"), where one call per segment pays a call's fixed cost per segment.
 * A null pointer, numSegments == 0 with size > 0, or host offsets that break the rules: PFAC_STATUS_INVALID_PARAMETER;
 * size == 0: success, nothing done; a host-only handle on the GPU path: PFAC_STATUS_LIB_NOT_EXIST.
 * DEVICE offsets are not checked (that would cost a sync): they are the caller's contract, like the sizes of the buffers.
 * The kernels clamp every offset to [0, size] and take a decreasing pair as an empty segment, so bad offsets give wrong
 * results but never a read or write outside the buffers. */

/* full result over device buffers (d_offsets: numSegments + 1 size_t in device memory); asynchronous on the default stream,
 * like PFAC_matchFromDevice */
PFAC_status_t PFACX_matchBatchFromDevice(PFAC_handle_t handle, char *d_input, size_t size, const size_t *d_offsets, size_t numSegments,
                                         int *d_matched_result);
/* full result over host buffers; follows PFAC_setPlatform (the CPU platforms match segment by segment); synchronous; h_offsets is
 * validated */
PFAC_status_t PFACX_matchBatchFromHost(PFAC_handle_t handle, char *h_input, size_t size, const size_t *h_offsets, size_t numSegments,
                                       int *h_matched_result);
/* compacted: the (id, position) pairs in position order as PFAC_matchFromDeviceReduce returns them (d_matched_result and d_pos hold
 * `size` entries), plus d_segFirst[numSegments + 1]: the pairs of segment k are entries [d_segFirst[k], d_segFirst[k + 1]);
 * size < 2^31; synchronous (the count comes to the host) */
PFAC_status_t PFACX_matchBatchFromDeviceReduce(PFAC_handle_t handle, char *d_input, size_t size, const size_t *d_offsets, size_t numSegments,
                                               int *d_matched_result, int *d_pos, int *d_segFirst, int *h_num_matched);

/* All matches.  The calls above report ONE pattern per position, the longest that starts there.  Rule-based users (intrusion
 * detection, log scanning) need every pattern that occurs, since each belongs to a rule of its own.
 *   The ALL-MATCH LIST of an input is the set of pairs (position p, pattern id) such that pattern id occurs at p; positions count
 *   from the start of the input.  ORDER: ascending position; within one position the longest pattern first, the shorter ones
 *   behind it in descending length -- so the first pair of each position is the pair PFAC_matchFromDeviceReduce reports there.
 *   Duplicate lines load as one pattern, reported under the highest of their IDs as in every other call, and are listed once.
 *   The list can be longer than the input (patterns a, aa, ..., a x 8 over a run of a: up to 8 pairs per position): the count
 *   is a size_t.  Positions are int: size < 2^31, as for the compacted calls.
 * Every pattern that starts at p is a prefix of the longest one there, so the list follows from the longest-match result and
 * PFACX_TABLE_PREFIX_PATTERN (DESIGN.md "all matches").
 * d_ids / d_pos (h_ids / h_pos) hold `capacity` entries each, capacity >= size (they double as the scan's pair list, as in
 * PFAC_matchFromDeviceReduce); a smaller capacity is PFAC_STATUS_INVALID_PARAMETER.  A list longer than capacity: exactly its first
 * `capacity` pairs are written and nothing behind them, *h_num_matched is the full count and the call returns
 * PFACX_STATUS_OUTPUT_TRUNCATED -- grow the arrays and call again (capacity = size * maxMatchesPerPosition of PFACX_getInfo never
 * truncates).  Null pointers, size == 0 (success, *h_num_matched = 0), size >= 2^31 and a host-only handle on the GPU path are
 * handled as in PFAC_matchFromDeviceReduce.  All three calls are synchronous (the count comes to the host). */
#define PFACX_STATUS_OUTPUT_TRUNCATED ((PFAC_status_t)10100)

/* over device buffers; the GPU platform's match path (whatever kernel variant, walker, perf mode and texture mode the handle selects) */
PFAC_status_t PFACX_matchAllFromDevice(PFAC_handle_t handle, char *d_input, size_t size, int *d_ids, int *d_pos, size_t capacity,
                                       size_t *h_num_matched);
/* over host buffers; follows PFAC_setPlatform: the CPU platforms (host-only handles included) match on the CPU, the GPU platform
 * runs the pipelined path of PFAC_matchFromHostReduce; either way the list is expanded in place on the host.  This and every other host form
 * that scans and then works on the pairs (PFACX_count / matchLines / matchSpans / matchDisjoint / matchWords / rulesMatch ...FromHost) and
 * PFACX_replaceFromHost: a call whose handle receives another pattern set from a second thread while it runs returns
 * PFAC_STATUS_PATTERNS_NOT_READY (rule sets: PFAC_STATUS_INVALID_PARAMETER) and writes no result counts */
PFAC_status_t PFACX_matchAllFromHost(PFAC_handle_t handle, char *h_input, size_t size, int *h_ids, int *h_pos, size_t capacity,
                                     size_t *h_num_matched);
/* batch form (offsets as for PFACX_matchBatch*; device offsets are clamped, never checked): every segment its own all-match list,
 * positions relative to the buffer, the lists concatenated in segment order; d_segFirst[numSegments + 1] (device) indexes the
 * whole list: the pairs of segment k are [d_segFirst[k], d_segFirst[k + 1]) (indices past capacity name pairs not written) */
PFAC_status_t PFACX_matchAllBatchFromDevice(PFAC_handle_t handle, char *d_input, size_t size, const size_t *d_offsets, size_t numSegments,
                                            int *d_ids, int *d_pos, size_t capacity, size_t *d_segFirst, size_t *h_num_matched);

/* Streams: input that arrives over time -- a reassembled TCP flow, a tailed log, a file read in pieces.  The calls above take their
 * buffer's last byte for the end of the data; a stream carries what is still undecided from one piece to the next.
 *   Let M = maxPatternLen of the handle's set and S, of length T, the stream's pieces so far, concatenated in call order.  The pairs
 *   returned by all piece calls since the stream was opened (or reset), followed by the pairs of PFACX_streamFlush, are exactly the
 *   (id, position) list PFAC_matchFromHostReduce on a CPU platform returns for S as ONE buffer -- same pairs, ascending position,
 *   nothing twice, nothing missing -- however S was cut: pieces of 0 bytes and pieces shorter than M included.
 *   A position is FINAL once M - 1 bytes behind it have been seen.  A piece call reports exactly the pairs at stream positions
 *   [R, max(R, T - (M - 1))), T counted with the piece and R where the previous call stopped reporting (0 after open / reset).
 *   PFACX_streamFlush declares the end of the stream, reports the pairs at [R, T) with the stream's end as the end of the data, and
 *   leaves the stream reset (T = R = 0, free to be fed by either kind of call).  With M == 1 nothing is ever pending.
 * POSITIONS are int, relative to the first byte of the piece of that call: a pair that starts in bytes carried over from earlier
 * pieces has a negative position (never below -(M - 1)).  *h_pieceOffset receives the stream offset of the piece's first byte (T
 * before the call), so *h_pieceOffset + position is the position in S: a stream has no 2^31 limit, one piece has (size < 2^31).
 * The positions of PFACX_streamFlush are relative to T (all negative).
 * capacity: entries of each of the two arrays, >= size + M (a call can report up to M - 1 carried positions on top of its own, and the
 * arrays double as the scan's pair list); PFACX_streamFlush: >= M.  Smaller: PFAC_STATUS_INVALID_PARAMETER, the stream unchanged --
 * as after any failed call: repeat it and get what it would have returned.
 * A stream is fed by ONE kind of call, fixed by its first piece call of size > 0 after open / reset / flush: device calls (the carried
 * bytes live in device memory, PFACX_streamFlush takes device arrays) or host calls (host memory, host arrays); the other kind is
 * PFAC_STATUS_INVALID_PARAMETER.  The host form follows PFAC_setPlatform like PFACX_matchAllFromHost: the CPU platforms, host-only
 * handles included, run entirely on the CPU; the GPU platform runs the pipelined path of PFAC_matchFromHostReduce.  The device form on
 * a host-only handle is PFAC_STATUS_LIB_NOT_EXIST.  Null pointers and size >= 2^31: PFAC_STATUS_INVALID_PARAMETER; size == 0: success,
 * zero pairs, the stream unchanged.  A caseless handle (PFACX_READ_NOCASE) matches the folded set over the folded stream; the caller's
 * buffers are never modified.
 * A stream belongs to the pattern set that was loaded when it was opened or last reset: after the handle reads or loads another set,
 * piece and flush calls return PFAC_STATUS_INVALID_PARAMETER until PFACX_streamReset.  Any number of streams per handle (one per
 * flow); PFAC_destroy closes the handle's streams.  A call takes the handle's lock like the other match calls (two threads may drive
 * two streams of one handle; one stream takes one call at a time).  All calls are synchronous (the count comes to the host).
 * MEMORY: a device-fed stream holds two buffers of M - 1 bytes for its carried bytes (plus 2 (M - 1) bytes where M exceeds 24 Ki).
 * They are state, not scratch: counted under deviceTableBytes of PFACX_getInfo, kept by PFACX_trim, freed by PFACX_streamClose.
 * COST: the piece is scanned in place -- no copy; a call adds one small launch for the seam to the compacted call over
 * the same bytes, and a piece shorter than M - 1 bytes is that launch alone. */
typedef struct PFACX_stream_s *PFACX_stream_t;
PFAC_status_t PFACX_streamOpen(PFAC_handle_t handle, PFACX_stream_t *stream);
PFAC_status_t PFACX_streamReset(PFACX_stream_t stream);      /* forget the carried bytes, T = R = 0; adopt the handle's current pattern set */
PFAC_status_t PFACX_streamClose(PFACX_stream_t stream);
PFAC_status_t PFACX_streamMatchFromDevice(PFACX_stream_t stream, char *d_piece, size_t size, int *d_ids, int *d_pos, size_t capacity,
                                          int *h_num_matched, unsigned long long *h_pieceOffset);
PFAC_status_t PFACX_streamMatchFromHost(PFACX_stream_t stream, char *h_piece, size_t size, int *h_ids, int *h_pos, size_t capacity,
                                        int *h_num_matched, unsigned long long *h_pieceOffset);
PFAC_status_t PFACX_streamFlush(PFACX_stream_t stream, int *ids, int *pos, size_t capacity, int *h_num_matched);

/* Flow sets: many streams advanced by ONE call.  A buffer of packets that belong to many reassembled flows is matched in one launch
 * sequence -- the cost of PFACX_matchBatchFromDeviceReduce -- and every flow keeps what is still undecided from batch to batch -- the
 * exactness of PFACX_stream*.  A flow set is numFlows streams of one handle whose state the library keeps together; flows are named
 * by their index, 0 .. numFlows - 1.
 *   A piece call takes one buffer of `size` bytes cut into numPieces pieces by h_offsets[numPieces + 1] (the rules of
 *   PFACX_matchBatchFromHost: first 0, last `size`, never decreasing; empty pieces are allowed); piece k belongs to flow
 *   h_flowIds[k].  It returns exactly what this sequence returns, the pair lists concatenated in piece order: for k = 0 ..
 *   numPieces - 1, PFACX_streamMatchFromHost on a CPU platform with piece k on a stream of its own per flow.  The pairs of piece k are
 *   entries [pieceFirst[k], pieceFirst[k + 1]): the carried positions the piece makes final, then the piece's own final positions,
 *   ascending; positions are int, relative to the first byte of piece k (carried ones negative, never below -(M - 1));
 *   h_pieceOffsets[k] is that flow's T before the call.  Finality, caseless sets and "the caller's buffers are never modified" are
 *   those of the streams, per flow.
 *   PFACX_flowsFlush declares the end of the n named flows: PFACX_streamFlush per flow, in the order named, first[n + 1] indexing the
 *   pairs; those flows are left reset.
 * OFFSETS AND FLOW IDS ARE HOST ARRAYS and are validated completely: an id >= numFlows, offsets that break the rules, or A FLOW NAMED
 * TWICE IN ONE CALL is PFAC_STATUS_INVALID_PARAMETER.  Pieces of one flow that arrive in one batch are laid adjacent by the caller and
 * passed as ONE piece.
 * capacity (entries of each of ids / pos) >= size + numPieces * (M - 1), a sum below 2^31; the flush: >= max(1, n * (M - 1)).  Smaller:
 * PFAC_STATUS_INVALID_PARAMETER.  An empty piece: zero pairs, the flow unchanged, its offset reported; size == 0 with numPieces > 0 is
 * a batch of empty pieces and succeeds.  numPieces == 0 needs size == 0: zero pairs, pieceFirst is not written (either form).
 * The arrays double as the scan's pair list, as in PFAC_matchFromDeviceReduce: entries below `size` may be overwritten beyond the
 * pairs returned; nothing is written at or beyond `capacity`.
 * A FAILED CALL -- any status but success -- LEAVES EVERY FLOW UNCHANGED: repeat it and get what it would have returned.
 * A flow set is fed by ONE kind of call, fixed by its first piece call that carries a non-empty piece until a reset of all flows:
 * the device form (carries in device memory; the flush takes device arrays, `first` included) or the host form (host memory, host
 * arrays); the other kind is PFAC_STATUS_INVALID_PARAMETER.  The host form follows PFAC_setPlatform: the CPU platforms, host-only
 * handles included, run on the CPU; the GPU platform runs the pipelined host path piece by piece (it keeps the contract, not the
 * link rate).  The device form on a host-only handle is PFAC_STATUS_LIB_NOT_EXIST.
 * After the handle reads or loads another pattern set every piece and flush call is PFAC_STATUS_INVALID_PARAMETER until
 * PFACX_flowsReset(flows, NULL, 0).  Calls take the handle's lock and the set's own (one call at a time per set; two threads may
 * drive two sets of one handle); PFAC_destroy closes the handle's flow sets.  All calls are synchronous.
 * MEMORY: a device-fed set holds ONE allocation of 2 x numFlows x (M - 1) bytes (plus alignment) for its carries, made by the first
 * device call: state, counted under deviceTableBytes of PFACX_getInfo, kept by PFACX_trim, freed by PFACX_flowsClose.  What a call
 * uploads and stages (offsets, ids, per-piece counts, a staging list of pairs) is grow-only scratch of the handle:
 * deviceScratchBytes, given back by PFACX_trim.
 * COST: one compacted scan of the buffer in place, a handful of seam and merge launches whatever the number of pieces,
 * and 5 - 7 ns of host and device work per piece: about the batch call for pieces of tens of KiB, several times it for packet-sized
 * pieces, thousands of times less than one stream call per piece. */
typedef struct PFACX_flows_s *PFACX_flows_t;
PFAC_status_t PFACX_flowsOpen(PFAC_handle_t handle, size_t numFlows, PFACX_flows_t *flows);
PFAC_status_t PFACX_flowsClose(PFACX_flows_t flows);
/* forget the state of the n named flows (T = R = 0); h_flowIds == NULL, n == 0: of all flows, and adopt the handle's current set */
PFAC_status_t PFACX_flowsReset(PFACX_flows_t flows, const unsigned int *h_flowIds, size_t n);
PFAC_status_t PFACX_flowsMatchFromDevice(PFACX_flows_t flows, char *d_input, size_t size, const size_t *h_offsets, const unsigned int *h_flowIds,
                                         size_t numPieces, int *d_ids, int *d_pos, size_t capacity, int *d_pieceFirst /* numPieces + 1 */,
                                         unsigned long long *h_pieceOffsets /* numPieces */, int *h_num_matched);
PFAC_status_t PFACX_flowsMatchFromHost(PFACX_flows_t flows, char *h_input, size_t size, const size_t *h_offsets, const unsigned int *h_flowIds,
                                       size_t numPieces, int *h_ids, int *h_pos, size_t capacity, int *h_pieceFirst /* numPieces + 1 */,
                                       unsigned long long *h_pieceOffsets /* numPieces */, int *h_num_matched);
/* declare the end of the n named flows: their pending pairs, flow by flow in the order named; first[n + 1] indexes them */
PFAC_status_t PFACX_flowsFlush(PFACX_flows_t flows, const unsigned int *h_flowIds, size_t n, int *ids, int *pos, size_t capacity, int *first,
                               int *h_num_matched);

/* Lines: the lines of a buffer that contain a pattern -- grep -F -f patterns -- or, with PFACX_LINES_INVERT, the lines that contain none (grep -v).
 *   LINES.  Let the input have n bytes and q_0 < ... < q_(K-1) be the positions of its '\n' bytes.  Line k, k < K, is the bytes [q_(k-1) + 1, q_k)
 *   with q_(-1) = -1: the '\n' is not part of the line, a '\r' in front of it is.  If n > 0 and the last byte is not '\n', the bytes behind the last
 *   '\n' are one more line (also when it is the only one); an input that ends in '\n' has no empty line behind it -- what wc -l and grep count.
 *   numLines is K or K + 1; n == 0 has no lines.
 *   A line MATCHES if the full result of PFAC_matchFromHost on a CPU platform over the whole buffer is non-zero at some position of the line.  No
 *   pattern contains '\n' (the pattern format ends a pattern there), so this is "a pattern occurs inside the line"; an empty line never matches.
 *   A caseless handle (PFACX_READ_NOCASE) folds patterns and input as in every other call; '\n' is not a letter, the line ends are those of the
 *   caller's bytes, and the caller's buffer is never modified.
 * PFACX_matchLines*: the selected lines in ascending order, each once however many matches it holds: lineStart[i] = the offset of the line's first
 * byte, lineLen[i] = its length without the '\n' (0 is possible under INVERT), lineIndex[i] (unless the pointer is null) = its 0-based number k.
 * *h_numLines and *h_numSelected are always written on success.
 * capacity: entries of each array, >= size (smaller: PFAC_STATUS_INVALID_PARAMETER).  lineStart / lineLen double as the scan's pair list, as the
 * arrays of every compacted call do: entries below `size` may be overwritten beyond the lines returned; nothing is written at or beyond capacity.
 * numLines <= size: the list is never truncated.
 * size >= 2^31, an unknown flag bit, a null pointer other than lineIndex: PFAC_STATUS_INVALID_PARAMETER; no pattern set: PFAC_STATUS_PATTERNS_NOT_READY;
 * size == 0: success, 0 lines, 0 selected, nothing touched; the device form on a host-only handle: PFAC_STATUS_LIB_NOT_EXIST.
 * Both calls are synchronous (the counts come to the host) and take the handle's lock like the other match calls.  The device form runs on whatever
 * kernel variant, walker, perf mode and texture mode the handle selects.  The host form follows PFAC_setPlatform: the CPU platforms, host-only
 * handles included, run entirely on the CPU (the CPU matcher plus memchr); the GPU platform runs the pipelined path of PFAC_matchFromHostReduce and
 * does the line work on the host.
 * MEMORY of the device form: grow-only handle scratch of about 0.32 bytes per input byte -- with B = (size + 15) / 2048 + 1: 256 B + (256 B + 256) +
 * 128 B + 2 x (4 (B + 1) + 4 (B + 1) + 4 B) bytes, each term rounded up to 256 -- a function of the size, not of the data: deviceScratchBytes of
 * PFACX_getInfo, freed by PFACX_trim, not allocated before the first lines call.
 * COST: the compacted scan without its ordering launches, one more streaming read of the input, and passes over size / 8 bytes of
 * bitmaps.
 *
 * PFACX_gatherLinesFromDevice: the lines (d_lineStart[i], d_lineLen[i]), i < numSelected, of d_input written as text into d_out, in list order:
 * line i's bytes, then a '\n' behind every line -- behind a last line that had none in the input too, as grep prints it.  *h_outBytes = the sum of
 * lineLen[i] + 1 (at most size + 1 for a list of PFACX_matchLines*).  More than outCapacity: PFACX_STATUS_OUTPUT_TRUNCATED, *h_outBytes still the
 * full size, nothing written at or beyond outCapacity, the contents of d_out unspecified.  numSelected == 0: success, *h_outBytes = 0, d_out may be
 * null.  The line arrays are DEVICE memory and the caller's contract, as the device offsets of the batch calls are: the kernels clamp every (start,
 * len) to [0, size] (*h_outBytes counts the clamped lengths), so bad arrays give wrong text but never an access outside the buffers.  The call reads
 * the caller's original bytes, never a folded copy.  Synchronous; scratch: 8 bytes per selected line (deviceScratchBytes). */
#define PFACX_LINES_INVERT 1u     /* select the lines that do NOT match (grep -v) */

PFAC_status_t PFACX_matchLinesFromDevice(PFAC_handle_t handle, char *d_input, size_t size, unsigned int flags,
                                         int *d_lineStart, int *d_lineLen, int *d_lineIndex /* may be NULL */, size_t capacity,
                                         size_t *h_numLines, size_t *h_numSelected);
PFAC_status_t PFACX_matchLinesFromHost  (PFAC_handle_t handle, char *h_input, size_t size, unsigned int flags,
                                         int *h_lineStart, int *h_lineLen, int *h_lineIndex /* may be NULL */, size_t capacity,
                                         size_t *h_numLines, size_t *h_numSelected);
PFAC_status_t PFACX_gatherLinesFromDevice(PFAC_handle_t handle, const char *d_input, size_t size,
                                          const int *d_lineStart, const int *d_lineLen, size_t numSelected,
                                          char *d_out, size_t outCapacity, size_t *h_outBytes);

/* Lines with context: the lines around the lines PFACX_matchLines* select -- grep -A after -B before (-C n: both n).  Lines, line numbers, "a line
 * matches", the caseless fold and PFACX_LINES_INVERT are exactly those of PFACX_matchLines*.
 *   SELECTED.  Let H be the set of line numbers the plain call would select with the same flags: the matching lines, or under PFACX_LINES_INVERT
 *   the lines that do not match.  With before and after -- any value -- the selected lines are { k in [0, numLines) : some h in H has
 *   h - before <= k <= h + after }, evaluated without wrap-around: before = after = 0xFFFFFFFF selects every line as soon as H is not empty, and
 *   nothing when it is.
 *   GROUPS.  A group is a maximal run of consecutive selected line numbers; groups are numbered from 0 in ascending order.  Two windows that touch
 *   or overlap are one group, as in grep, which prints "--" only where line numbers jump.
 * The selected lines come in ascending order, each once; lineStart, lineLen and lineIndex (may be null) are as in PFACX_matchLines*.  lineTag[i]
 * (unless the pointer is null) = group << 1 | m: m = 1 if line lineIndex[i] is in H -- the line grep prints with ':' --, m = 0 if it is context,
 * which grep prints with '-'.  There are at most (numLines + 1) / 2 groups, so a tag is a non-negative int.  *h_numMatching = |H|, *h_numGroups =
 * the number of groups, *h_numSelected = the length of the list; all four counts are written on every success.
 * Consequences: with before = after = 0 the list is exactly that of PFACX_matchLines* with the same flags, every tag has m = 1 and the groups are
 * the runs of adjacent matching lines; PFACX_gatherLinesFromDevice over (lineStart, lineLen) gives the text of grep -A / -B without its "--" lines;
 * a caller who wants separators inserts one wherever lineTag[i] >> 1 changes.
 * Everything else is PFACX_matchLines* word for word: capacity >= size entries of each array (smaller: PFAC_STATUS_INVALID_PARAMETER); lineStart /
 * lineLen double as the scan's pair list, entries below `size` may be overwritten beyond the lines returned, nothing is written at or beyond
 * capacity; numSelected <= numLines <= size, the list is never truncated.  size >= 2^31, an unknown flag bit, a null pointer other than lineIndex
 * and lineTag: PFAC_STATUS_INVALID_PARAMETER; no pattern set: PFAC_STATUS_PATTERNS_NOT_READY; size == 0: success, all four counts 0, nothing
 * touched; the device form on a host-only handle: PFAC_STATUS_LIB_NOT_EXIST.  Both calls are synchronous and take the handle's lock; the device
 * form runs on whatever kernel variant, walker, perf mode and texture mode the handle selects; the host form follows PFAC_setPlatform as
 * PFACX_matchLinesFromHost does (host-only handles included) and widens on the host; its temporaries are two bits per possible line
 * (PFAC_STATUS_ALLOC_FAILED if they cannot be had).
 * MEMORY of the device form: the scratch of PFACX_matchLinesFromDevice and, in a buffer of its own that a plain lines call never allocates, with
 * B = (size + 15) / 2048 + 1: (256 B + 256) + 128 B + 4 B + 4 B + 4 (B + 1) + 4 B + 4 B + 4 (B + 1) + 4 bytes, each term rounded up to 256 --
 * about 0.20 bytes per input byte, a function of the size alone: deviceScratchBytes of PFACX_getInfo, freed by PFACX_trim.
 * COST: the plain call plus four launches over size / 8 bytes of bitmaps by line number; the same for every before and after.
 * OUT OF SCOPE: "--" separators written by the gather; -m NUM; per-line match counts; context over streams or flows; context per segment of a
 * batch. */
PFAC_status_t PFACX_matchLinesContextFromDevice(PFAC_handle_t handle, char *d_input, size_t size, unsigned int flags,
                                                unsigned int before, unsigned int after,
                                                int *d_lineStart, int *d_lineLen, int *d_lineIndex /* may be NULL */, int *d_lineTag /* may be NULL */,
                                                size_t capacity, size_t *h_numLines, size_t *h_numSelected, size_t *h_numMatching, size_t *h_numGroups);
PFAC_status_t PFACX_matchLinesContextFromHost  (PFAC_handle_t handle, char *h_input, size_t size, unsigned int flags,
                                                unsigned int before, unsigned int after,
                                                int *h_lineStart, int *h_lineLen, int *h_lineIndex /* may be NULL */, int *h_lineTag /* may be NULL */,
                                                size_t capacity, size_t *h_numLines, size_t *h_numSelected, size_t *h_numMatching, size_t *h_numGroups);

/* Spans: the bytes of a buffer that belong to a match -- what grep --color highlights -- and the buffer with those bytes overwritten (redaction).
 *   COVERED.  Let r be the full result of PFAC_matchFromHost on a CPU platform over the whole buffer of n bytes and len(id) the length of pattern id.
 *   Byte b is covered if some position p <= b has r[p] > 0 and b < p + len(r[p]).  Every pattern that occurs at p is a prefix of the longest one
 *   there, so the covered bytes are the union of ALL occurrences of ALL patterns, not only of the longest.  A match always ends inside the buffer: no
 *   clipping.
 *   The SPANS are the maximal runs of covered bytes: ascending, disjoint and never adjacent -- matches that touch ("abab" under the pattern "ab") are
 *   one span.  numSpans <= (n + 1) / 2 <= n: a list of `size` entries is never truncated.
 *   A caseless handle (PFACX_READ_NOCASE): the spans of the folded set over the folded input; the caller's bytes are never modified, and the redaction
 *   reads the caller's original bytes.
 * PFACX_matchSpans*: span i is [spanStart[i], spanStart[i] + spanLen[i]), spanLen[i] >= 1; *h_coveredBytes = the sum of the lengths.  Both counts are
 * written on every success.  capacity: entries of each array, >= size (smaller: PFAC_STATUS_INVALID_PARAMETER).  The arrays double as the scan's pair
 * list, as the arrays of every compacted call do: entries below `size` may be overwritten beyond the spans returned; nothing is written at or beyond
 * capacity.
 * size >= 2^31 or a null pointer: PFAC_STATUS_INVALID_PARAMETER; no pattern set: PFAC_STATUS_PATTERNS_NOT_READY; size == 0: success, both counts 0,
 * nothing touched; the device form on a host-only handle: PFAC_STATUS_LIB_NOT_EXIST.
 * Both calls are synchronous (the counts come to the host) and take the handle's lock.  The device form runs on whatever kernel variant, walker, perf
 * mode and texture mode the handle selects.  The host form follows PFAC_setPlatform: the CPU platforms, host-only handles included, run on the CPU
 * matcher plus one sequential running-maximum pass, the list written in place (span i comes from position or pair >= i); the GPU platform runs the
 * pipelined path of PFAC_matchFromHostReduce and merges on the host.
 * MEMORY of the device form: grow-only handle scratch proportional to the PAIRS of the scan, not to the input -- with P pairs, S = min(P, (size + 1)
 * / 2) and B = (P + 511) / 512: 2 x 4 S + 4 B + 4 (B + 1) + 4 B + 4 (B + 1) + 256 bytes, each term rounded up to 256: 8.04 bytes per pair at most,
 * 4 bytes per input byte when every byte starts a match, nothing when nothing matches -- plus the device copy of the pattern lengths (4 bytes per
 * pattern, shared with the batch calls): deviceScratchBytes of PFACX_getInfo, freed by PFACX_trim.
 * COST: the compacted scan WITH its ordering launches, then eight small launches over the pairs; no further pass over the input.
 *
 * PFACX_redactSpansFromDevice: d_out[b] = fill for every b < size inside one of the numSpans spans, d_out[b] = d_input[b] for every other.  d_out ==
 * d_input is allowed (in place: only covered bytes are written); any other overlap of the two ranges: PFAC_STATUS_INVALID_PARAMETER.  numSpans == 0: a
 * plain copy, or nothing when in place (the span arrays may then be null).  size == 0: success, nothing touched.  Any alignment of d_input and d_out.
 * The span arrays are DEVICE memory and the caller's contract, like the arrays of the gather call: the kernel clamps every (start, len) to [0, size]
 * and expects the ascending disjoint list PFACX_matchSpans* returns; any other list gives unspecified text in d_out[0, size), never an access outside
 * the two buffers.  Asynchronous on the default stream, like PFAC_matchFromDevice: nothing comes back to the host.  Takes the handle's lock; needs no
 * pattern set and no scratch.  A host-only handle: PFAC_STATUS_LIB_NOT_EXIST. */
PFAC_status_t PFACX_matchSpansFromDevice(PFAC_handle_t handle, char *d_input, size_t size,
                                         int *d_spanStart, int *d_spanLen, size_t capacity,
                                         size_t *h_numSpans, size_t *h_coveredBytes);
PFAC_status_t PFACX_matchSpansFromHost  (PFAC_handle_t handle, char *h_input, size_t size,
                                         int *h_spanStart, int *h_spanLen, size_t capacity,
                                         size_t *h_numSpans, size_t *h_coveredBytes);
PFAC_status_t PFACX_redactSpansFromDevice(PFAC_handle_t handle, const char *d_input, size_t size,
                                          const int *d_spanStart, const int *d_spanLen, size_t numSpans,
                                          unsigned char fill, char *d_out);

/* Counts: which patterns occurred, and how often -- hit counts per rule, term frequencies, grep -c per keyword -- without a pair list.
 *   Let F = numOfPatterns and r be the full result of PFAC_matchFromHost on a CPU platform over the buffer.
 *   L[id] = #{p : r[p] == id} is the LONGEST histogram; A[id] = #{p : pattern id occurs at p} counts ALL occurrences: the number of pairs with that
 *   id in the all-match list of PFACX_matchAll*.  Every pattern that occurs at p is a prefix of the longest one there, so A[id] = L[id] + the sum of
 *   A[q] over all q with PFACX_TABLE_PREFIX_PATTERN[q] == id: the counts follow from the longest matches and never cost the expanded list.
 *   Duplicate lines are one pattern, counted under the highest of their IDs; the lower IDs stay 0.  A caseless handle (PFACX_READ_NOCASE) counts the
 *   folded set over the folded input; the caller's bytes are never modified.
 * counts[] is indexed by pattern id: numCounts >= F + 1 entries (smaller: PFAC_STATUS_INVALID_PARAMETER).  Entries [0, F] are written: counts[id] = A[id]
 * (PFACX_COUNT_LONGEST: L[id]), entry 0 = 0.  With PFACX_COUNT_ACCUMULATE the call ADDS to entries [1, F] instead and leaves entry 0 alone: many buffers,
 * the pieces of a stream.  Nothing at or beyond F + 1 is ever written.
 * PFACX_countFromDevice / ...FromHost: *h_total = what this call added -- the sum of the chain lengths over the longest pairs, exactly *h_num_matched of
 * PFACX_matchAll* for the same input; with PFACX_COUNT_LONGEST the number of pairs.  Both are synchronous (the scan's count comes to the host) and take
 * the handle's lock.  size >= 2^31, an unknown flag bit or a null pointer: PFAC_STATUS_INVALID_PARAMETER; no pattern set: PFAC_STATUS_PATTERNS_NOT_READY;
 * size == 0: success, *h_total = 0, the counts zeroed (untouched under ACCUMULATE); the device form on a host-only handle: PFAC_STATUS_LIB_NOT_EXIST.
 * The device form runs on whatever kernel variant, walker, perf mode and texture mode the handle selects.  The host form follows PFAC_setPlatform:
 * the CPU platforms, host-only handles included, run the CPU matcher plus a host loop over internal temporaries (4 bytes per input byte; a failed
 * allocation: PFAC_STATUS_ALLOC_FAILED); the GPU platform runs the pipelined path of PFAC_matchFromHostReduce (temporaries of 8 bytes per input byte)
 * and builds the histogram on the host.
 * PFACX_countPairsFromDevice: the same counts from a list of pair ids the caller already has -- the ids any compacted call returned (reduce, batch,
 * stream, flows); with ACCUMULATE over the pieces of a stream and its flush, the counts of the stream.  WITHOUT PFACX_COUNT_LONGEST EVERY PAIR ALSO
 * COUNTS FOR EVERY PATTERN ON ITS PREFIX CHAIN, SO THE LIST MUST BE A LONGEST LIST (one pair per position), NOT THE ALL-MATCH LIST OF PFACX_matchAll*
 * -- that list counts with PFACX_COUNT_LONGEST.  d_ids is DEVICE memory and the caller's contract: any 4-byte alignment; an id outside [1, F] is
 * ignored, never used as an index.  numPairs == 0: the counts zeroed, or nothing under ACCUMULATE (d_ids may then be null); numPairs >= 2^31:
 * PFAC_STATUS_INVALID_PARAMETER.  Asynchronous on the default stream, like PFACX_redactSpansFromDevice: nothing comes back to the host.
 * PFACX_countNonzeroFromDevice: the patterns that occurred -- (d_ids[i], d_outCounts[i]) = (id, d_counts[id]) for every non-zero entry of
 * d_counts[0, numCounts), ascending id.  *h_numDistinct = their number, *h_total = the sum of all entries; both are written on every success.  More than
 * `capacity`: PFACX_STATUS_OUTPUT_TRUNCATED, exactly the first `capacity` entries written and nothing behind them, both values still the full ones (with
 * capacity == 0 the arrays may be null).  numCounts == 0: success with zeros; numCounts >= 2^31: PFAC_STATUS_INVALID_PARAMETER.  Needs no pattern set:
 * d_counts[0, numCounts) is taken as given, entry 0 takes part like any other.  Synchronous.
 * MEMORY of the device forms: grow-only handle scratch, deviceScratchBytes of PFACX_getInfo, freed by PFACX_trim.  PFACX_countFromDevice: the pair list
 * of the scan in the pair scratch the all-match calls own, 8 bytes per input byte; 4 (F + 1) + 8 bytes for L and the total, each rounded up to 256;
 * and, for the all-occurrence form of a set in which a pattern is a prefix of another, the {prefix, chain length} table, 8 (F + 1) bytes, shared with
 * PFACX_matchAll*.  PFACX_countPairsFromDevice: the last two alone.  PFACX_countNonzeroFromDevice, with B = (numCounts + 255) / 256: 4 B + 4 (B + 1) +
 * 8 B + 16 bytes, each term rounded up to 256 (the same allocation as L: the larger of the two).
 * COST: the compacted scan WITHOUT its ordering launches, one pass over the pairs, two passes over the F patterns. */
#define PFACX_COUNT_LONGEST    1u   /* counts = L (one pattern per position) instead of A */
#define PFACX_COUNT_ACCUMULATE 2u   /* add to counts[] instead of overwriting it: many buffers, the pieces of a stream */

PFAC_status_t PFACX_countFromDevice(PFAC_handle_t handle, char *d_input, size_t size, unsigned int flags,
                                    unsigned long long *d_counts, size_t numCounts, size_t *h_total);
PFAC_status_t PFACX_countFromHost  (PFAC_handle_t handle, char *h_input, size_t size, unsigned int flags,
                                    unsigned long long *h_counts, size_t numCounts, size_t *h_total);
/* the same histogram from an id list the caller already has (the d_ids of ANY compacted call: reduce, batch, stream, flows) */
PFAC_status_t PFACX_countPairsFromDevice(PFAC_handle_t handle, const int *d_ids, size_t numPairs, unsigned int flags,
                                         unsigned long long *d_counts, size_t numCounts);
/* the patterns that occurred: (id, count) for every counts[id] != 0, ascending id */
PFAC_status_t PFACX_countNonzeroFromDevice(PFAC_handle_t handle, const unsigned long long *d_counts, size_t numCounts,
                                           int *d_ids, unsigned long long *d_outCounts, size_t capacity,
                                           size_t *h_numDistinct, unsigned long long *h_total);

/* Disjoint matches and replacement: the input tokenised into matches that do not overlap -- find_iter under leftmost-longest semantics -- and the text
 * with every token substituted by a string that belongs to its pattern (sed -e s/p1/r1/g -e ... in one pass, replace_all).
 *   Let r be the full result of PFAC_matchFromHost on a CPU platform over the buffer of n bytes and len(id) the length of pattern id.
 *   THE DISJOINT LIST is what this loop selects:
 *       p = 0
 *       while p < n:
 *           if r[p] > 0: take (r[p], p); p += len(r[p])
 *           else:        p += 1
 *   Among all matches the loop takes the one that starts leftmost, among those that start at one position the longest, and goes on behind the taken
 *   match: a match that starts inside a taken match is not taken, even if it reaches further.  The list is ascending, the ranges [p, p + len) are
 *   disjoint (they may touch), numTokens <= n; coveredBytes is the sum of the lengths.  Duplicate lines report under the highest id, as in every other
 *   call.  A caseless handle (PFACX_READ_NOCASE): the list of the folded set over the folded input; the caller's bytes are never modified, and the
 *   replacement reads the caller's original bytes.
 *   THE REPLACEMENT TEXT of a token list (id_k, start_k), k < numTokens, and a replacement table repl(id) is
 *       gap_0 repl(id_0) gap_1 repl(id_1) ... gap_numTokens
 *   where gap_k is the input between the end of token k - 1 (0 in front of the first token) and start_k, and the last gap runs to n.
 *   outBytes = n - the sum of len(id_k) + the sum of |repl(id_k)|: a size_t, computed in 64 bits; it can exceed 2^32.
 * PFACX_matchDisjoint*: token k is (ids[k], pos[k]).  Both counts are written on every success.  capacity: entries of each array, >= size (smaller:
 * PFAC_STATUS_INVALID_PARAMETER).  The arrays double as the scan's pair list, as the arrays of every compacted call do: entries below `size` may be
 * overwritten beyond the tokens returned; nothing is written at or beyond capacity.
 * size >= 2^31 or a null pointer: PFAC_STATUS_INVALID_PARAMETER; no pattern set: PFAC_STATUS_PATTERNS_NOT_READY; size == 0: success, both counts 0,
 * nothing touched; the device form on a host-only handle: PFAC_STATUS_LIB_NOT_EXIST.
 * Both calls are synchronous (the counts come to the host) and take the handle's lock.  The device form runs on whatever kernel variant, walker, perf
 * mode and texture mode the handle selects.  The host form follows PFAC_setPlatform: the CPU platforms, host-only handles included, run on the CPU
 * matcher plus the sequential loop above over the pairs, the list written in place (token k comes from pair >= k); the GPU platform runs the pipelined
 * path of PFAC_matchFromHostReduce and the same loop on the host.
 * MEMORY of the device form: grow-only handle scratch proportional to the PAIRS of the scan, not to the input -- with P pairs and B = (P + 511) / 512:
 * 2 x 4 P + P + 4 B + 4 (B + 1) + 256 bytes, each term rounded up to 256: 9.02 bytes per pair at most, nothing when nothing matches -- plus the device
 * copy of the pattern lengths (4 bytes per pattern, shared with the batch and the spans calls): deviceScratchBytes of PFACX_getInfo, freed by PFACX_trim.
 * COST: the compacted scan WITH its ordering launches, then 6 + ceil(log2(B)) small launches over the pairs; no further pass over the
 * input.
 *
 * PFACX_replaceFromDevice: the replacement text into d_out.  The replacement of pattern id is d_replBytes[d_replOff[id], d_replOff[id + 1]): numOff
 * >= F + 2 entries, entry 0 unused (with tokens, a smaller numOff: PFAC_STATUS_INVALID_PARAMETER); replBytes < 2^31; an empty replacement deletes the
 * match.  The token and offset arrays are DEVICE memory and the caller's contract, like the span arrays of the redaction: every start is clamped to
 * [0, size], the length of a token is the length of pattern id of the handle's CURRENT set, clipped to size - start, an id outside [1, F] makes the
 * token a no-op (nothing removed, nothing inserted), every offset is clamped to [0, replBytes], a decreasing pair of offsets is an empty replacement.
 * For the ascending disjoint list PFACX_matchDisjoint* returns the output is exactly the replacement text; any other list gives unspecified text and
 * an unspecified *h_outBytes, never an access outside the four buffers.  More than outCapacity: PFACX_STATUS_OUTPUT_TRUNCATED, *h_outBytes still the
 * full size, nothing written at or beyond outCapacity, the contents of d_out unspecified; with outCapacity == 0 d_out may be null: the size query.
 * [d_out, d_out + outCapacity) must not overlap [d_input, d_input + size): PFAC_STATUS_INVALID_PARAMETER (a text whose length changes has no in-place
 * form).  numTokens == 0: a plain copy (the token and replacement arrays may then be null); size == 0: success, *h_outBytes = 0; numTokens >= 2^31 or
 * size >= 2^31: PFAC_STATUS_INVALID_PARAMETER; no pattern set: PFAC_STATUS_PATTERNS_NOT_READY -- unlike the redaction the call needs the pattern
 * lengths; a host-only handle: PFAC_STATUS_LIB_NOT_EXIST.  Any alignment of d_input, d_out and d_replBytes.  Synchronous (the size comes to the host);
 * takes the handle's lock.  Scratch: 8 bytes per token (the same allocation as the selection's).  Matches that are deleted and touch each other own
 * no output byte; the tile of the output they fall into still walks them.
 * PFACX_replaceFromHost: the same contract over host arrays: one sequential loop of memcpy whatever the platform, host-only handles included. */
PFAC_status_t PFACX_matchDisjointFromDevice(PFAC_handle_t handle, char *d_input, size_t size,
                                            int *d_ids, int *d_pos, size_t capacity,
                                            size_t *h_numTokens, size_t *h_coveredBytes);
PFAC_status_t PFACX_matchDisjointFromHost  (PFAC_handle_t handle, char *h_input, size_t size,
                                            int *h_ids, int *h_pos, size_t capacity,
                                            size_t *h_numTokens, size_t *h_coveredBytes);
PFAC_status_t PFACX_replaceFromDevice(PFAC_handle_t handle, const char *d_input, size_t size,
                                      const int *d_ids, const int *d_pos, size_t numTokens,
                                      const int *d_replOff, size_t numOff, const char *d_replBytes, size_t replBytes,
                                      char *d_out, size_t outCapacity, size_t *h_outBytes);
PFAC_status_t PFACX_replaceFromHost  (PFAC_handle_t handle, const char *h_input, size_t size,
                                      const int *h_ids, const int *h_pos, size_t numTokens,
                                      const int *h_replOff, size_t numOff, const char *h_replBytes, size_t replBytes,
                                      char *h_out, size_t outCapacity, size_t *h_outBytes);

/* Rule sets: which segments of a batch contain EVERY pattern of a rule -- a Snort rule's content strings that must all occur in one packet, "ERROR
 * and payment-service in the same line".  The all-match list says which pattern occurred where; this is the segmented group-by over (segment, rule)
 * behind it, done on the device behind the scan.
 *   A RULE SET is R rules over the handle's current pattern set of F patterns: rule r is the set of pattern ids h_rulePatterns[h_ruleOff[r],
 *   h_ruleOff[r + 1]).  Pattern id OCCURS IN SEGMENT k if the all-match list of segment k alone (PFACX_matchAll* / PFACX_matchBatch*) contains a pair
 *   with that id: occurrences lie entirely inside the segment; a pattern that is only a proper prefix of the longest one at a position counts; a
 *   match that crosses a segment border does not.  Rule r FIRES on segment k if every one of its patterns occurs in k.
 *   A caseless handle (PFACX_READ_NOCASE) folds patterns and input as in every other call; the caller's bytes are never modified.  Duplicate pattern
 *   lines are one pattern and a rule may name any of their ids: at open every named id is resolved to the id that is reported (the highest), and
 *   after that ids repeated within one rule count once.
 * PFACX_rulesOpen copies the arrays.  PFAC_STATUS_INVALID_PARAMETER unless: every rule has 1 to 32 distinct patterns after resolution, every id lies
 * in [1, F], h_ruleOff[0] == 0 and the offsets never decrease, 0 < numRules < 2^24 (the total number of ids is an int: below 2^31), no pointer is
 * null.  Without a pattern set: PFAC_STATUS_PATTERNS_NOT_READY.
 * THE FIRED LIST: the pairs (segment, rule) = (firedSeg[i], firedRule[i]) in ascending segment order, ascending rule order within a segment, each
 * pair once.  segFirst (numSegments + 1 entries, may be NULL): the fired rules of segment k are entries [segFirst[k], segFirst[k + 1]).  The list can
 * be longer than the input -- one byte that is a pattern named by a thousand rules fires a thousand rules -- so `capacity` (entries of each array)
 * is free and need not be >= size.  A list longer than capacity: exactly its first `capacity` pairs are written and nothing behind them,
 * *h_numFired is the full count, segFirst is complete, and the call returns PFACX_STATUS_OUTPUT_TRUNCATED; with capacity == 0 the two arrays may be
 * null: the count query.  The scan's own pair list lives in the handle's pair scratch, never in the caller's arrays.
 * Offsets follow the rules of PFACX_matchBatch*: host offsets are validated (first 0, last `size`, never decreasing), device offsets are clamped and
 * never checked (wrong offsets: a wrong list, never an access outside the buffers).  offsets == NULL with numSegments == 1: the whole buffer is one
 * segment.  PFAC_STATUS_INVALID_PARAMETER: numSegments >= 2^31, size >= 2^31, a null pointer other than those named above, offsets == NULL with
 * numSegments != 1, numSegments == 0 with size > 0.  size == 0: success, 0 fired, segFirst all zero where given and numSegments > 0.  The device form on
 * a host-only handle: PFAC_STATUS_LIB_NOT_EXIST.  Both calls are synchronous (the count comes to the host) and take the handle's lock.
 * The device form runs on whatever kernel variant, walker, perf mode and texture mode the handle selects.  The host form follows PFAC_setPlatform:
 * the CPU platforms, host-only handles included, run on the CPU -- the longest pairs segment by segment, their prefix chains, one mask per touched
 * rule (temporaries: 4 bytes per input byte and per segment, 4 per rule); the GPU platform runs the pipelined path of PFACX_matchBatchFromHost and the
 * same loop on the host.
 * A rule set belongs to the pattern set that was loaded when it was opened: after the handle reads or loads another set the ids mean something
 * else, every match call returns PFAC_STATUS_INVALID_PARAMETER and only PFACX_rulesClose works.  Any number of rule sets per handle; PFAC_destroy
 * closes them, as it closes streams and flow sets.
 * MEMORY: the device tables of a rule set -- with I ids in all rules after resolution: 4 (F + 2) + 4 I + 4 R bytes, three allocations made by the first
 * device call (opening on a host-only handle works) -- are state: counted under deviceTableBytes of PFACX_getInfo, kept by PFACX_trim, freed by
 * PFACX_rulesClose.  What a device call stages is grow-only handle scratch, deviceScratchBytes, given back by PFACX_trim: 8 (numSegments + 1) bytes
 * rounded up to 256 for the per-segment counts and their scan, and what the scan behind it shares with other calls: the pair list (8 bytes per input
 * byte, the pair scratch of PFACX_matchAll* / PFACX_countFromDevice), 4 (numSegments + 1) bytes for the first pair of each segment, the {prefix, chain
 * length} table (8 (F + 1) bytes), the pattern lengths (4 (F + 1) bytes) and the fix-up's scratch of PFACX_matchBatchFromDeviceReduce.  Nothing is
 * sized by segments x rules.
 * COST: the ordered compacted batch scan, then two passes over the pairs whose work follows the pairs times the memberships of the
 * patterns on their prefix chains.
 *
 * CONDITIONED RULE SETS (PFACX_rulesOpenEx): a rule's member is a pattern id with a polarity and a position window -- Snort's
 * content:!"x", offset and depth; "starts with ERROR, contains payment, does not contain retry".  Rule r is the members h_members[h_ruleOff[r],
 * h_ruleOff[r + 1]).  The result is an ordinary PFACX_rules_t: the match calls, PFACX_rulesClose, the fired list, segFirst, capacity, truncation, the
 * count query, offsets, the generation check, PFAC_destroy, PFACX_trim, the lock and the caseless fold are exactly as above.
 *   An OCCURRENCE is as above: pattern id at segment-relative start s, of length L, wholly inside a segment of n bytes; a proper prefix of the
 *   longest pattern at a position counts.
 *   The occurrence SATISFIES THE MEMBER'S WINDOW if, with a = s -- or a = n - s - L with PFACX_RULE_FROM_END --, a >= offset and (depth == 0 or
 *   a + L <= offset + depth); evaluated without wrap-around (offset = depth = 0xFFFFFFFF satisfies nothing).  offset 0, depth L: startswith; the same
 *   with PFACX_RULE_FROM_END: endswith; Snort's offset:o; depth:d maps directly; {id, 0, 0, 0} is every occurrence.
 *   A positive member HOLDS if some occurrence of its pattern satisfies its window; a PFACX_RULE_NOT member holds if none does.  The rule FIRES on
 *   a segment if every member holds.  The test is made for every pattern on a prefix chain by itself: over "GET /admin" the member {GET, depth 3}
 *   holds although the longest pattern at 0, `GET /admin`, fails that window.
 *   Ids are resolved as above (duplicate lines: the reported id); members equal in (resolved id, flags, offset, depth) count once; the same id with
 *   another window or polarity is another member; a rule that contradicts itself never fires.
 * PFAC_STATUS_INVALID_PARAMETER: everything PFACX_rulesOpen refuses (1 to 32 distinct MEMBERS after resolution), a flag bit other than the two
 * below, a rule without a positive member (it would fire on segments in which nothing matches, which the pass never visits).
 * A set whose members are all {id, 0, 0, 0} gives the list of PFACX_rulesOpen over the same ids on every input.
 * Device offsets are clamped to [0, size] before they become a segment's bounds; a pair whose position relative to them is negative, or whose
 * pattern ends behind them, satisfies nothing; no input byte is read for the test (wrong offsets: a wrong list, never an access outside the buffers).
 * MEMORY: a conditioned set adds 8 bytes per member after resolution to its device tables: 4 (F + 2) + 4 I + 4 R + 8 I bytes, four allocations; a
 * set opened by PFACX_rulesOpen allocates nothing new.  A device call of a conditioned set stages the pattern lengths (4 (F + 1) bytes of handle
 * scratch) also when d_offsets is NULL.  The host form of a conditioned set keeps 8 bytes per input byte instead of 4.
 * OUT OF SCOPE: rules of negated members only, minimum counts, more than 32 members, conditioned members over streams or flows (plain rule sets over flows: PFACX_flowRules*; distance / within: below).
 *
 * ORDERED RULE MEMBERS (PFACX_rulesOpenSeq): members that also carry Snort's relative modifiers -- "B starts at least `distance` bytes
 * behind the end of A and ends within `within` bytes of it": `timeout` within 40 bytes after `payment-service`; `User-Agent:` and then `sqlmap`.
 * Rule r is the members h_members[h_ruleOff[r], h_ruleOff[r + 1]) of type PFACX_rule_seq_member_t; PFACX_rule_member_t is unchanged.  The result is
 * an ordinary PFACX_rules_t: the match calls, PFACX_rulesClose, the fired list, segFirst, capacity, truncation, the count query, offsets (host
 * offsets validated, device offsets clamped), the generation check, PFAC_destroy, PFACX_trim, the lock and the caseless fold are exactly as above.
 *   An occurrence and a member's own window {flags & PFACX_RULE_FROM_END, offset, depth} are exactly those of PFACX_rulesOpenEx: a proper prefix of
 *   the longest pattern at a position counts, the occurrence lies wholly inside the segment.
 *   A member with PFACX_RULE_RELATIVE is tied to the member immediately in front of it in the rule, its predecessor.  A maximal run "member without
 *   PFACX_RULE_RELATIVE, then PFACX_RULE_RELATIVE members" is a CHAIN m_0 .. m_c.  The chain HOLDS if there are occurrences o_0 .. o_c such that o_j
 *   is an occurrence of m_j's pattern that satisfies m_j's own window and, for every j >= 1, with e = start(o_j-1) + len(o_j-1): start(o_j) >= e +
 *   distance_j and (within_j == 0 or start(o_j) + len(o_j) <= e + within_j) -- evaluated without wrap-around (distance = 0xFFFFFFFF satisfies
 *   nothing).  Any such assignment will do: existence, what Snort's backtracking search decides; never a greedy first or last occurrence.  distance
 *   is unsigned, so two neighbouring members of a chain never share a byte.  {PFACX_RULE_RELATIVE, distance 0, within 0}: somewhere behind its
 *   predecessor, not overlapping it; within == len(B) with distance 0: adjacent; within < len(B): never.
 *   The rule FIRES on a segment if every chain holds and every member outside a chain -- positive or PFACX_RULE_NOT, without PFACX_RULE_RELATIVE --
 *   holds as under PFACX_rulesOpenEx.  Chains are independent of each other: two chains may use the same occurrence.
 *   A rule that contains a PFACX_RULE_RELATIVE member keeps its members in the order given and nothing is merged (ids are resolved to the reported
 *   id, as everywhere); 32 members at most.  A rule without one is treated exactly as PFACX_rulesOpenEx treats it, merging of equal members included.
 * PFAC_STATUS_INVALID_PARAMETER: everything PFACX_rulesOpenEx refuses, a flag bit other than the three below, PFACX_RULE_RELATIVE on the first member
 * of a rule, together with PFACX_RULE_NOT, or behind a PFACX_RULE_NOT member, distance or within non-zero on a member without PFACX_RULE_RELATIVE.
 * A set without any PFACX_RULE_RELATIVE member gives the list of PFACX_rulesOpenEx over the same members on every input, from the same kernels.
 * The device form verifies a rule whose members all passed their own tests (a CANDIDATE) in the block that owns the segment, from the pairs'
 * positions and the pattern lengths: no input byte is read, device offsets are clamped exactly as for a conditioned set.  The host form verifies
 * it by a loop over the segment's occurrences.  Both are exact.
 * MEMORY: a set with a chain adds, with K links (the members of all chains), 4 (R + 1) + 20 K bytes in two allocations to its device tables (state:
 * deviceTableBytes, kept by PFACX_trim, freed by PFACX_rulesClose); a device call of such a set adds 8 bytes per pair of the scan -- two arrays of 4
 * bytes per pair, each rounded up to 256 -- to the handle's grow-only rules scratch (deviceScratchBytes, freed by PFACX_trim).  A set without a
 * chain adds neither.
 * COST: the conditioned passes, plus, in both passes, for every candidate with chains one walk over the pairs of its segment per link:
 * candidates x links x pairs of the segment.  A rule whose first member is common and whose segments are huge (one segment of many MiB) is what this
 * is not for: give such a rule a rare member outside the chain, or cut the input into records.
 * OUT OF SCOPE: negative distance, negated relative members, relative to a member other than the one in front, isdataat and byte tests, minimum
 * counts, ordered members over streams or flows (plain rule sets over flows: PFACX_flowRules*), a report of where the chain matched. */
#define PFACX_RULE_NOT      1u   /* the member holds if NO occurrence satisfies its window (content:!"...") */
#define PFACX_RULE_FROM_END 2u   /* the window is measured from the segment's end instead of its start */
#define PFACX_RULE_RELATIVE 4u   /* PFACX_rulesOpenSeq: distance / within tie the member to the one in front of it */
typedef struct { int pattern; unsigned int flags, offset, depth; } PFACX_rule_member_t;   /* depth 0: no upper bound */
typedef struct { int pattern; unsigned int flags, offset, depth, distance, within; } PFACX_rule_seq_member_t;  /* within 0: no upper bound */
typedef struct PFACX_rules_s *PFACX_rules_t;
PFAC_status_t PFACX_rulesOpen (PFAC_handle_t handle, const int *h_ruleOff /* numRules + 1 */, const int *h_rulePatterns,
                               size_t numRules, PFACX_rules_t *rules);
PFAC_status_t PFACX_rulesOpenEx(PFAC_handle_t handle, const int *h_ruleOff /* numRules + 1 */, const PFACX_rule_member_t *h_members,
                                size_t numRules, PFACX_rules_t *rules);
PFAC_status_t PFACX_rulesOpenSeq(PFAC_handle_t handle, const int *h_ruleOff /* numRules + 1 */, const PFACX_rule_seq_member_t *h_members,
                                 size_t numRules, PFACX_rules_t *rules);
PFAC_status_t PFACX_rulesClose(PFACX_rules_t rules);
PFAC_status_t PFACX_rulesMatchFromDevice(PFACX_rules_t rules, char *d_input, size_t size, const size_t *d_offsets, size_t numSegments,
                                         int *d_firedSeg, int *d_firedRule, size_t capacity, size_t *d_segFirst /* numSegments + 1, may be NULL */,
                                         size_t *h_numFired);
PFAC_status_t PFACX_rulesMatchFromHost  (PFACX_rules_t rules, char *h_input, size_t size, const size_t *h_offsets, size_t numSegments,
                                         int *h_firedSeg, int *h_firedRule, size_t capacity, size_t *h_segFirst /* may be NULL */,
                                         size_t *h_numFired);

/* Flow-rule sets: rules whose patterns arrive in different pieces of a flow -- `User-Agent:` in one packet, `sqlmap` three batches later.  PFACX_flows*
 * reports every occurrence of every flow exactly once however the flow was cut; PFACX_rules* says which segments of ONE buffer hold every pattern of
 * a rule.  This is what joins them: per-flow state that outlives a call, and the decision "complete now, not before", on the device behind the
 * flows call, without a copy of the pairs to the host.
 *   A FLOW-RULE SET is R plain rules over the handle's current pattern set -- h_ruleOff / h_rulePatterns exactly as PFACX_rulesOpen takes, validates
 *   and resolves them (1 to 32 distinct patterns a rule after resolution of duplicate lines, 0 < numRules < 2^24) -- plus the state of numFlows
 *   flows, 0 < numFlows < 2^31, all empty at open.
 *   THE CALLS TAKE PAIRS, NOT BYTES: what PFACX_flowsMatchFromDevice / ...FromHost just returned -- `ids`, `pieceFirst`, the call's h_flowIds and
 *   *h_num_matched as numPairs -- or what PFACX_flowsFlush returned: `ids`, `first` and the flows named.  No position is read.  The set is
 *   independent of the PFACX_flows_t: the caller uses the same flow indices and mirrors a flow's flush or reset with PFACX_flowRulesReset.  A single
 *   stream is a flow set of one flow.
 *   Pattern id HAS OCCURRED in flow f if some pair fed for f since its last reset carries that id on its prefix chain (PFACX_TABLE_PREFIX_PATTERN;
 *   the pair's own id included): a proper prefix of the longest pattern at a position counts.
 *   Rule r FIRES on piece k (flow f = h_flowIds[k]) in the call after whose pairs every pattern of r has occurred in f for the first time.  Each
 *   (flow, rule) fires once until the flow is reset; two members that arrive in the same call fire the rule once; pairs that only repeat what was
 *   seen fire nothing.  Over one stream fed completely, flush included, the rules fired over all calls are exactly the fired list of
 *   PFACX_rulesMatchFromHost over the stream as one segment.
 * THE FIRED LIST: the pairs (piece, rule) = (firedPiece[i], firedRule[i]) in ascending piece order, ascending rule order within a piece.
 * pieceFiredFirst (numPieces + 1 size_t, may be NULL): the rules fired on piece k are entries [pieceFiredFirst[k], pieceFiredFirst[k + 1]).
 * `capacity` (entries of each array) is free; with capacity == 0 the two arrays may be null: the count query.
 * STATE CHANGES ONLY ON SUCCESS.  A list longer than capacity: exactly its first `capacity` pairs are written and nothing behind them, *h_numFired is
 * the full count, pieceFiredFirst is complete, the call returns PFACX_STATUS_OUTPUT_TRUNCATED -- and NO FLOW'S STATE CHANGES: repeat the call with
 * larger arrays and get the whole list.  Any status but PFAC_STATUS_SUCCESS leaves every flow unchanged.  Feeding the same pairs twice is harmless:
 * the second list is empty.
 * Host arrays are validated completely: every h_flowIds[k] < numFlows, no flow twice in one call, and for the host form pieceFirst[0] == 0,
 * pieceFirst[numPieces] == numPairs, never decreasing.  Device arrays are the caller's contract: a pieceFirst entry is clamped to [0, numPairs], a
 * decreasing pair is an empty piece, an id outside [1, F] is skipped (in both forms) -- wrong device arrays give a wrong list, never an access outside
 * the buffers.  The pair arrays are never written.  PFAC_STATUS_INVALID_PARAMETER: a null pointer other than those named above (d_pairIds may be
 * null with numPairs == 0), numPairs or numPieces >= 2^31, numFlows == 0 or >= 2^31, numPieces == 0 with numPairs > 0.  numPieces == 0 with
 * numPairs == 0: success, nothing fired, nothing written.  The device form on a host-only handle: PFAC_STATUS_LIB_NOT_EXIST.  Without a pattern
 * set: PFAC_STATUS_PATTERNS_NOT_READY.
 * PFACX_flowRulesReset empties the n named flows (ids below numFlows), or, with (NULL, 0), all flows.  A set is fed by one kind of call, host or
 * device, until a reset of all flows (the other kind: PFAC_STATUS_INVALID_PARAMETER), as flow sets are.  After the handle reads or loads another
 * pattern set the ids mean something else: every call returns PFAC_STATUS_INVALID_PARAMETER and only PFACX_flowRulesClose works, as for rule sets.
 * Calls take the handle's lock and the set's own and are synchronous.  Any number of sets per handle; PFAC_destroy closes them.  A caseless handle
 * needs nothing special: the ids are those of the folded set.  The host form is a loop over the host arrays on every platform.
 * MEMORY, with F patterns, I ids in all rules after resolution, and D distinct ids among them: a flow holds a bitmap of D bits, ceil(D / 32) 32-bit
 * words.  A device-fed set makes, on its first device call, ONE allocation of numFlows x 4 x ceil(D / 32) bytes for the bitmaps and five for its
 * tables -- 4 (F + 2) + 4 I bytes for the rule set inverted by pattern, 4 (R + 1) for the first member of each rule (its full mask follows from
 * their number), 4 I for the forward list rule -> bits and 4 (F + 1) for the table pattern -> bit: 4 (F + 2) + 8 I + 4 (R + 1) + 4 (F + 1) bytes.  All
 * of it is state: counted under deviceTableBytes of PFACX_getInfo, kept by PFACX_trim, freed by PFACX_flowRulesClose.  What a device call stages is
 * grow-only handle scratch, deviceScratchBytes, given back by PFACX_trim: 4 numPieces bytes for the flow ids and 8 (numPieces + 1) for the fired
 * counts and their scan, each rounded up to 256, and the {prefix, chain length} table (8 (F + 1) bytes) it shares with other calls.  A host-fed set
 * keeps the same bitmaps in host memory.  Nothing is sized by flows x rules or pieces x rules.
 * COST: two passes over the pairs whose work follows the pairs times the memberships of the patterns on their prefix chains, at most
 * 32 bit tests per rule a piece touches, and one pass that sets bits.
 * OUT OF SCOPE: conditioned and ordered members over flows (PFACX_rulesOpenEx / PFACX_rulesOpenSeq members), a report of which call supplied which
 * member, device-resident flow ids, changing rules without reopening. */
typedef struct PFACX_flowRules_s *PFACX_flowRules_t;
PFAC_status_t PFACX_flowRulesOpen(PFAC_handle_t handle, const int *h_ruleOff /* numRules + 1 */, const int *h_rulePatterns, size_t numRules,
                                  size_t numFlows, PFACX_flowRules_t *fr);
PFAC_status_t PFACX_flowRulesClose(PFACX_flowRules_t fr);
PFAC_status_t PFACX_flowRulesReset(PFACX_flowRules_t fr, const unsigned int *h_flowIds, size_t n);   /* NULL, 0: all flows */
PFAC_status_t PFACX_flowRulesPairsFromDevice(PFACX_flowRules_t fr, const int *d_pairIds, size_t numPairs, const int *d_pieceFirst /* numPieces + 1 */,
                                             const unsigned int *h_flowIds, size_t numPieces, int *d_firedPiece, int *d_firedRule, size_t capacity,
                                             size_t *d_pieceFiredFirst /* numPieces + 1, may be NULL */, size_t *h_numFired);
PFAC_status_t PFACX_flowRulesPairsFromHost  (PFACX_flowRules_t fr, const int *h_pairIds, size_t numPairs, const int *h_pieceFirst /* numPieces + 1 */,
                                             const unsigned int *h_flowIds, size_t numPieces, int *h_firedPiece, int *h_firedRule, size_t capacity,
                                             size_t *h_pieceFiredFirst /* may be NULL */, size_t *h_numFired);

/* Per-segment counts: how often each pattern occurred in each segment of a batch -- the term-document matrix of a corpus, the keyword feature vector
 * of each log line or packet, grep -c per keyword per file -- as a sparse matrix in CSR form.  It is the join of PFACX_count* (how often, over one
 * buffer) and PFACX_rules* (in which segment), without the expanded all-match list and without a dense segments x F matrix.
 *   Offsets follow the rules of PFACX_matchBatch*: numSegments + 1 entries, first 0, last `size`, never decreasing, empty segments allowed.
 *   For segment k, A_k[id] is the number of pairs with that id in the all-match list of segment k alone (PFACX_matchAll* / PFACX_matchBatch*): a
 *   proper prefix of the longest pattern at a position counts; a match that crosses a segment border does not.  With PFACX_COUNT_LONGEST the call
 *   counts L_k[id], the number of positions of segment k whose longest pattern is id.  Duplicate pattern lines count under the reported (highest)
 *   id.  A caseless handle (PFACX_READ_NOCASE) counts the folded set over the folded input; the caller's bytes are never modified.
 *   THE COUNT LIST is the entries (id, count) with count != 0, in ascending segment order and ascending id within a segment.
 * Output is CSR: ids[i] (int) and counts[i] (unsigned int; a count is at most size < 2^31); the entries of segment k are [segFirst[k],
 * segFirst[k + 1]).  segFirst has numSegments + 1 size_t entries and is REQUIRED whenever numSegments > 0: it is the row pointer.  *h_numEntries is
 * the full length of the list.  *h_total is the sum of all counts: *h_num_matched of PFACX_matchAllBatchFromDevice over the same batch, or the
 * number of longest pairs under PFACX_COUNT_LONGEST.
 * Capacity and truncation are those of the fired list of PFACX_rules*: `capacity` (entries of each array) is free and need not be >= size.  A list
 * longer than capacity: exactly its first `capacity` entries are written and nothing behind them, segFirst, *h_numEntries and *h_total are complete,
 * and the call returns PFACX_STATUS_OUTPUT_TRUNCATED; with capacity == 0 the two arrays may be null: the count query.  The scan's own pair list
 * lives in the handle's pair scratch, never in the caller's arrays.
 * The only flag is PFACX_COUNT_LONGEST; any other bit, PFACX_COUNT_ACCUMULATE included: PFAC_STATUS_INVALID_PARAMETER.  offsets == NULL with
 * numSegments == 1: the whole buffer is one segment.  Host offsets are validated, device offsets are clamped and never checked (wrong offsets: a
 * wrong list, never an access outside the buffers).  PFAC_STATUS_INVALID_PARAMETER: numSegments >= 2^31, size >= 2^31, a null pointer other than
 * those named above, offsets == NULL with numSegments != 1, numSegments == 0 with size > 0.  No pattern set: PFAC_STATUS_PATTERNS_NOT_READY.  size ==
 * 0: success, both values 0, segFirst all zero where numSegments > 0.  A device form on a host-only handle: PFAC_STATUS_LIB_NOT_EXIST.  All three
 * calls are synchronous (the values come to the host) and take the handle's lock.
 * The device form runs on whatever kernel variant, walker, perf mode and texture mode the handle selects.  The host form follows PFAC_setPlatform:
 * the CPU platforms, host-only handles included, run on the CPU -- the longest pairs segment by segment, their prefix chains, one counter per touched
 * pattern (temporaries: 4 bytes per input byte and per segment, 4 per pattern; a failed allocation: PFAC_STATUS_ALLOC_FAILED); the GPU platform runs
 * the pipelined path of PFACX_matchBatchFromHost and the same loop on the host.  A pattern set that another thread replaces during a host call:
 * PFAC_STATUS_PATTERNS_NOT_READY, no count written.
 * PFACX_countBatchPairsFromDevice: the same list from a LONGEST pair list the caller already has -- d_matched_result and d_segFirst of
 * PFACX_matchBatchFromDeviceReduce, or `ids` and `first` of a PFACX_flows* call (per-flow counts); it runs no scan.  The warning of
 * PFACX_countPairsFromDevice applies: WITHOUT PFACX_COUNT_LONGEST EVERY PAIR ALSO COUNTS FOR EVERY PATTERN ON ITS PREFIX CHAIN, so an all-match
 * list counts with PFACX_COUNT_LONGEST.  The arrays are DEVICE memory and the caller's contract: d_pairIds at any 4-byte alignment, an id outside
 * [1, F] is ignored and never used as an index; d_segFirstPairs (numSegments + 1 ints; NULL with numSegments == 1: one segment of all pairs) is
 * clamped to [0, numPairs] where it is read, a decreasing pair is an empty segment.  numPairs >= 2^31: PFAC_STATUS_INVALID_PARAMETER; numPairs ==
 * 0 (d_pairIds may then be null): success, zeros, segFirst zeroed.
 * A SEGMENT IS ONE BLOCK'S WORK on the device: 256 threads walk its pairs once for every window of 8192 pattern ids it has an id in.  Batches of
 * packets, lines and documents are what the call is for; counts over one huge buffer are what PFACX_countFromDevice is for.
 * MEMORY of the device forms: grow-only handle scratch, deviceScratchBytes of PFACX_getInfo, freed by PFACX_trim: 8 (numSegments + 1) + 8 bytes
 * rounded up to 256 for the per-segment entry counts, their scan and the sum, and -- PFACX_countBatchFromDevice only -- what the scan behind it
 * shares with other calls: the pair list (8 bytes per input byte, the pair scratch of PFACX_matchAll* / PFACX_countFromDevice / PFACX_rules*),
 * 4 (numSegments + 1) bytes for the first pair of each segment, the pattern lengths (4 (F + 1) bytes) and the fix-up's scratch of
 * PFACX_matchBatchFromDeviceReduce; both forms, for the all-occurrence counts of a set in which a pattern is a prefix of another, the {prefix, chain
 * length} table (8 (F + 1) bytes).  Nothing is sized by segments x patterns.
 * COST: the ordered compacted batch scan, then two passes over the pairs whose work follows the pairs times their chain lengths
 * times the windows a segment touches -- the LDS atomics and, for the all-occurrence counts, the reads of the {prefix, chain length} table too: a
 * pair's whole chain is read again in every window its segment touches, and an id of another window costs its table load for nothing -- and a
 * one-block scan of the numSegments entry counts between the passes, which is what millions of segments pay for (5m has the figures).
 * OUT OF SCOPE: a dense segments x F output, PFACX_COUNT_ACCUMULATE across calls, one long segment split over several blocks, counts over flows
 * with carried state (the pairs form covers per-call flow output), minimum-count rule members. */
PFAC_status_t PFACX_countBatchFromDevice(PFAC_handle_t handle, char *d_input, size_t size, const size_t *d_offsets, size_t numSegments,
                                         unsigned int flags, int *d_ids, unsigned int *d_counts, size_t capacity,
                                         size_t *d_segFirst /* numSegments + 1 */, size_t *h_numEntries, unsigned long long *h_total);
PFAC_status_t PFACX_countBatchFromHost  (PFAC_handle_t handle, char *h_input, size_t size, const size_t *h_offsets, size_t numSegments,
                                         unsigned int flags, int *h_ids, unsigned int *h_counts, size_t capacity,
                                         size_t *h_segFirst /* numSegments + 1 */, size_t *h_numEntries, unsigned long long *h_total);
PFAC_status_t PFACX_countBatchPairsFromDevice(PFAC_handle_t handle, const int *d_pairIds, size_t numPairs,
                                              const int *d_segFirstPairs /* numSegments + 1 */, size_t numSegments, unsigned int flags,
                                              int *d_ids, unsigned int *d_counts, size_t capacity, size_t *d_segFirst,
                                              size_t *h_numEntries, unsigned long long *h_total);

/* Whole-word and delimiter-bounded matches: the occurrences whose neighbours in the input are not in a byte class -- `grep -w -F -f`, `grep -x`, "the
 * field of a CSV record equals one of 100 000 keys", term frequencies that do not count `the` inside `other`.
 *   A CLASS W is a set of byte values, given as 256 bits in `unsigned int cls[8]`: byte b is in W if bit b & 31 of cls[b >> 5] is set.  h_class == NULL:
 *   the default class [0-9A-Za-z_].  The eight words are HOST memory in every call and are copied.
 *   Let the input have n bytes.  An occurrence of pattern id at p, of length L = len(id), is BOUNDED if (p == 0 or in[p - 1] is not in W) and (p + L == n
 *   or in[p + L] is not in W).  This is the test of grep -w; it does not ask whether the pattern's own edge bytes are in W (a pattern "-x-" is bounded
 *   between two spaces, where a regular expression's \b would refuse it).
 *   THE WORD LIST (flags 0): for every position p at which some pattern has a bounded occurrence, the pair (the LONGEST such pattern, p); positions
 *   ascend.  The longest pattern at p may fail the test where a shorter one -- a proper prefix of it -- passes: `foo` and `foobar` over "foo bar" and
 *   over "foobar".  The list is never longer than the list of PFAC_matchFromDeviceReduce, so it has at most `size` pairs.
 *   ALL (PFACX_WORDS_ALL): every bounded occurrence; positions ascend, within one position the longest pattern comes first, as in PFACX_matchAll*.  This
 *   list can be longer than the input: the patterns `a`, `a a`, `a a a`, `a a a a`, `a a a a a` over the 9 bytes "a a a a a" give 15 pairs.  So the
 *   count is a size_t and truncation follows PFACX_matchAll* exactly: the first `capacity` pairs are written, nothing at or behind `capacity`,
 *   *h_num_matched is the full count, and the call returns PFACX_STATUS_OUTPUT_TRUNCATED.
 *   Duplicate lines report under the highest id, as everywhere.  A caseless handle (PFACX_READ_NOCASE) matches the folded set over the folded input;
 *   THE CLASS IS TESTED ON THE CALLER'S ORIGINAL BYTES, which are never modified: a class with 'a' but without 'A' tells "a" from "A" around a match.
 *   CONSEQUENCES: an empty class (all zero) bounds everything -- ALL is then exactly the list of PFACX_matchAll*, the word list exactly the list of
 *   PFAC_matchFromDeviceReduce.  A full class leaves only occurrences with p == 0 and p + L == n.  The class "every byte but '\n'" is grep -x: the
 *   occurrence is a whole line, with or without a last newline.  The class "every byte but ',' and '\n'" gives whole CSV fields.
 *   PFACX_countPairsFromDevice(..., PFACX_COUNT_LONGEST) over the ids of the ALL list gives whole-word term frequencies.
 * PFACX_matchWordsFromDevice / ...FromHost: capacity = entries of each array, >= size (smaller: PFAC_STATUS_INVALID_PARAMETER): as in PFACX_matchAll*
 * the caller's arrays take the scan's unordered list before the result is written, so entries below `size` may be overwritten beyond the count.
 * size >= 2^31, an unknown flag bit, or a null pointer other than h_class: PFAC_STATUS_INVALID_PARAMETER.  No pattern set:
 * PFAC_STATUS_PATTERNS_NOT_READY.  size == 0: success, 0 pairs, nothing touched.  A device form on a host-only handle: PFAC_STATUS_LIB_NOT_EXIST.  All
 * three calls are synchronous (the count comes to the host) and take the handle's lock.  The device form runs on whatever kernel variant, walker, perf
 * mode and texture mode the handle selects.  The host form follows PFAC_setPlatform like PFACX_countFromHost: the CPU platforms, host-only handles
 * included, use the CPU matcher and a host loop over temporaries of 8 bytes per input byte; the GPU platform uses the pipelined pairs path and the
 * same loop.
 * PFACX_wordsPairsFromDevice: the same lists from a LONGEST list the caller already has -- the pairs of PFAC_matchFromDeviceReduce, or of
 * PFACX_matchBatchFromDeviceReduce, whose positions are relative to the buffer -- over the same d_input; it runs no second scan.  THE LIST MUST BE A
 * LONGEST LIST, one pair per position, ascending (the all-match list would report every chain again from each of its members).  The pair arrays are
 * DEVICE memory and the caller's contract, like the token arrays of PFACX_replaceFromDevice: an id outside [1, F] is ignored, a position outside
 * [0, size) too, a chain member whose [pos, pos + len) does not lie inside [0, size] is not kept, and nothing outside the buffers is ever read or
 * written.  `capacity` is free; with capacity == 0 the output arrays may be null: the count query.  Output arrays that overlap the input pair arrays:
 * PFAC_STATUS_INVALID_PARAMETER; numPairs >= 2^31 too.  numPairs == 0: success, 0 pairs.
 * OUT OF SCOPE: the pairs of streams and flow sets (negative positions, carried bytes that are no longer in the caller's buffer) and per-segment
 * boundaries of a batch -- the byte in front of a segment's first byte is its neighbour like any other; a caller who wants segment ends to bound puts a
 * byte outside W between the segments.
 * MEMORY of the device forms: grow-only handle scratch, deviceScratchBytes of PFACX_getInfo, freed by PFACX_trim.  Both: 8 (B + 1) bytes rounded up to
 * 256 with B = (P + 255) / 256 blocks for P longest pairs (never more than eight blocks per compute unit), and 4 (F + 1) bytes of pattern lengths
 * (shared with the batch calls); a set in which one pattern is a prefix of another also 8 (F + 1) bytes of {prefix, chain length} table (shared with
 * PFACX_matchAll* and PFACX_count*).  PFACX_matchWordsFromDevice: also the ordered pair list, exactly the pair scratch a PFACX_matchAll* call
 * over the same input allocates (8 bytes per pair the scan's ordering has room for).
 * COST: the compacted scan WITH its ordering launches, then two passes over the pairs that read at most 1 + chainLen input bytes per
 * pair and a one-block scan between them: the extra over PFACX_matchAll* follows the pairs, not the bytes. */
#define PFACX_WORDS_ALL 1u   /* every bounded occurrence instead of the longest one per position */
PFAC_status_t PFACX_matchWordsFromDevice(PFAC_handle_t handle, char *d_input, size_t size, const unsigned int *h_class /* 8 words or NULL */,
                                         unsigned int flags, int *d_ids, int *d_pos, size_t capacity, size_t *h_num_matched);
PFAC_status_t PFACX_matchWordsFromHost  (PFAC_handle_t handle, char *h_input, size_t size, const unsigned int *h_class /* 8 words or NULL */,
                                         unsigned int flags, int *h_ids, int *h_pos, size_t capacity, size_t *h_num_matched);
PFAC_status_t PFACX_wordsPairsFromDevice(PFAC_handle_t handle, const char *d_input, size_t size, const unsigned int *h_class /* 8 words or NULL */,
                                         unsigned int flags, const int *d_pairIds, const int *d_pairPos, size_t numPairs,
                                         int *d_ids, int *d_pos, size_t capacity, size_t *h_num_matched);

/* Pattern groups: each segment of a batch sees only its own patterns -- the fast-pattern set of a packet's port groups in an IDS, a tenant's keyword
 * list over that tenant's records, a per-language stop list per document -- with ONE compiled set and ONE scan over the whole batch.
 *   There are 64 GROUPS.  Pattern id has the mask M[id] = h_patternMasks[id] (numMasks >= F + 1 entries, entry 0 ignored; fewer:
 *   PFAC_STATUS_INVALID_PARAMETER); bit g set: the pattern is in group g.  PFACX_groupsOpen copies the table.  Duplicate pattern lines are one
 *   pattern, reported under the highest of their ids as everywhere; the mask of the reported id is the OR of the masks of ALL ids that name that
 *   pattern (the same string in two port groups, under two ids, belongs to both -- the resolution PFACX_rulesOpen does for ids), and the ids that
 *   are never reported end with mask 0.  A pattern whose mask is 0 is never reported by these calls.
 *   Segment k has the mask segMasks[k]; segMasks == NULL: every segment has all 64 bits set.  Pattern id is ENABLED in segment k if
 *   M[id] & segMasks[k] is non-zero.
 *   THE ALL-MATCH LIST of segment k is that of PFACX_matchAllBatchFromDevice: occurrences wholly inside the segment, positions relative to the
 *   buffer and ascending, within one position the longest pattern first.
 *   THE GROUP LIST, with PFACX_GROUPS_ALL: the all-match list of every segment without the pairs of patterns that are not enabled in that segment,
 *   the segments concatenated.  With flags 0: the first pair of each position of that list -- THE LONGEST ENABLED PATTERN at each position that has
 *   one.  That is not a filter over the longest pairs: where the longest pattern at a position belongs to another group, a proper prefix of it that
 *   is enabled is reported (`foo` in group 0, `foobar` in group 1, "foobar" in a segment of group 0: `foo`).
 *   CONSEQUENCES: all pattern masks and all segment masks ~0: ALL is exactly the list of PFACX_matchAllBatchFromDevice, flags 0 exactly the list of
 *   PFACX_matchBatchFromDeviceReduce.  A segment mask of 0 gives an empty segment.  A caseless handle (PFACX_READ_NOCASE) folds as in every other
 *   call.  No input byte is ever read by the pass behind the scan, and the caller's buffers are never modified.
 * segFirst (numSegments + 1 size_t, optional): entries [segFirst[k], segFirst[k + 1]) of the list are segment k's pairs; complete also under truncation.
 * segGroups (numSegments 64-bit words, optional): segGroups[k] = the OR of M[id] & segMasks[k] over ALL enabled occurrences of segment k, whatever
 * the flags and the capacity: "which groups have a hit in this segment", the prefilter answer an IDS asks for; available with capacity == 0; a
 * segment without a hit gets 0.
 * `capacity` (entries of each pair array) is free, as for the fired list of PFACX_rules*: the scan's pair list lives in the handle's pair scratch,
 * never in the caller's arrays.  A list longer than capacity: exactly its first `capacity` pairs are written and nothing at or behind `capacity`,
 * *h_num_matched is the full length, segFirst and segGroups are complete, and the call returns PFACX_STATUS_OUTPUT_TRUNCATED; with capacity == 0
 * the two pair arrays may be null: the count query.
 * Offsets follow the rules of PFACX_matchBatch*: host offsets are validated; device offsets and device segment masks are the caller's contract,
 * clamped and never checked (wrong offsets: a wrong list, never an access outside the buffers).  offsets == NULL with numSegments == 1: the whole
 * buffer is one segment -- the plain "subset of the set" call.
 * PFAC_STATUS_INVALID_PARAMETER: size >= 2^31, numSegments >= 2^31, an unknown flag bit, a required null pointer, offsets == NULL with numSegments
 * != 1, numSegments == 0 with size > 0, numMasks < F + 1.  No pattern set at open: PFAC_STATUS_PATTERNS_NOT_READY.  size == 0: success, 0 pairs,
 * segFirst and segGroups zeroed where given.  A device form on a host-only handle: PFAC_STATUS_LIB_NOT_EXIST; opening on one works.  After the
 * handle reads or loads another pattern set every match call returns PFAC_STATUS_INVALID_PARAMETER and only PFACX_groupsClose works.  PFAC_destroy
 * closes the handle's group tables, as it closes rule sets.  All calls are synchronous and take the handle's lock.  The device forms run on
 * whatever kernel variant, walker, perf mode and texture mode the handle selects; the host form follows PFAC_setPlatform like
 * PFACX_countBatchFromHost: the CPU platforms, host-only handles included, run on the CPU -- the longest pairs segment by segment, then their
 * prefix chains (temporaries: 8 bytes per input byte, 4 per segment) --, the GPU platform runs the pipelined path of PFACX_matchBatchFromHost and
 * the same loop.  A pattern set that another thread replaces during a host call: PFAC_STATUS_INVALID_PARAMETER, as after the call.
 * PFACX_groupsPairsFromDevice runs no scan: it takes a LONGEST list with the first pair of each segment -- d_matched_result, d_pos and d_segFirst of
 * PFACX_matchBatchFromDeviceReduce, or ids, pos and pieceFirst of a PFACX_flows* call, which PFACX_wordsPairsFromDevice cannot take: this pass
 * reads no input.  Positions are copied through as they are, negative ones included: that gives per-flow groups.  The arrays are DEVICE memory and
 * the caller's contract: an id outside [1, F] is ignored and never used as an index; every entry of d_segFirstPairs (numSegments + 1 ints; NULL
 * with numSegments == 1: one segment of all pairs) is clamped to [0, numPairs] and then raised to the largest entry in front of it, so a
 * decreasing pair is an empty segment; pairs before the first or behind the last bound belong to no segment.  Output arrays that overlap the
 * input pair arrays: PFAC_STATUS_INVALID_PARAMETER; numPairs >= 2^31 too.  numPairs == 0: success with zeros.
 * MEMORY of the device forms.  The mask table, 8 (F + 1) bytes made by the first device call, is state like a rule set's tables: counted under
 * deviceTableBytes, kept by PFACX_trim, freed by PFACX_groupsClose.  Grow-only handle scratch (deviceScratchBytes, freed by PFACX_trim): 8 (B + 1)
 * bytes rounded up to 256, B = one block per 256 longest pairs, eight per compute unit at most, and with a segment array 4 (numSegments + 1) bytes
 * rounded up to 256 for its bounds; PFACX_groupsMatchFromDevice also what the scan shares with PFACX_countBatchFromDevice (the pair list, the first
 * pair of each segment, the pattern lengths, the fix-up's scratch); a set in which a pattern is a prefix of another the {prefix, chain length}
 * table of PFACX_matchAll*.  Nothing is sized by segments x patterns.
 * COST: the ordered compacted batch scan, then two passes over the pairs that walk each pair's chain through two 8-byte tables and
 * a one-block scan between them: the extra over the scan follows the pairs and the segments, not the bytes.
 * OUT OF SCOPE: more than 64 groups; changing masks without close and reopen; a per-pair output of the groups that hit (the caller has M[id] &
 * segMasks[k]); groups inside PFACX_rules* or PFACX_countBatch* (feed their pairs forms); carried state across flows calls. */
typedef struct PFACX_groups_s *PFACX_groups_t;
#define PFACX_GROUPS_ALL 1u   /* every enabled occurrence instead of the longest enabled one per position */
PFAC_status_t PFACX_groupsOpen (PFAC_handle_t handle, const unsigned long long *h_patternMasks, size_t numMasks /* >= F + 1 */, PFACX_groups_t *groups);
PFAC_status_t PFACX_groupsClose(PFACX_groups_t groups);
PFAC_status_t PFACX_groupsMatchFromDevice(PFACX_groups_t groups, char *d_input, size_t size, const size_t *d_offsets, size_t numSegments,
                                          const unsigned long long *d_segMasks /* numSegments, may be NULL */, unsigned int flags,
                                          int *d_ids, int *d_pos, size_t capacity, size_t *d_segFirst /* numSegments + 1, may be NULL */,
                                          unsigned long long *d_segGroups /* numSegments, may be NULL */, size_t *h_num_matched);
PFAC_status_t PFACX_groupsMatchFromHost  (PFACX_groups_t groups, char *h_input, size_t size, const size_t *h_offsets, size_t numSegments,
                                          const unsigned long long *h_segMasks, unsigned int flags,
                                          int *h_ids, int *h_pos, size_t capacity, size_t *h_segFirst, unsigned long long *h_segGroups,
                                          size_t *h_num_matched);
PFAC_status_t PFACX_groupsPairsFromDevice(PFACX_groups_t groups, const int *d_pairIds, const int *d_pairPos, size_t numPairs,
                                          const int *d_segFirstPairs /* numSegments + 1; NULL with numSegments == 1 */, size_t numSegments,
                                          const unsigned long long *d_segMasks, unsigned int flags,
                                          int *d_ids, int *d_pos, size_t capacity, size_t *d_segFirst, unsigned long long *d_segGroups,
                                          size_t *h_num_matched);

/* Per-pattern case sensitivity over a caseless set: `nocase` as a property of each pattern, as in a Snort rule's `content:` -- `password` in any
 * case next to `AKIA` and `-----BEGIN` exact, `host: ` in any case next to `GET ` exact -- with ONE caseless handle and ONE scan.
 *   The pattern text has lines 1 .. F, ids as the reader assigns them.  Line i has the flag s_i = h_sensitive[i] != 0 (1: case-sensitive, 0: caseless;
 *   entry 0 ignored).  fold is the ASCII fold of PFACX_READ_NOCASE: 'A'-'Z' -> 'a'-'z', every other byte unchanged.
 *   OCCURRENCE: line i occurs at p iff p + len_i <= n and, s_i = 1: in[p, p + len_i) equals the line byte for byte; s_i = 0: the folded input bytes
 *   equal the folded line.
 *   SAME PATTERN: two lines whose flags are equal and whose bytes (s = 1) or folded bytes (s = 0) are equal.  They are reported once, under the
 *   highest of their ids: the duplicate rule of every reader.  A sensitive `GET`, a sensitive `get` and a caseless `Get` are three patterns.
 *   THE LIST (flags 0): one pair per position that has an occurrence, the longest occurring pattern, on equal length the highest id; positions
 *   ascend.  That is not a filter over the caseless longest pairs: where the longest candidate fails its exact compare, a proper prefix may pass.
 *   ALL (PFACX_CASE_ALL): every distinct occurring pattern, by position, then length descending, then id descending.
 *   Reported ids are line numbers: the handle's id space; they differ from the handle's only where the caseless handle collapsed several lines.
 * PFACX_caseOpen: the handle must hold a set read with PFACX_READ_NOCASE (else PFAC_STATUS_INVALID_PARAMETER).  `patterns` is the same text,
 * unfolded, readFlags the PFACX_READ_STRICT / PFACX_READ_STRIP_CR bits of that read (any other bit, PFACX_READ_NOCASE included: ignored).  The
 * text goes through the reader's own line splitter; a text whose folded lines are not the handle's set -- another F, or a folded line that differs
 * from the handle's pattern of that id -- and numFlags < F + 1 are PFAC_STATUS_INVALID_PARAMETER.  The text and the flags are copied.
 * *maxMatchesPerPosition (may be NULL): the largest number of ALL pairs one position can have.  The object belongs to the handle like a group
 * table: PFAC_destroy closes it, and after the handle reads or loads another set every match call returns PFAC_STATUS_INVALID_PARAMETER and only
 * PFACX_caseClose works.  Opening on a host-only handle works.
 * PFACX_caseMatchFromDevice: capacity = entries of each array, >= size (smaller: PFAC_STATUS_INVALID_PARAMETER): as in PFACX_matchWordsFromDevice
 * the caller's arrays take the scan's unordered list before the result is written.  PFACX_caseMatchFromHost and PFACX_casePairsFromDevice:
 * `capacity` is free, with capacity == 0 the output arrays may be null: the count query.  A list longer than capacity: its first `capacity` pairs
 * are written, nothing at or behind `capacity`, *h_num_matched is the full length, and the call returns PFACX_STATUS_OUTPUT_TRUNCATED.
 * size >= 2^31, an unknown flag bit, a required null pointer: PFAC_STATUS_INVALID_PARAMETER.  size == 0: success, 0 pairs, nothing touched.  A
 * device form on a host-only handle: PFAC_STATUS_LIB_NOT_EXIST.  All calls are synchronous and take the handle's lock.  The input is never
 * modified.  The host form follows PFAC_setPlatform like PFACX_matchWordsFromHost (temporaries: 8 bytes per input byte).
 * PFACX_casePairsFromDevice: the same lists from an ordered LONGEST list of the caseless handle over the same d_input (the pairs of
 * PFAC_matchFromDeviceReduce); it runs no scan and reads the caller's unfolded bytes.  The pair arrays are the caller's contract: an id outside
 * [1, F] or a position outside [0, size) is a pair that gives nothing, a member that does not fit the input is not kept, an unsorted list gets
 * unspecified values, and nothing outside the buffers is ever read or written.  Output arrays that overlap the pair arrays, numPairs >= 2^31:
 * PFAC_STATUS_INVALID_PARAMETER.  numPairs == 0: success, 0 pairs.
 * MEMORY.  The tables, made by the first device call, are state of the object (deviceTableBytes, kept by PFACX_trim, freed by PFACX_caseClose):
 * 8 bytes per distinct pattern, 4 (F + 2) bytes, and the bytes of the sensitive patterns, each padded to a multiple of 4.  Grow-only handle
 * scratch: 8 (B + 1) bytes rounded up to 256, B = one block per 256 longest pairs, eight per compute unit at most; the pattern lengths and the
 * {prefix, chain length} table shared with PFACX_matchWords*; PFACX_caseMatchFromDevice also the pair scratch of PFACX_matchAll*.
 * COST: the caseless compacted scan with its ordering launches, then two passes over the pairs that compare the bytes of the
 * sensitive candidates, four at a time; a thread per pair, so long sensitive patterns make lanes uneven.
 * OUT OF SCOPE: the pairs of streams and flow sets; a full-result-vector form; segment bounds of a batch; non-ASCII folds; a read flag or a
 * compiled-file form of the flags. */
typedef struct PFACX_case_s *PFACX_case_t;
#define PFACX_CASE_ALL 1u   /* every distinct occurring pattern instead of the longest one per position */
PFAC_status_t PFACX_caseOpen (PFAC_handle_t handle, const char *patterns, size_t size, unsigned int readFlags,
                              const unsigned char *h_sensitive, size_t numFlags /* >= F + 1, indexed by ID */,
                              PFACX_case_t *cs, int *maxMatchesPerPosition /* may be NULL */);
PFAC_status_t PFACX_caseClose(PFACX_case_t cs);
PFAC_status_t PFACX_caseMatchFromDevice(PFACX_case_t cs, char *d_input, size_t size, unsigned int flags,
                                        int *d_ids, int *d_pos, size_t capacity, size_t *h_num_matched);
PFAC_status_t PFACX_caseMatchFromHost  (PFACX_case_t cs, char *h_input, size_t size, unsigned int flags,
                                        int *h_ids, int *h_pos, size_t capacity, size_t *h_num_matched);
PFAC_status_t PFACX_casePairsFromDevice(PFACX_case_t cs, const char *d_input, size_t size, unsigned int flags,
                                        const int *d_pairIds, const int *d_pairPos, size_t numPairs,
                                        int *d_ids, int *d_pos, size_t capacity, size_t *h_num_matched);

/* Masked byte signatures with wildcards: binary signatures of the ClamAV kind -- `4D 5A ?? ?? 50 45 00 00`, `E8 ?? ?? ?? ?? 5? C3` -- and text
 * rules such as `id=`, any 4 bytes, `;`.  The library picks one fully specified run of each signature as its ANCHOR, loads the distinct anchors as
 * the handle's pattern set, scans for them with the product kernels and verifies every signature of every anchor occurrence against the input.
 *   SIGNATURES.  S signatures, ids 1 .. S in the order given.  Signature i has len_i >= 1 byte pairs (v, m); the library canonicalises v &= m.
 *   OCCURRENCE: signature i occurs at start s iff 0 <= s, s + len_i <= n and (in[s + k] ^ v_k) & m_k == 0 for every k.  Every signature is its
 *   own entry: two identical signatures are both reported.
 *   ANCHOR.  A candidate is a run of bytes with mask 0xFF and a value other than 0x0A (the pattern reader splits lines at 0x0A, so that byte is
 *   never part of an anchor: it is verified like a wildcard byte).  The anchor is the longest such run, the leftmost of equal ones, cut to its first
 *   maxAnchorLen bytes; maxAnchorLen == 0 stands for 32.  A signature without such a byte is refused.  The rule is documented, but
 *   callers rely on PFACX_sigGetAnchors.
 *   THE LIST: every occurrence as (id, start), ordered by ANCHOR POSITION start + anchorOff[id] ascending; at one anchor position the longer
 *   anchor first; within one anchor ids descend -- pair order, chain order, id order: the project's convention.  It is NOT sorted by start.
 * PFACX_sigOpen: the signatures in CSR form in host memory -- h_values / h_masks[h_sigOff[i - 1], h_sigOff[i]) are signature i, h_sigOff has
 * numSigs + 1 entries --, copied.  It loads the distinct anchors into the handle exactly as PFACX_readPatternFromMemory would: the handle's set is
 * REPLACED (objects opened on the earlier set go stale as after any read), the handle becomes case-sensitive, and handle id q is the q-th distinct
 * anchor in order of first appearance.  PFAC_STATUS_INVALID_PARAMETER, with the handle's set untouched: a required null pointer, numSigs == 0 or
 * >= 2^31 - 1, and -- with the signature's id in *badSig (may be NULL; else 0) -- an h_sigOff that does not ascend (an empty signature), a
 * signature longer than 65 535 bytes, a signature without a fully specified byte other than 0x0A; also signatures of more than 2^32 bytes in all.
 * PFACX_sigOpenText: a parser in front of PFACX_sigOpen and nothing else.  One signature per '\n'-terminated line: hex digit pairs in either
 * letter case, a byte may be `??`, `x?` or `?x`; blanks and tabs between pairs are ignored, and so is a '\r' in front of the '\n'.  Refused with
 * PFAC_STATUS_INVALID_PARAMETER and the 1-based line in *badLine (may be NULL): an empty line, a digit without its partner, any other character,
 * bytes behind the last '\n' (as under PFACX_READ_STRICT), and a line the binary form refuses.  A text without any line: *badLine = 0.
 * PFACX_sigGetAnchors: by signature id (n >= S + 1 entries each, entry 0 is 0; smaller: PFAC_STATUS_INVALID_PARAMETER; an array may be NULL) the
 * handle's pattern id of the anchor, the anchor's offset inside the signature and its length.
 * The object belongs to the handle like a case object: PFAC_destroy closes it, and after the handle reads or loads another set every call on it
 * returns PFAC_STATUS_INVALID_PARAMETER and only PFACX_sigClose works.  Opening on a host-only handle works.
 * PFACX_sigMatchFromDevice: capacity = entries of each array, >= size (smaller: PFAC_STATUS_INVALID_PARAMETER): as in PFACX_caseMatchFromDevice
 * the caller's arrays take the scan's unordered list before the result is written.  PFACX_sigMatchFromHost and PFACX_sigPairsFromDevice:
 * `capacity` is free, with capacity == 0 the output arrays may be null: the count query.  A list longer than capacity: its first `capacity`
 * entries are written, nothing at or behind `capacity`, *h_num_matched is the full length, and the call returns PFACX_STATUS_OUTPUT_TRUNCATED.
 * size >= 2^31, a required null pointer: PFAC_STATUS_INVALID_PARAMETER.  size == 0: success, 0 entries, nothing touched.  A device form on a
 * host-only handle: PFAC_STATUS_LIB_NOT_EXIST.  All calls are synchronous and take the handle's lock.  The input is never modified.  The host
 * form follows PFAC_setPlatform like PFACX_caseMatchFromHost (temporaries: 8 bytes per input byte).
 * PFACX_sigPairsFromDevice: the same list from an ordered LONGEST list of the handle over the same d_input (the pairs PFAC_matchFromDeviceReduce
 * leaves); it runs no scan.  The pair arrays are the caller's contract: an id outside [1, F] or a position outside [0, size) is a pair that
 * gives nothing, an unsorted list gets unspecified values, and nothing outside the buffers is ever read or written.  Output arrays that overlap
 * the pair arrays, numPairs >= 2^31: PFAC_STATUS_INVALID_PARAMETER.  numPairs == 0: success, 0 entries.
 * MEMORY.  The tables, made by the first device call, are state of the object (deviceTableBytes, kept by PFACX_trim, freed by PFACX_sigClose):
 * 16 bytes per signature, 4 (F + 2) bytes, and twice the bytes of each signature padded to a multiple of 4.  Grow-only handle scratch: 8 (B + 1)
 * bytes rounded up to 256, B = one block per 256 longest pairs, eight per compute unit at most; the {prefix, chain length} table shared with
 * PFACX_matchWords*; PFACX_sigMatchFromDevice also the pair scratch of PFACX_matchAll*.
 * COST: the compacted scan over the anchors with its ordering launches, then two passes over the pairs that compare the masked
 * bytes of the candidates, four at a time; a thread per pair, so long signatures and large classes make lanes uneven.
 * OUT OF SCOPE (bounded gaps between parts: PFACX_gapsig* below): alternatives and negated bytes; caseless signatures; segment bounds of a batch; the pairs of
 * streams and flow sets; a full-result-vector form; a list sorted by start; a compiled-file form. */
typedef struct PFACX_sig_s *PFACX_sig_t;
PFAC_status_t PFACX_sigOpen    (PFAC_handle_t handle, const unsigned char *h_values, const unsigned char *h_masks,
                                const size_t *h_sigOff /* numSigs + 1 */, size_t numSigs, size_t maxAnchorLen /* 0: 32 */,
                                PFACX_sig_t *sig, int *badSig /* may be NULL */);
PFAC_status_t PFACX_sigOpenText(PFAC_handle_t handle, const char *text, size_t size, size_t maxAnchorLen /* 0: 32 */,
                                PFACX_sig_t *sig, int *badLine /* may be NULL */);
PFAC_status_t PFACX_sigGetAnchors(PFACX_sig_t sig, int *h_anchorId, int *h_anchorOff, int *h_anchorLen, size_t n /* >= S + 1, indexed by ID */);
PFAC_status_t PFACX_sigClose(PFACX_sig_t sig);
PFAC_status_t PFACX_sigMatchFromDevice(PFACX_sig_t sig, char *d_input, size_t size,
                                       int *d_ids, int *d_pos, size_t capacity, size_t *h_num_matched);
PFAC_status_t PFACX_sigMatchFromHost  (PFACX_sig_t sig, char *h_input, size_t size,
                                       int *h_ids, int *h_pos, size_t capacity, size_t *h_num_matched);
PFAC_status_t PFACX_sigPairsFromDevice(PFACX_sig_t sig, const char *d_input, size_t size,
                                       const int *d_pairIds, const int *d_pairPos, size_t numPairs,
                                       int *d_ids, int *d_pos, size_t capacity, size_t *h_num_matched);

/* Patterns matched within k mismatches: DNA reads against a panel of probes or primers, keyword lists over OCR output or typed text, known byte
 * sequences that have been patched in a few places.  The library cuts each pattern into k + 1 disjoint parts -- at any occurrence within k
 * substitutions at least one part is exact: the pigeonhole cut --, loads the distinct PIECES (the heads of the parts) as the handle's pattern set,
 * scans for them with the product kernels and counts the differing bytes of every pattern of every piece occurrence against the input.
 *   PATTERNS.  S patterns, ids 1 .. S in the order given, byte strings of L_i >= 1 bytes; h_budget[i - 1] = k_i, the number of bytes of pattern i
 *   that may differ, 0 .. PFACX_APPROX_MAX_MISMATCHES.  Every pattern is its own entry: two identical patterns are both reported.
 *   OCCURRENCE: pattern i occurs at start s with distance d iff 0 <= s, s + L_i <= n, d = #{t : in[s + t] != pat_i[t]} and d <= k_i.
 *   Substitutions only: no insertions, no deletions.
 *   PIECES.  Part j (j = 0 .. k) of a pattern of L bytes is [j L / (k + 1), (j + 1) L / (k + 1)), rounded down; its piece is the first
 *   min(part length, maxPieceLen) bytes of the part.  maxPieceLen == 0 stands for 32 and minPieceLen == 0 for 4: both defaults are suppositions
 *   carried over from the anchor default of PFACX_sigOpen, not measured.  A pattern shorter than (k + 1) minPieceLen is refused: its pieces would
 *   be candidates too often.  The pattern reader splits lines at 0x0A, so a piece that holds that byte is refused; a 0x0A outside every piece is
 *   compared like any other byte.  The rule is documented, but callers rely on PFACX_approxGetPieces.
 *   EACH OCCURRENCE ONCE.  An occurrence is found once per exact piece; it is reported by its LOWEST EXACT PIECE j*, the smallest j whose piece
 *   bytes equal in[s + partStart_j ...].
 *   THE LIST: every occurrence as (id, start) with its distance in a third array, ordered by CANDIDATE POSITION start + partStart_{j*} ascending;
 *   at one candidate position the longer piece first; within one piece string by pattern id descending, then by piece index descending -- pair
 *   order, chain order, table order: the project's convention.  It is NOT sorted by start.  It may be longer than size: several patterns can
 *   start at one position.
 * PFACX_approxOpen: the patterns in CSR form in host memory -- h_bytes[h_patOff[i - 1], h_patOff[i]) is pattern i, h_patOff has numPatterns + 1
 * entries, h_budget numPatterns --, copied.  It loads the distinct pieces into the handle exactly as PFACX_readPatternFromMemory would: the
 * handle's set is REPLACED (objects opened on the earlier set go stale as after any read), the handle becomes case-sensitive, and handle id q is
 * the q-th distinct piece in order of first appearance (pattern by pattern, piece by piece).  It checks under the handle's lock that the set it
 * adopts is the one it loaded.  PFAC_STATUS_INVALID_PARAMETER, with the handle's set untouched: a required null pointer, numPatterns == 0 or
 * >= 2^31 - 1, and -- with the pattern's id in *badPattern (may be NULL; else 0) -- an h_patOff that does not ascend (an empty pattern), a
 * pattern longer than 65 535 bytes, a budget outside [0, 7], L < (k + 1) minPieceLen, a piece that holds 0x0A (the first of these by pattern id);
 * also patterns of more than 2^32 bytes in all.
 * PFACX_approxGetPieces: h_pieceOff, numPatterns + 2 entries in CSR form BY ID (h_pieceOff[0] = h_pieceOff[1] = 0; the pieces of pattern i are
 * h_pieceOff[i] .. h_pieceOff[i + 1], piece j of it at h_pieceOff[i] + j; h_pieceOff[numPatterns + 1] = the number of pieces, the sum of
 * k_i + 1), and per piece the handle's pattern id of its string, its start inside the pattern and its length, n entries each.  Any array may be
 * NULL; n smaller than the number of pieces with one of the three per-piece arrays given: PFAC_STATUS_INVALID_PARAMETER, nothing written; with
 * all three NULL n is not looked at (h_pieceOff alone says how many there are).
 * The object belongs to the handle like a signature object: PFAC_destroy closes it, and after the handle reads or loads another set every call
 * on it returns PFAC_STATUS_INVALID_PARAMETER and only PFACX_approxClose works.  Opening on a host-only handle works.
 * PFACX_approxMatchFromDevice: capacity = entries of each array, >= size (smaller: PFAC_STATUS_INVALID_PARAMETER): as in
 * PFACX_sigMatchFromDevice d_ids and d_pos take the scan's unordered list before the result is written.  d_mis (may be NULL in every form) is
 * only ever written below min(the list, capacity).  PFACX_approxMatchFromHost and PFACX_approxPairsFromDevice: `capacity` is free, with
 * capacity == 0 the output arrays may be null: the count query.  A list longer than capacity: its first `capacity` entries are written, nothing
 * at or behind `capacity`, *h_num_matched is the full length, and the call returns PFACX_STATUS_OUTPUT_TRUNCATED.  size >= 2^31, a required null
 * pointer: PFAC_STATUS_INVALID_PARAMETER.  size == 0: success, 0 entries, nothing touched.  A device form on a host-only handle:
 * PFAC_STATUS_LIB_NOT_EXIST.  All calls are synchronous and take the handle's lock.  The input is never modified.  The host form follows
 * PFAC_setPlatform like PFACX_sigMatchFromHost (temporaries: 8 bytes per input byte).
 * PFACX_approxPairsFromDevice: the same list from an ordered LONGEST list of the handle over the same d_input (the pairs
 * PFAC_matchFromDeviceReduce leaves); it runs no scan.  The pair arrays are the caller's contract: an id outside [1, F] or a position outside
 * [0, size) is a pair that gives nothing, an unsorted list gets unspecified values, and nothing outside the buffers is ever read or written.
 * Output arrays (d_mis included) that overlap the pair arrays, numPairs >= 2^31: PFAC_STATUS_INVALID_PARAMETER.  numPairs == 0: success, 0 entries.
 * MEMORY.  The tables, made by the first device call, are state of the object (deviceTableBytes, kept by PFACX_trim, freed by
 * PFACX_approxClose): 16 bytes per piece, 4 (F + 2) bytes, and the bytes of each pattern padded to a multiple of 4.  Grow-only handle scratch:
 * 8 (B + 1) bytes rounded up to 256, B = one block per 256 longest pairs, eight per compute unit at most; the {prefix, chain length} table shared
 * with PFACX_matchWords*; PFACX_approxMatchFromDevice also the pair scratch of PFACX_matchAll*.
 * COST: the compacted scan over the pieces with its ordering launches, then two passes over the pairs that count the differing
 * bytes of the candidates, four at a time, and give up every 16 bytes where the budget is spent; a thread per pair, so long patterns and large
 * classes make lanes uneven, and short pieces over a small alphabet (4-byte pieces over ACGT: a false candidate per piece at 1 position in 256)
 * make candidates frequent: this costs more than signatures do.
 * OUT OF SCOPE: insertions and deletions; caseless or masked approximate patterns; pieces chosen by rarity; segment bounds of a batch; the pairs
 * of streams and flow sets; a list sorted by start; a full-result-vector form; a compiled-file form; a wave per long pattern. */
#define PFACX_APPROX_MAX_MISMATCHES 7
typedef struct PFACX_approx_s *PFACX_approx_t;
PFAC_status_t PFACX_approxOpen(PFAC_handle_t handle, const unsigned char *h_bytes, const size_t *h_patOff /* numPatterns + 1 */,
                               const int *h_budget /* numPatterns */, size_t numPatterns, size_t minPieceLen /* 0: 4 */,
                               size_t maxPieceLen /* 0: 32 */, PFACX_approx_t *approx, int *badPattern /* may be NULL */);
PFAC_status_t PFACX_approxGetPieces(PFACX_approx_t approx, size_t *h_pieceOff /* numPatterns + 2, CSR by ID */, int *h_pieceId, int *h_pieceStart,
                                    int *h_pieceLen, size_t n /* >= the number of pieces */);
PFAC_status_t PFACX_approxClose(PFACX_approx_t approx);
PFAC_status_t PFACX_approxMatchFromDevice(PFACX_approx_t approx, char *d_input, size_t size,
                                          int *d_ids, int *d_pos, int *d_mis /* may be NULL */, size_t capacity, size_t *h_num_matched);
PFAC_status_t PFACX_approxMatchFromHost  (PFACX_approx_t approx, char *h_input, size_t size,
                                          int *h_ids, int *h_pos, int *h_mis /* may be NULL */, size_t capacity, size_t *h_num_matched);
PFAC_status_t PFACX_approxPairsFromDevice(PFACX_approx_t approx, const char *d_input, size_t size,
                                          const int *d_pairIds, const int *d_pairPos, size_t numPairs,
                                          int *d_ids, int *d_pos, int *d_mis /* may be NULL */, size_t capacity, size_t *h_num_matched);

/* Signatures with bounded gaps between parts: the variable-length signatures of the ClamAV / YARA kind -- `4D 5A {2-6} 50 45 00 00`,
 * `E8 ?? ?? ?? ?? [0-8] 5? C3`.  As for PFACX_sig* the library picks one fully specified run of each signature as its ANCHOR, loads the distinct
 * anchors as the handle's pattern set, scans for them with the product kernels and verifies every signature of every anchor occurrence against
 * the input; here the verification searches over the gap widths.
 *   SIGNATURES.  S signatures, ids 1 .. S in the order given.  Signature i is a sequence of m_i parts, 1 <= m_i <= 64; a part is a string of 1 ..
 *   65 535 byte pairs (v, m) as in PFACX_sig*, canonicalised v &= m; between part j and part j + 1 stands a gap [lo_j, hi_j], 0 <= lo_j <= hi_j
 *   <= 65 535.  The SLACK, the sum of hi_j - lo_j, is at most PFACX_GAPSIG_MAX_SLACK = 63: where a part can lie relative to any other then fits
 *   one 64-bit mask.  The span, the sum of the lengths and of the hi_j, stays below 2^31 - 1 (the other limits keep it below 2^23).
 *   EMBEDDING of signature i at start s in n bytes: offsets o_0 = s, o_{j+1} = o_j + len_j + g_j with lo_j <= g_j <= hi_j, 0 <= s,
 *   o_{m-1} + len_{m-1} <= n, and (in[o_j + k] ^ v_{j,k}) & m_{j,k} == 0 for every part j and byte k.  OCCURRENCE: signature i occurs at s iff an
 *   embedding at s exists.  THE LIST holds one entry (id, start, end) per (id, start) that occurs; end is the SMALLEST o_{m-1} + len_{m-1} over
 *   all embeddings at s -- a minimum over all gap choices, not what a lazy left-to-right choice finds.  Every signature is its own entry: two
 *   identical signatures are both reported.  A signature of one part gives the entries PFACX_sig* gives for it, with end = start + len.
 *   ANCHOR.  The rule of PFACX_sigOpen over all parts: a candidate is a run of bytes with mask 0xFF and a value other than 0x0A inside ONE part (a
 *   run never crosses a part boundary, not even over a gap {0}); the anchor is the longest run, of equal ones the one in the lowest part, then
 *   the leftmost, cut to its first maxAnchorLen bytes; 0 stands for 32 (the unmeasured supposition of PFACX_sigOpen).  A signature without such
 *   a byte is refused.  Callers rely on PFACX_gapsigGetAnchors.
 *   EACH OCCURRENCE ONCE.  The anchor part a may lie at several offsets for one start.  (id, s) is listed by the occurrence of part a at the
 *   SMALLEST offset x that lies on some embedding at s -- not the smallest x that the parts in front of a reach: an x whose tail cannot be
 *   completed owns nothing.
 *   ORDER: by the owning anchor occurrence, x + anchorOff ascending; at one position the longer anchor first; within one anchor ids descend;
 *   within one (anchor occurrence, signature) starts ascend.  It is NOT sorted by start.
 * PFACX_gapsigOpen: CSR form in host memory, copied -- h_values / h_masks[h_partOff[j], h_partOff[j + 1]) are part j, the parts of signature i are
 * h_sigPart[i - 1] .. h_sigPart[i] - 1, h_gapLo[j] / h_gapHi[j] the gap BEHIND part j (the entry of a signature's last part is not read).  It
 * loads the distinct anchors exactly as PFACX_sigOpen does: the handle's set is REPLACED, the handle becomes case-sensitive, handle id q is the
 * q-th distinct anchor in order of first appearance, and it checks under the handle's lock that the set it adopts is the one it loaded.
 * PFAC_STATUS_INVALID_PARAMETER, with the handle's set untouched: a required null pointer (all six arrays), numSigs == 0 or >= 2^31 - 1, and --
 * with the id of the FIRST such signature in *badSig (may be NULL; else 0) -- no part or more than 64, an empty part or one longer than 65 535
 * bytes, lo > hi or hi > 65 535, a slack above 63, a span of 2^31 - 1 or more; behind those, by id, a signature without a fully specified
 * byte other than 0x0A.
 * PFACX_gapsigOpenText: a parser in front of it and nothing else: the grammar of PFACX_sigOpenText plus gap tokens between byte pairs: `{n}`,
 * `{n-m}`, `{-m}` (0 .. m), and the same in brackets, `[n]`, `[n-m]`, `[-m]`; decimal, no blanks inside.  `??` bytes stay inside their part.
 * Refused with the 1-based line in *badLine: all PFACX_sigOpenText refuses, a gap at the start or the end of a line, two gaps in a row, n > m, an
 * unbounded gap (`*`, `{n-}`), an empty or unclosed token, a number above 65 535, and a line the binary form refuses.
 * PFACX_gapsigGetAnchors: by signature id (n >= S + 1 entries each, entry 0 is 0; an array may be NULL) the handle's pattern id of the anchor,
 * the part that holds it, its offset inside that part and its length.
 * The object belongs to the handle like a signature object (PFAC_destroy closes it; stale after another read; host-only handles can open).
 * The three match calls are those of PFACX_approx* word for word, with d_end (may be NULL in every form; only ever written below min(the list,
 * capacity)) in the place of d_mis: the device form needs capacity >= size and its arrays take the scan's unordered list first; the host and
 * pairs forms take any capacity, 0 with null arrays is the count query; a longer list: the first `capacity` entries, the full length, and
 * PFACX_STATUS_OUTPUT_TRUNCATED; size >= 2^31 or a required null pointer: PFAC_STATUS_INVALID_PARAMETER; size == 0: success, nothing touched;
 * a device form on a host-only handle: PFAC_STATUS_LIB_NOT_EXIST; the pairs form ignores ids outside [1, F] and positions outside [0, size),
 * refuses output arrays (d_end included) that overlap the pair arrays and numPairs >= 2^31, and owns an occurrence only through pairs of its
 * list.  All calls are synchronous and take the handle's lock.  The input is never modified, and nothing outside it is read.
 * MEMORY.  The tables, made by the first device call, are state of the object (deviceTableBytes, kept by PFACX_trim, freed by
 * PFACX_gapsigClose): 16 bytes per signature, 16 per part, 4 (F + 2) bytes, and twice the bytes of each part padded to a multiple of 4.
 * Grow-only handle scratch as for PFACX_sig*.
 * COST: the compacted scan over the anchors with its ordering launches, then two passes over the pairs; a thread per pair runs the
 * whole search of a candidate -- up to 64 starts, each up to parts x 64 masked compares, most of which end in their first dword.
 * OUT OF SCOPE: unbounded gaps and slack above 63; alternatives and negated bytes; caseless parts; anchors chosen by rarity; a wave per long
 * search; segment bounds, stream and flow pairs; a full-result-vector form; a list sorted by start. */
#define PFACX_GAPSIG_MAX_SLACK 63
typedef struct PFACX_gapsig_s *PFACX_gapsig_t;
PFAC_status_t PFACX_gapsigOpen(PFAC_handle_t handle, const unsigned char *h_values, const unsigned char *h_masks,
                               const size_t *h_partOff /* numParts + 1: bytes */, const size_t *h_sigPart /* numSigs + 1: parts */,
                               const unsigned int *h_gapLo, const unsigned int *h_gapHi /* numParts each; entry of a signature's last part ignored */,
                               size_t numSigs, size_t maxAnchorLen /* 0: 32 */, PFACX_gapsig_t *sig, int *badSig /* may be NULL */);
PFAC_status_t PFACX_gapsigOpenText(PFAC_handle_t handle, const char *text, size_t size, size_t maxAnchorLen /* 0: 32 */,
                                   PFACX_gapsig_t *sig, int *badLine /* may be NULL */);
PFAC_status_t PFACX_gapsigGetAnchors(PFACX_gapsig_t sig, int *h_anchorId, int *h_anchorPart, int *h_anchorOff /* inside that part */,
                                     int *h_anchorLen, size_t n /* >= S + 1, indexed by ID */);
PFAC_status_t PFACX_gapsigClose(PFACX_gapsig_t sig);
PFAC_status_t PFACX_gapsigMatchFromDevice(PFACX_gapsig_t sig, char *d_input, size_t size,
                                          int *d_ids, int *d_pos, int *d_end /* may be NULL */, size_t capacity, size_t *h_num_matched);
PFAC_status_t PFACX_gapsigMatchFromHost  (PFACX_gapsig_t sig, char *h_input, size_t size,
                                          int *h_ids, int *h_pos, int *h_end /* may be NULL */, size_t capacity, size_t *h_num_matched);
PFAC_status_t PFACX_gapsigPairsFromDevice(PFACX_gapsig_t sig, const char *d_input, size_t size,
                                          const int *d_pairIds, const int *d_pairPos, size_t numPairs,
                                          int *d_ids, int *d_pos, int *d_end /* may be NULL */, size_t capacity, size_t *h_num_matched);

/* Patterns matched within k EDITS, insertions and deletions included: a typed keyword (`pasword`, `passsword`), OCR output that drops or doubles
 * a letter, a DNA read with an indel, a byte sequence with an instruction inserted -- what PFACX_approx* leaves out of scope.  The pigeonhole cut
 * carries over: an alignment with at most k edits over k + 1 disjoint parts leaves one part untouched, so its piece is exact somewhere in the
 * input.  The exact piece fixes only a diagonal, not a start, so every candidate is verified by a banded dynamic program.
 *   PATTERNS.  S byte strings, ids 1 .. S in the order given, L_i bytes; h_budget[i - 1] = k_i, the number of edits, 0 .. PFACX_EDIT_MAX_EDITS.
 *   An edit is a substituted, an inserted or a deleted byte, each at cost 1 (Levenshtein).  Identical patterns are both reported.
 *   DISTANCE AT AN END.  For an end e, 0 <= e <= n ("the match ends in front of in[e]"), D_i(e) = min over 0 <= s <= e of ed(pat_i, in[s, e)):
 *   Sellers' recurrence C[0][c] = 0, C[r][0] = r, C[r][c] = min(C[r-1][c-1] + (pat[r-1] != in[c-1]), C[r-1][c] + 1, C[r][c-1] + 1),
 *   D(e) = C[L][e].  Nothing outside [0, n) exists: a start in front of 0 or an end behind n is no occurrence.
 *   OCCURRENCE AND ENTRY.  Pattern i occurs at end e iff D_i(e) <= k_i.  The entry is (id, start, end, distance): distance = D_i(e), start = the
 *   LARGEST s with ed(pat_i, in[s, e)) = D_i(e), the shortest best match.  L > k is enforced, so start < end always.
 *   WHICH ENDS.  flags 0: every end that occurs, the textbook output -- an exact copy with k = 2 gives five entries.  PFACX_EDIT_BEST_ENDS (a
 *   flag of the open call): only the ends with all three of D(e) <= k, D(e - 1) > D(e), and e == n or D(e + 1) >= D(e).  This is a three-point
 *   rule on D and nothing else; it is not a plateau analysis.
 *   PIECES.  The cut is that of PFACX_approxOpen, word for word: part j is [j L / (k + 1), (j + 1) L / (k + 1)), its piece the first
 *   min(part length, maxPieceLen) bytes of the part; the defaults are 4 and 32.  Refused with the id in *badPattern and the handle's set
 *   untouched: L < (k + 1) minPieceLen, a piece that holds 0x0A, L > 65 535, k > 7, an empty pattern.  The distinct pieces are loaded as the
 *   handle's set, which is REPLACED; the handle becomes case-sensitive, and handle id q is the q-th distinct piece.  PFACX_editGetPieces has the
 *   signature and the meaning of PFACX_approxGetPieces.
 *   CANDIDATES AND OWNERSHIP.  A candidate is (piece j of pattern i exact at input position p).  With o the start of the piece in the pattern
 *   it has the diagonal d0 = p - o and COVERS the ends e with |e - L - d0| <= k, clipped to [0, n].  Every occurrence (i, e) is covered by at
 *   least one candidate: the untouched part of a best alignment.  EACH OCCURRENCE ONCE: (i, e) is listed by the covering candidate with the
 *   smallest j, and of those the smallest p.  The test reads the input, not the pair list: (i, e) is dropped on behalf of (j, p) where some
 *   piece j' < j of the pattern is exact at a p' in [e - L + o_j' - k, e - L + o_j' + k] with the piece inside [0, n), or piece j itself at a
 *   p' in [e - L + o_j - k, p - 1].  The pairs form therefore owns an occurrence only through pairs of its list.
 *   THE LIST: by owning candidate position p ascending; at one position the longer piece first; within one piece string pattern ids
 *   descending, then piece indices descending; within one (candidate, entry) ends ascending -- pair order, chain order, table order.  It is
 *   NOT sorted by start or end, and it may be longer than size.
 * PFACX_editOpen: the arguments of PFACX_approxOpen and `flags`: 0 or PFACX_EDIT_BEST_ENDS; any other bit: PFAC_STATUS_INVALID_PARAMETER.
 * PFACX_editMatchFromDevice / FromHost / PFACX_editPairsFromDevice: d_pos takes the start; d_end and d_dist each stand where d_mis stands in
 * PFACX_approx*: each may be NULL in every form, and each is only ever written below min(the list, capacity).  Everything else is that of
 * PFACX_approx*, word for word: capacity and truncation (PFACX_STATUS_OUTPUT_TRUNCATED, the full length in *h_num_matched), the device form's
 * capacity >= size, the 2^31 limits, size == 0, host-only handles, locking, staleness after another read, the refusal of output arrays (all
 * four) that overlap the pair arrays, pairs with ids or positions that give nothing, deviceTableBytes / PFACX_trim / close.
 * MEMORY: as PFACX_approx* (16 bytes per piece, 4 (F + 2) bytes, the patterns' bytes padded to dwords; scratch 8 (B + 1) bytes rounded to 256).
 * COST: a thread per pair runs L x (4 k + 3) dependent cell updates for a candidate that holds, in both passes; a candidate that
 * is far off ends at the first test of the early exit (every 4 rows).  This is far more than the compare of PFACX_approx*.
 * OUT OF SCOPE: weighted edits and transpositions; caseless or masked patterns; pieces chosen by rarity; segment bounds, stream and flow pairs;
 * a full-result-vector form; a list sorted by end; a compiled-file form; budgets above 7. */
#define PFACX_EDIT_MAX_EDITS 7
#define PFACX_EDIT_BEST_ENDS 1u
typedef struct PFACX_edit_s *PFACX_edit_t;
PFAC_status_t PFACX_editOpen(PFAC_handle_t handle, const unsigned char *h_bytes, const size_t *h_patOff /* numPatterns + 1 */,
                             const int *h_budget /* numPatterns */, size_t numPatterns, size_t minPieceLen /* 0: 4 */,
                             size_t maxPieceLen /* 0: 32 */, unsigned int flags, PFACX_edit_t *edit, int *badPattern /* may be NULL */);
PFAC_status_t PFACX_editGetPieces(PFACX_edit_t edit, size_t *h_pieceOff /* numPatterns + 2, CSR by ID */, int *h_pieceId, int *h_pieceStart,
                                  int *h_pieceLen, size_t n /* >= the number of pieces */);
PFAC_status_t PFACX_editClose(PFACX_edit_t edit);
PFAC_status_t PFACX_editMatchFromDevice(PFACX_edit_t edit, char *d_input, size_t size, int *d_ids, int *d_pos /* start */,
                                        int *d_end /* may be NULL */, int *d_dist /* may be NULL */, size_t capacity, size_t *h_num_matched);
PFAC_status_t PFACX_editMatchFromHost  (PFACX_edit_t edit, char *h_input, size_t size, int *h_ids, int *h_pos /* start */,
                                        int *h_end /* may be NULL */, int *h_dist /* may be NULL */, size_t capacity, size_t *h_num_matched);
PFAC_status_t PFACX_editPairsFromDevice(PFACX_edit_t edit, const char *d_input, size_t size,
                                        const int *d_pairIds, const int *d_pairPos, size_t numPairs, int *d_ids, int *d_pos /* start */,
                                        int *d_end /* may be NULL */, int *d_dist /* may be NULL */, size_t capacity, size_t *h_num_matched);

/* Signatures of byte classes with bounded repeats: the token rules of a secret / PII / DLP scanner -- `AKIA[0-9A-Z]{16}`, `ghp_[A-Za-z0-9]{36}`,
 * `xox[baprs]-[0-9A-Za-z-]{10,48}`, `[0-9]{3}-[0-9]{2}-[0-9]{4}`, `sess=[0-9a-f]{32};` --, what PFACX_sig* and PFACX_gapsig* leave out of scope as
 * "alternatives and negated bytes".  Both are special cases: `??` is the full class {1}, `5?` a class of 16 bytes {1}, a gap `{2-6}` the full
 * class {2,6}.  As for PFACX_gapsig* the library picks one run of literal bytes of each signature as its ANCHOR, loads the distinct anchors as the
 * handle's pattern set, scans for them with the product kernels and verifies every signature of every anchor occurrence against the input.
 *   CLASSES.  A table of numClasses byte classes, 1 .. 65 535 of them, each 256 bits in `unsigned int[8]` exactly as the class of
 *   PFACX_matchWords* / PFACX_split*: byte b is in the class iff bit b & 31 of word b >> 5 is set.  An empty class is refused.
 *   SIGNATURES.  S signatures, ids 1 .. S in the order given.  A signature is a sequence of ELEMENTS (class c, lo, hi): lo .. hi bytes, each in
 *   class c; 0 <= lo <= hi <= 65 535 and hi >= 1.  A literal byte is a class of one value with {1,1}.  The SLACK, the sum of hi - lo, is at most
 *   PFACX_CLSIG_MAX_SLACK = 63, the limit of PFACX_gapsig* for the same reason: where an element can lie relative to any other is one 64-bit mask.
 *   At open the library FUSES every maximal run of neighbouring elements that have a one-byte class and lo == hi into one LITERAL PART, whose bytes
 *   are the elements' bytes repeated lo times each; every other element is one CLASS PART.  After fusion a signature has 1 .. 64 parts, a literal
 *   part at most 65 535 bytes, and its span, the sum of all hi, stays below 2^23.
 *   EMBEDDING of a signature of m elements at start s in n bytes: run lengths r_j in [lo_j, hi_j], o_0 = s, o_{j+1} = o_j + r_j, every byte of
 *   in[o_j, o_j + r_j) in C_j, s >= 0 and end = o_m <= n.  Nothing outside [0, n) exists.
 *   BOUNDARIES, per signature, optional: a class index notBefore and a class index notAfter, -1 for none.  A start is VALID iff s == 0 or in[s - 1]
 *   is not in notBefore; an end e is valid iff e == n or in[e] is not in notAfter; an embedding counts only if its start and its end are valid.
 *   This is `(?<![..])` and `(?![..])`: without it a 16-letter token rule fires inside every longer base64 run.
 *   OCCURRENCE AND ENTRY.  Signature i occurs at s iff a valid embedding at s exists.  THE LIST holds one entry (id, start, end) per (id, start)
 *   that occurs; end is the LARGEST valid end over all embeddings at s -- the leftmost-longest end a token extractor wants --, with the open flag
 *   PFACX_CLSIG_SHORTEST_END the smallest, which is the meaning of PFACX_gapsig*.  Both are a maximum / minimum over all run-length choices, not
 *   what a greedy or lazy left-to-right choice finds.  Identical signatures are both reported.  The anchor has at least one byte, so start < end.
 *   ANCHOR.  The rule of PFACX_gapsigOpen over the literal parts: a candidate is a run of bytes other than 0x0A inside ONE literal part; the anchor
 *   is the longest run, of equal ones the one in the lowest part, then the leftmost, cut to its first maxAnchorLen bytes; 0 stands for 32 (the
 *   unmeasured supposition of PFACX_sigOpen -- still a supposition).  A signature without such a byte (`[0-9]{3}[a-f]{2}`) is refused.  Callers
 *   rely on PFACX_clsigGetAnchors.
 *   EACH OCCURRENCE ONCE.  The owner rule of PFACX_gapsig*: the anchor part a may lie at several offsets for one start.  (id, s) is listed by
 *   the occurrence of part a at the SMALLEST offset x that lies on some VALID embedding at s: an x whose tail cannot be completed, or completes
 *   only to ends that are not valid, owns nothing.
 *   ORDER: by the owning anchor occurrence, x + anchorOff ascending; at one position the longer anchor first; within one anchor ids descend;
 *   within one (anchor occurrence, signature) starts ascend.  It is NOT sorted by start.
 * PFACX_clsigOpen: host memory, copied -- h_classes holds 8 * numClasses words; element k is (h_elemClass[k], h_elemLo[k], h_elemHi[k]); the
 * elements of signature i are h_sigElem[i - 1] .. h_sigElem[i] - 1; h_notBefore / h_notAfter hold numSigs class indices each (-1: none; either
 * array may be NULL: none for any signature).  flags: 0 or PFACX_CLSIG_SHORTEST_END; any other bit: PFAC_STATUS_INVALID_PARAMETER.  It loads the
 * distinct anchors exactly as PFACX_gapsigOpen does: the handle's set is REPLACED, the handle becomes case-sensitive, handle id q is the q-th
 * distinct anchor in order of first appearance, and it checks under the handle's lock that the set it adopts is the one it loaded.
 * PFAC_STATUS_INVALID_PARAMETER, with the handle's set untouched: a required null pointer (h_classes, the three element arrays, h_sigElem, sig),
 * numSigs == 0 or >= 2^31 - 1, numClasses == 0 or > 65 535, an empty class, and -- with the id of the FIRST such signature in *badSig (may be
 * NULL; else 0) -- a signature without elements, a class index outside the table (in notBefore / notAfter too, other than -1), lo > hi,
 * hi == 0, hi > 65 535, a slack above 63, more than 64 parts after fusion, a literal part longer than 65 535 bytes, a span of 2^23 or more;
 * behind those, by id, a signature without a literal byte other than 0x0A.
 * PFACX_clsigOpenText: a parser in front of it and nothing else; one signature per '\n'-terminated line (a '\r' in front of the '\n' is
 * ignored), in a subset of regular-expression syntax chosen so that every accepted line means the same to Python's `re` on bytes with re.DOTALL.
 * A UNIT is a literal byte (any byte but `\ . [ ] ( ) { } ? * + | ^ $`; bytes >= 0x80 are literals), an escape (`\xHH`, `\n \r \t \f \v \0`, `\`
 * plus one of the metacharacters), a class escape (`\d \D \w \W \s \S`, ASCII; \s = blank \t \n \r \f \v), `.` (any byte), or a bracket set
 * `[...]` / `[^...]` of literals, escapes, class escapes and ranges `a-z`; inside a set `]` and `\` are always escaped, `-` is literal at the
 * first or last place or escaped, `^` is literal unless first.  A QUANTIFIER may follow a unit: `{n}`, `{n,m}`, or `?` = {0,1}; decimal, no
 * blanks.  At the very start of a line, optionally `(?<![set])`; at the very end, optionally `(?![set])`, each with a bracket set's body.
 * Refused with the 1-based line in *badLine: `* + | ( ) ^ $` elsewhere, `{n,}`, `{,m}`, n > m, a quantifier without a unit or two in a row, an
 * unclosed set, an empty set, a range that descends, an unknown escape, a number above 65 535, an empty line, bytes behind the last '\n', and a
 * line the binary form refuses.  A text without a line: *badLine = 0.  Identical classes are stored once.
 * PFACX_clsigGetAnchors: by signature id (n >= S + 1 entries each, entry 0 is 0; an array may be NULL) the handle's pattern id of the anchor,
 * the part AFTER FUSION that holds it, its offset inside that part and its length.
 * The object belongs to the handle like a gapped-signature object (PFAC_destroy closes it; stale after another read; host-only handles can
 * open).  The three match calls are those of PFACX_gapsig* word for word: the device form needs capacity >= size and its arrays take the scan's
 * unordered list first; the host and pairs forms take any capacity, 0 with null arrays is the count query; a longer list: the first `capacity`
 * entries, the full length, and PFACX_STATUS_OUTPUT_TRUNCATED; d_end may be NULL in every form and is only ever written below min(the list,
 * capacity); size >= 2^31 or a required null pointer: PFAC_STATUS_INVALID_PARAMETER; size == 0: success, nothing touched; a device form on a
 * host-only handle: PFAC_STATUS_LIB_NOT_EXIST; the pairs form ignores ids outside [1, F] and positions outside [0, size), refuses output arrays
 * (d_end included) that overlap the pair arrays and numPairs >= 2^31, and owns an occurrence only through pairs of its list.  The host form
 * follows PFAC_setPlatform.  All calls are synchronous and take the handle's lock.  The input is never modified, and nothing outside it is read.
 * MEMORY.  The tables, made by the first device call, are state of the object (deviceTableBytes, kept by PFACX_trim, freed by PFACX_clsigClose):
 * 32 bytes per signature, 16 per part, 4 (F + 2) bytes, the literal parts' bytes padded to a multiple of 4 each, 32 bytes per class.
 * Grow-only handle scratch as for PFACX_gapsig*.
 * COST: the compacted scan over the anchors with its ordering launches, then two passes over the pairs; a thread per pair runs the
 * whole search of a candidate -- up to 64 starts, each a walk of at most hi + 64 bytes per class part and a compare per set bit per literal part.
 * OUT OF SCOPE: unbounded repeats and slack above 63; alternation and groups; caseless literals (write `[Aa]`); `\b`; anchors chosen by rarity;
 * a wave per long search; stream and flow pairs; a full-result-vector form; a list sorted by start; a compiled-file form.
 *
 * THE BATCH FORMS (PFACX_clsigBatch*): one buffer that holds many packets, log lines or small files, cut by numSegments + 1 offsets of size_t
 * under the rules of PFACX_matchBatch* -- host offsets are validated (offsets[0] == 0, offsets[numSegments] == size, never decreasing; else
 * PFAC_STATUS_INVALID_PARAMETER), device offsets are never checked: each is clamped to [0, size] and raised to the largest entry in front of it,
 * so bad device offsets give the answer for the clamped offsets and never an access outside the buffers.  PFACX_split* makes such offsets on the
 * device.  Segment k is [o_k, o_{k+1}) of the clamped offsets, and every definition above holds with [o_k, o_{k+1}) in place of [0, n): an
 * embedding lies inside ONE segment; a start is valid iff s == o_k or in[s - 1] is not in notBefore; an end is valid iff e == o_{k+1} or in[e]
 * is not in notAfter; the owner rule and the largest / smallest end range over the embeddings inside the segment only.  THE LIST is exactly the
 * concatenation, in segment order, of what PFACX_clsigMatchFromDevice returns for each segment alone, o_k added to every start and end, each
 * segment's entries in that call's order; a batch of one segment is the plain call.  No filter over the plain call's list gives this: a crossing
 * embedding may hide a shorter one that stays inside (the reported end is a maximum or minimum), and an entry that a neighbour's byte forbids is
 * not in the plain list at all.
 *   A FULL notBefore CLASS therefore means "at the start of the segment" and a full notAfter class "ends with the segment": the text form writes
 *   them `(?<![\x00-\xff])` and `(?![\x00-\xff])`.
 *   d_segFirst / h_segFirst (may be NULL): numSegments + 1 entries of size_t; entry k is the list index of segment k's first entry, entry
 *   numSegments the full length; indices past `capacity` name entries that were not written, as in PFACX_matchAllBatchFromDevice.  Written
 *   whatever the capacity (the count query fills it).
 *   numSegments: at least 1 for size > 0, below 2^31 - 1; a NULL offsets array: PFAC_STATUS_INVALID_PARAMETER.
 *   The pairs form finds each pair's segment from its POSITION, so the pairs of a plain, a batch or an all-match scan of the handle over the same
 *   input all work; a pair whose position lies in no segment (in front of o_0, at or behind the last offset) owns nothing.  For a pair list that
 *   does not ascend by position the entries are still right pair by pair, and d_segFirst is unspecified.
 * Everything else is the plain calls' word for word: capacity (the device form: capacity >= size), truncation, the count query, size >= 2^31,
 * size == 0 (success, nothing touched, d_segFirst neither), host-only handles, the handle's lock, the overlap refusals of the pairs form,
 * PFACX_CLSIG_SHORTEST_END from the open call.  Scratch: 4 (numSegments + 1) bytes more.  The device form scans the whole buffer once, as the
 * plain call does, and searches each candidate inside its segment (DESIGN.md 5za says why that is enough, and what the call costs). */
#define PFACX_CLSIG_MAX_SLACK    63
#define PFACX_CLSIG_SHORTEST_END 1u
typedef struct PFACX_clsig_s *PFACX_clsig_t;
PFAC_status_t PFACX_clsigOpen(PFAC_handle_t handle, const unsigned int *h_classes /* 8 * numClasses */, size_t numClasses,
                              const unsigned int *h_elemClass, const unsigned int *h_elemLo, const unsigned int *h_elemHi /* numElems each */,
                              const size_t *h_sigElem /* numSigs + 1 */, const int *h_notBefore, const int *h_notAfter /* numSigs each; may be NULL */,
                              size_t numSigs, size_t maxAnchorLen /* 0: 32 */, unsigned int flags, PFACX_clsig_t *sig, int *badSig /* may be NULL */);
PFAC_status_t PFACX_clsigOpenText(PFAC_handle_t handle, const char *text, size_t size, size_t maxAnchorLen /* 0: 32 */, unsigned int flags,
                                  PFACX_clsig_t *sig, int *badLine /* may be NULL */);
PFAC_status_t PFACX_clsigGetAnchors(PFACX_clsig_t sig, int *h_anchorId, int *h_anchorPart /* after fusion */, int *h_anchorOff /* inside that part */,
                                    int *h_anchorLen, size_t n /* >= S + 1, indexed by ID */);
PFAC_status_t PFACX_clsigClose(PFACX_clsig_t sig);
PFAC_status_t PFACX_clsigMatchFromDevice(PFACX_clsig_t sig, char *d_input, size_t size,
                                         int *d_ids, int *d_pos, int *d_end /* may be NULL */, size_t capacity, size_t *h_num_matched);
PFAC_status_t PFACX_clsigMatchFromHost  (PFACX_clsig_t sig, char *h_input, size_t size,
                                         int *h_ids, int *h_pos, int *h_end /* may be NULL */, size_t capacity, size_t *h_num_matched);
PFAC_status_t PFACX_clsigPairsFromDevice(PFACX_clsig_t sig, const char *d_input, size_t size,
                                         const int *d_pairIds, const int *d_pairPos, size_t numPairs,
                                         int *d_ids, int *d_pos, int *d_end /* may be NULL */, size_t capacity, size_t *h_num_matched);
PFAC_status_t PFACX_clsigBatchMatchFromDevice(PFACX_clsig_t sig, char *d_input, size_t size, const size_t *d_offsets /* numSegments + 1 */,
                                              size_t numSegments, int *d_ids, int *d_pos, int *d_end /* may be NULL */, size_t capacity,
                                              size_t *d_segFirst /* numSegments + 1; may be NULL */, size_t *h_num_matched);
PFAC_status_t PFACX_clsigBatchMatchFromHost  (PFACX_clsig_t sig, char *h_input, size_t size, const size_t *h_offsets /* numSegments + 1 */,
                                              size_t numSegments, int *h_ids, int *h_pos, int *h_end /* may be NULL */, size_t capacity,
                                              size_t *h_segFirst /* numSegments + 1; may be NULL */, size_t *h_num_matched);
PFAC_status_t PFACX_clsigBatchPairsFromDevice(PFACX_clsig_t sig, const char *d_input, size_t size, const size_t *d_offsets /* numSegments + 1 */,
                                              size_t numSegments, const int *d_pairIds, const int *d_pairPos, size_t numPairs,
                                              int *d_ids, int *d_pos, int *d_end /* may be NULL */, size_t capacity,
                                              size_t *d_segFirst /* numSegments + 1; may be NULL */, size_t *h_num_matched);

/* Cover: an UNSORTED list of intervals as the maximal runs of the bytes they cover -- the step between a list of (id, start, end) hits
 * (PFACX_gapsig*, PFACX_edit*, PFACX_clsig* and PFACX_clsigBatch*, whose lists are ordered by the owning anchor, not by start, and hold duplicate
 * starts, nested and overlapping intervals) and PFACX_redactSpansFromDevice, which takes an ascending disjoint list.  Any caller-made list works
 * as well; no matcher runs, and no pattern set is needed.
 *   COVERED.  Interval i is [s_i, e_i) with s_i = start[i] and e_i = end[i] -- with PFACX_COVER_LENGTHS in `flags` the second array holds lengths
 *   and e_i = start[i] + end[i] in 64-bit arithmetic.  Every interval is clamped to [0, size] where it is read; one that is empty after the clamp
 *   (e <= s, s >= size, e <= 0, a negative length) covers nothing.  Byte b of [0, size) is covered iff some clamped interval holds it.  No order
 *   is assumed: duplicates, nesting and overlap are all legal.  No input buffer is taken and none is read: `size` only bounds the positions.
 *   The SPANS are exactly those of PFACX_matchSpans*: the maximal runs of covered bytes, ascending, disjoint and never adjacent -- intervals that
 *   touch ([a, b) and [b, c)) form one span.  spanLen[i] >= 1; *h_coveredBytes = the sum of the lengths; numSpans <= (size + 1) / 2.  The result
 *   is a legal argument of PFACX_redactSpansFromDevice as it stands.
 *   Spans know NO SEGMENTS: over the list of a batch call (PFACX_clsigBatch*, whose entries are offsets into the whole buffer) a span that ends
 *   with one segment and one that starts the next touch and come out as one.
 * capacity: entries of each span array, ANY value -- the arrays are not a scan's scratch here.  More spans than `capacity`: exactly the first
 * `capacity` spans are written and nothing behind them, both counts are still the full ones, and the call returns PFACX_STATUS_OUTPUT_TRUNCATED.
 * capacity == 0 with null span arrays is the count query.
 * PFAC_STATUS_INVALID_PARAMETER: a null count pointer, null interval arrays with numIntervals > 0, null span arrays with capacity > 0, size >=
 * 2^31, numIntervals >= 2^31, a flag bit other than PFACX_COVER_LENGTHS and, in the device form, a span array that overlaps an interval array (the
 * rule of the pairs forms).  size == 0: success, both counts 0, nothing touched.  numIntervals == 0: success, both counts 0, no span written.
 * The device form on a host-only handle: PFAC_STATUS_LIB_NOT_EXIST.  The host form runs on the CPU on every platform, host-only handles included:
 * the clamped intervals sorted by start and one sweep, memory proportional to numIntervals, never to `size`.  Both forms are synchronous and take
 * the handle's lock.  The interval arrays are never modified.
 * MEMORY of the device form: grow-only handle scratch sized by `size` alone -- a hierarchy of bitmaps with fan-out 32, a bit per byte at the
 * bottom: about size / 8 x 32 / 31 bytes, plus 8 bytes per 32 KiB of positions -- zeroed by one memset per call: deviceScratchBytes of
 * PFACX_getInfo, freed by PFACX_trim.
 * COST: the memset, at most 14 atomic ORs per interval however long it is, two passes over the bitmap; not measured yet. */
#define PFACX_COVER_LENGTHS 1u   /* the second array holds lengths, not ends */
PFAC_status_t PFACX_coverSpansFromDevice(PFAC_handle_t handle, const int *d_start, const int *d_end, size_t numIntervals, size_t size,
                                         unsigned int flags, int *d_spanStart, int *d_spanLen, size_t capacity,
                                         size_t *h_numSpans, size_t *h_coveredBytes);
PFAC_status_t PFACX_coverSpansFromHost  (PFAC_handle_t handle, const int *h_start, const int *h_end, size_t numIntervals, size_t size,
                                         unsigned int flags, int *h_spanStart, int *h_spanLen, size_t capacity,
                                         size_t *h_numSpans, size_t *h_coveredBytes);

/* Order: a hit list put in START ORDER on the device -- the step between the lists of PFACX_sig* (id, start), PFACX_approx* (id, start, distance),
 * PFACX_gapsig* / PFACX_clsig* / PFACX_clsigBatch* (id, start, end) and PFACX_edit* (id, start, end, distance), which are in pair order, chain order,
 * id / table order -- the order of the owning anchor, not of the start --, and every call that takes positions non-decreasing.  Any caller-made list
 * works as well; no matcher runs, and no pattern set is needed.
 *   ORDER.  Entry k is the tuple of the given columns at index k; the call permutes the entries in place.  `start` ends up non-decreasing as SIGNED
 *   ints.  No range is assumed: negative starts (streams, flows) and values >= the size of any buffer are legal keys, which is why the call takes no
 *   `size`.  Among equal starts the incoming order is kept: the sort is stable.  With PFACX_ORDER_TIES_BY_ID in `flags`, entries with equal starts
 *   are put in ascending id order first (signed); entries equal in both start and id keep their incoming order.
 *   COLUMNS.  d_ids, d_end and d_aux are optional; each one that is given is permuted with `start`.  A bare position list is legal.
 *   PERMUTATION.  d_perm (numHits ints), where given, receives the incoming index of the entry now at k: callers with more columns gather them
 *   themselves.  Without d_perm the permutation is never materialised for the caller.
 *   ALREADY ORDERED.  *h_wasOrdered (where given) is 1 iff the list was already in the requested order; then no column is written and d_perm is the
 *   identity.  Every list that the library's reduce, all, words, disjoint and groups calls return takes this exit.
 *   The result is a legal argument of PFACX_locatePairsFromDevice, of PFACX_capturePairsFromDevice (with PFACX_CAPTURE_AT_POS) and of
 *   PFACX_coverSpansFromDevice.  Over a PFACX_clsigBatch* list, segFirst stays valid as it is: segments are ascending disjoint ranges and every
 *   start lies inside its segment, so ordering the whole list orders each segment's slice and moves no entry across a slice.
 * PFAC_STATUS_INVALID_PARAMETER: a null handle, a null d_start with numHits > 0, numHits >= 2^31, a flag bit other than PFACX_ORDER_TIES_BY_ID, that
 * flag without d_ids, any two of the given arrays overlapping, d_perm included (the rule of the pairs forms).  numHits == 0: success, nothing
 * touched, *h_wasOrdered = 1.  The device form on a host-only handle: PFAC_STATUS_LIB_NOT_EXIST.  Both forms are synchronous, take the handle's lock
 * and need no pattern set.  Scratch that cannot be allocated: PFAC_STATUS_ALLOC_FAILED, the caller's arrays untouched -- nothing of the caller's is
 * written before the last sorting pass has finished.  The host form is a stable sort of an index array with the same comparator, on the CPU on
 * every platform, host-only handles included, memory proportional to numHits.
 * MEMORY of the device form: grow-only handle scratch (deviceScratchBytes of PFACX_getInfo, freed by PFACX_trim), not allocated before the first
 * call: 40 bytes of probe words for a list that is found ordered; for one that needs a pass, with B = min((numHits + 2047) / 2048, 8 x compute
 * units) blocks, 40 + 16 numHits (two buffers of (key, index) pairs) + 4 numHits (one column temp) + 1024 B + 1024 B + 4 (the digit counts of the
 * blocks and their prefix) bytes, each of the six parts rounded up to 256.
 * COST: one probe launch; then three launches per 8-bit digit in which two keys differ (starts below 2^24 and ids below 2^16: three
 * digits, five with the ties flag), one gather and one copy per column.
 * OUT OF SCOPE: ordering by end or by id alone, dropping duplicates, 64-bit positions, merging two ordered lists, and exploiting the bounded
 * displacement of the library's own lists (an entry lies at most a pattern length from its place; open). */
#define PFACX_ORDER_TIES_BY_ID 1u   /* among equal starts: ascending id, then incoming order */
PFAC_status_t PFACX_orderHitsFromDevice(PFAC_handle_t handle, int *d_start, int *d_ids /* may be NULL */, int *d_end /* may be NULL */,
                                        int *d_aux /* may be NULL */, size_t numHits, unsigned int flags, int *d_perm /* may be NULL */,
                                        int *h_wasOrdered /* may be NULL */);
PFAC_status_t PFACX_orderHitsFromHost  (PFAC_handle_t handle, int *h_start, int *h_ids /* may be NULL */, int *h_end /* may be NULL */,
                                        int *h_aux /* may be NULL */, size_t numHits, unsigned int flags, int *h_perm /* may be NULL */,
                                        int *h_wasOrdered /* may be NULL */);

/* Split: the offsets that cut a buffer into records at the bytes of a delimiter class -- the `d_offsets` that PFACX_matchBatch*,
 * PFACX_matchAllBatchFromDevice, PFACX_rules*, PFACX_countBatch* and PFACX_groups* take, made where the text lies: the lines of a log, the records
 * of a CRLF protocol, the fields of a line.
 *   THE CLASS D is a set of byte values, 256 bits in `unsigned int cls[8]` exactly as the class of PFACX_matchWords*: byte b is in D if bit b & 31 of
 *   cls[b >> 5] is set.  The eight words are HOST memory in both calls and are copied.  h_class == NULL: the class {'\n'}.  The class is tested on the
 *   caller's bytes: a caseless handle (PFACX_READ_NOCASE) changes nothing -- 'A' in the class does not cut at 'a' --, and the input is never written.
 *   CUTS.  Let the input have n bytes; a position p with in[p] in D is a DELIMITER.
 *     flags 0:            every delimiter p with p + 1 < n gives the cut p + 1: a delimiter closes the segment in front of it.
 *     PFACX_SPLIT_BEFORE: every delimiter p with p > 0 gives the cut p: a delimiter opens the segment behind it.
 *     PFACX_SPLIT_RUNS:   only one delimiter of each maximal run of delimiters cuts -- without BEFORE the last one (in[p + 1] is not in D), with
 *                         BEFORE the first one (in[p - 1] is not in D).
 *   Cuts are distinct and lie strictly inside (0, n).  THE OFFSETS are 0, then the cuts ascending, then n; numSegments = the number of cuts + 1;
 *   segment k is in[offsets[k], offsets[k + 1]).  No segment is ever empty.
 *   CONSEQUENCES: with flags 0 and the default class, segment k is line k of the PFACX_matchLines* definition together with its '\n' (an unterminated
 *   last line is a segment like every other), and numSegments == numLines of those calls.  An empty class gives one segment, [0, n).  A full class
 *   gives n segments of one byte, under PFACX_SPLIT_RUNS one.
 *   SEGMENT ENDS.  Delimiters are never dropped: a segment includes its closing delimiter or, with PFACX_SPLIT_BEFORE, its opening one.  For the
 *   windows of PFACX_rulesOpenEx the delimiter counts as a byte of the segment: a PFACX_RULE_FROM_END window over lines cut with flags 0 measures
 *   from behind the '\n' -- "in the last 16 bytes of the line" needs offset 1 --, while PFACX_SPLIT_BEFORE puts the delimiter at the segment's front,
 *   where FROM_END windows never see it (windows from the start then count it as byte 0).  This is why BEFORE exists.
 * OUTPUT.  *h_numSegments is always the full count; *h_longest (may be NULL) is the longest segment in bytes -- the capacity a per-segment buffer
 * needs --, the full value also when the list is truncated.  `capacity` is the number of entries of the offsets array: numSegments + 1 are needed,
 * size + 1 always suffices.  A smaller capacity: exactly the first `capacity` entries are written -- 0 and the first capacity - 1 cuts --, nothing
 * at or behind them, and the call returns PFACX_STATUS_OUTPUT_TRUNCATED.  capacity == 0 is the count query: the array may be null.
 * LIMITS.  There is no 2^31 limit: positions are computed in 64 bits throughout (of the batch calls the full-result form has no limit either; the
 * others refuse sizes from 2^31 on).  size == 0: success, 0 segments, *h_longest = 0, nothing written.  PFAC_STATUS_INVALID_PARAMETER: an unknown
 * flag bit; a null handle, input or h_numSegments; a null array with capacity > 0; an offsets pointer that is not 8-byte aligned.  The call needs no
 * pattern set: on a handle without one it succeeds.  The device form on a host-only handle: PFAC_STATUS_LIB_NOT_EXIST.  Both forms take the handle's
 * lock and are synchronous (the counts come to the host).  The host form is a host loop on every platform, as PFACX_flowRulesPairsFromHost is; a
 * class of one byte runs at the speed of memchr.
 * MEMORY of the device form: grow-only handle scratch sized by the number of tiles alone -- with T = ceil(size / 16384): 8 (T + 1) + 16 T + 4 T +
 * 4 T + 4 T + 8 bytes, each term rounded up to 256: 0.0022 bytes per input byte, whatever the data.  Counted under deviceScratchBytes of
 * PFACX_getInfo, freed by PFACX_trim, not allocated before the first split call.
 * COST: two streaming reads of the input -- one counts the cuts per tile, one writes them -- and 8 bytes written per segment; between
 * them two one-block launches over the per-tile values.
 * OUT OF SCOPE: multi-byte delimiters ("\r\n" as ONE delimiter: the class {'\r', '\n'} with PFACX_SPLIT_RUNS cuts once per "\r\n", and once per
 * blank-line run); dropping the delimiters from the segments -- the batch calls take contiguous segments; quoting rules for CSV; device-resident
 * classes; splitting the pieces of a stream or flow. */
#define PFACX_SPLIT_BEFORE 1u   /* a delimiter opens the segment behind it instead of closing the one in front */
#define PFACX_SPLIT_RUNS   2u   /* a maximal run of delimiters cuts once */
PFAC_status_t PFACX_splitFromDevice(PFAC_handle_t handle, const char *d_input, size_t size, const unsigned int *h_class /* 8 words or NULL */,
                                    unsigned int flags, size_t *d_offsets, size_t capacity, size_t *h_numSegments, size_t *h_longest /* may be NULL */);
PFAC_status_t PFACX_splitFromHost  (PFAC_handle_t handle, const char *h_input, size_t size, const unsigned int *h_class /* 8 words or NULL */,
                                    unsigned int flags, size_t *h_offsets, size_t capacity, size_t *h_numSegments, size_t *h_longest /* may be NULL */);

/* Locate: the record and the column of every match -- what `grep -n -b -o` prints: the line of a log and the byte in it, the record of a CRLF protocol
 * and the offset inside it.  Every compacted call hands back positions as byte offsets into the buffer; these calls turn them into (record, column)
 * where the text lies, without the offsets array of PFACX_split*.
 *   RECORDS.  The class D (`unsigned int cls[8]`, HOST memory, copied; NULL: {'\n'}) and the flags (PFACX_SPLIT_BEFORE, PFACX_SPLIT_RUNS, the same
 *   values; any other bit: PFAC_STATUS_INVALID_PARAMETER) are those of PFACX_split*, word for word.  The class is tested on the caller's bytes: a
 *   caseless handle changes nothing.  Let C be the cuts PFACX_split* defines for (input, D, flags).  For a position p of [0, size):
 *     record(p) = the number of cuts c <= p;   start(p) = the largest cut <= p, 0 if there is none;   column(p) = p - start(p).
 *   Equivalently, with `offsets` the array PFACX_split* returns: record = (the number of offsets <= p) - 1, column = p - offsets[record].
 *   CONSEQUENCES: with the default class and flags 0, record is the 0-based line number (lineIndex of PFACX_matchLines*) and column the 0-based byte
 *   offset in the line; with flags 0 the '\n' byte itself belongs to the line it ends.  Both values are int: size >= 2^31 is
 *   PFAC_STATUS_INVALID_PARAMETER, as for every pairs call.  A position outside [0, size) -- the negative positions of streams and flows -- gets
 *   record = column = -1.
 * THE PAIRS FORMS take a position list that any call of the library left behind (reduce, matchAll, words, disjoint, groups).  The list must be
 * non-decreasing; equal neighbours are allowed, as PFACX_matchAll* produces them; every list the library returns is.  The arrays are the caller's
 * contract (device memory in the device form): a list that is not non-decreasing gives unspecified record and column values, but never an access
 * outside input[0, size), pos[0, numPairs) or the outputs' numPairs entries.  d_column may be NULL.  *h_numRecords (may be NULL) is the segment
 * count PFACX_split* would report.  numPairs == 0 or size == 0: success, no array is touched; *h_numRecords is still written (0 for size == 0).
 * The calls need no pattern set, are synchronous and take the handle's lock.  PFAC_STATUS_INVALID_PARAMETER: an unknown flag bit; a null handle or
 * input; a null list or record array with numPairs > 0; size or numPairs >= 2^31.  The device form on a host-only handle:
 * PFAC_STATUS_LIB_NOT_EXIST.  The host form is a host loop on every platform: one forward walk over input and positions together, no offsets array.
 * THE SCAN FORMS scan, then locate: ids and pos (`size` entries each) are exactly what PFAC_matchFromDeviceReduce / PFAC_matchFromHostReduce return,
 * record and column (may be NULL) belong to those pairs.  More pairs than locCapacity: exactly the first locCapacity record and column entries are
 * written, *h_num_matched is the full count and the call returns PFACX_STATUS_OUTPUT_TRUNCATED (locCapacity == 0: both arrays may be null).  A
 * caseless handle folds for the match and never for the class.  Error cases are those of PFAC_matchFromDeviceReduce, plus the flag check and a null
 * record array with locCapacity > 0.  The host form follows PFAC_setPlatform as PFACX_matchAllFromHost does: on the GPU platform the staged-piece
 * path of the other host forms, then the host loop.
 * MEMORY of the device forms: grow-only handle scratch sized by the number of tiles alone -- with T = ceil(size / 16384): 8 (T + 1) + 4 T + 4 T
 * bytes, each term rounded up to 256: 0.001 bytes per input byte, whatever the data and however many pairs.  Counted under deviceScratchBytes of
 * PFACX_getInfo, freed by PFACX_trim, not allocated before the first locate call.
 * COST: one streaming read of the input that counts the cuts per tile, two one-block launches over the per-tile values, a launch over
 * the list, and a second read of only the tiles that hold a pair; 4 bytes read and 8 written per pair.
 * OUT OF SCOPE: stream and flow pairs (positions that count from a piece's first byte); per-segment records of a batch; columns in characters (UTF-8)
 * or with tab expansion; 1-based numbering; unsorted position lists; device-resident classes. */
PFAC_status_t PFACX_locatePairsFromDevice(PFAC_handle_t handle, const char *d_input, size_t size, const unsigned int *h_class /* 8 words or NULL */,
                                          unsigned int flags, const int *d_pos, size_t numPairs, int *d_record, int *d_column /* may be NULL */,
                                          size_t *h_numRecords /* may be NULL */);
PFAC_status_t PFACX_locatePairsFromHost  (PFAC_handle_t handle, const char *h_input, size_t size, const unsigned int *h_class /* 8 words or NULL */,
                                          unsigned int flags, const int *h_pos, size_t numPairs, int *h_record, int *h_column /* may be NULL */,
                                          size_t *h_numRecords /* may be NULL */);
PFAC_status_t PFACX_matchLocatedFromDevice(PFAC_handle_t handle, char *d_input, size_t size, const unsigned int *h_class /* 8 words or NULL */,
                                           unsigned int flags, int *d_ids, int *d_pos /* size entries each */, int *d_record,
                                           int *d_column /* may be NULL */, size_t locCapacity, int *h_num_matched);
PFAC_status_t PFACX_matchLocatedFromHost  (PFAC_handle_t handle, char *h_input, size_t size, const unsigned int *h_class /* 8 words or NULL */,
                                           unsigned int flags, int *h_ids, int *h_pos /* size entries each */, int *h_record,
                                           int *h_column /* may be NULL */, size_t locCapacity, int *h_num_matched);

/* Capture: the value behind every match -- what a log or protocol user wants from a key like `Host: `, `user=`, `"session_id":"` or
 * `Content-Length:`: the bytes from the end of the match up to the next delimiter, with any blanks in front of the value skipped.  The patterns are
 * the keys, these calls give the (start, length) of the values on the device, and PFACX_gatherLinesFromDevice writes them as text: two calls, no
 * host round trip.
 *   INPUTS.  input[0, n), 0 < n < 2^31.  A pair list (id_k, pos_k), k < numPairs < 2^31: positions non-decreasing, equal neighbours allowed; every
 *   list the library returns is accepted (reduce, matchAll, words, disjoint, groups).  A skip class S: `h_skip`, 8 words of HOST memory, copied;
 *   NULL: the empty class.  A stop class D: `h_stop`, 8 words of HOST memory, copied; NULL: {'\n'}.  Bits are laid out exactly as for PFACX_split*.
 *   `window`, a size_t; 0: unbounded.  `flags`.  Both classes are tested on the caller's bytes: a caseless handle folds nothing here.  A byte that is
 *   in both classes counts as a stop byte only: the library uses S \ D, computed once on the host.
 *   FOR PAIR k:
 *     1. If pos_k is outside [0, n), then valStart[k] = -1 and valLen[k] = 0.  The same holds without PFACX_CAPTURE_AT_POS when id_k is outside
 *        [1, F] (F: the number of patterns).  The negative positions of streams and flows, and a caller's bad list, therefore give nothing.
 *     2. b = pos_k + len(id_k), where len(id_k) is the length of pattern id_k.  With PFACX_CAPTURE_AT_POS, b = pos_k.  Then b = min(b, n).
 *     3. w = n if window == 0, else min(n, b + window).  The pair never looks at a byte at or beyond w.
 *     4. s is the smallest position in [b, w) whose byte is not in S \ D.  If there is none, s = w.
 *     5. e is the smallest position in [s, w) whose byte is in D.  If there is none, e = w.
 *     6. valStart[k] = s and valLen[k] = e - s.  Zero is a legal length: an empty value, or a window spent on blanks.
 *   PFACX_CAPTURE_AT_POS uses the position as it is: ids may be NULL, the call needs no pattern set, and pos_k == n is then still outside [0, n) and
 *   falls under rule 1.  Any other flag bit: PFAC_STATUS_INVALID_PARAMETER.
 *   CONSEQUENCES: the stop byte is never part of the value.  With S empty, window == 0 and the default D, valStart + valLen is the position of the
 *   '\n' that ends the line of b; if the line has none, it is n.  D = {'\r', '\n'} handles CRLF.
 *   PFACX_gatherLinesFromDevice(d_input, size, d_valStart, d_valLen, numPairs, ...) writes the values as text, one per line; entries with
 *   valStart == -1 come out as empty lines (that call clamps: -1 becomes offset 0, and the length is 0).
 * THE PAIRS FORMS.  numPairs == 0 or size == 0: success, no array is touched.  PFAC_STATUS_INVALID_PARAMETER: a null handle or input; a null pos,
 * valStart or valLen with numPairs > 0; null ids without PFACX_CAPTURE_AT_POS; size or numPairs >= 2^31; an unknown flag.  Without
 * PFACX_CAPTURE_AT_POS a handle with no pattern set: PFAC_STATUS_PATTERNS_NOT_READY.  The device form on a host-only handle:
 * PFAC_STATUS_LIB_NOT_EXIST.  The arrays are the caller's contract (device memory in the device form): a list that is not non-decreasing gets
 * unspecified values, but never an access outside input[0, size), the list, or the outputs' numPairs entries.  The output arrays must not overlap the
 * list.  The calls are synchronous and take the handle's lock.  The host form is a host loop on every platform.
 * THE SCAN FORMS are PFAC_matchFromDeviceReduce (on the host: the same longest pairs) followed by the capture of the first min(count, capCapacity)
 * pairs: ids and pos (`size` entries each) are exactly what that call returns, valStart and valLen belong to those pairs.  More pairs than
 * capCapacity: exactly the first capCapacity entries are written, *h_num_matched is the full count and the call returns
 * PFACX_STATUS_OUTPUT_TRUNCATED (capCapacity == 0: both arrays may be null).  PFACX_CAPTURE_AT_POS is accepted.  A caseless handle folds for the match
 * and never for the classes.  Error cases are those of PFAC_matchFromDeviceReduce, plus the flag check and a null valStart or valLen with
 * capCapacity > 0.  The host form follows PFAC_setPlatform as PFACX_matchLocatedFromHost does.
 * MEMORY of the device forms: grow-only handle scratch sized by the number of tiles alone -- with T = ceil(size / 16384): 4 T + 8 bytes, each term
 * rounded up to 256, whatever the data and however many pairs; without PFACX_CAPTURE_AT_POS also the device copy of the pattern lengths that the
 * batch and spans calls share (4 bytes per pattern).  Counted under deviceScratchBytes of PFACX_getInfo, freed by PFACX_trim, not allocated before
 * the first capture call.
 * COST: no pass over the whole input.  A launch over the tiles' first-pair words, a launch over the list, and one read of only the
 * tiles of 16 KiB that hold a pair, each with the 1 KiB behind it; 8 bytes read (4 with PFACX_CAPTURE_AT_POS) plus one gathered length and 8 written
 * per pair.  A value that starts or ends more than 1 KiB behind its pair's tile is finished on the input itself, a pair alone: an unbounded window on
 * hostile input (no stop byte, or nothing but skip bytes) costs up to the rest of the buffer per pair.  Callers with untrusted input set a window.
 * OUT OF SCOPE: values in front of a match; quoted values and escapes; trimming trailing blanks; multi-byte stops; converting a value to a number;
 * per-segment bounds of a batch (a stop class that contains the record delimiter gives the same effect); the pairs of streams and flows;
 * device-resident classes; unsorted lists; a flag telling "ended at the window" from "ended at a stop byte" (the caller tests
 * input[valStart + valLen]). */
#define PFACX_CAPTURE_AT_POS 1u
PFAC_status_t PFACX_capturePairsFromDevice(PFAC_handle_t handle, const char *d_input, size_t size, const unsigned int *h_skip /* 8 words or NULL */,
                                           const unsigned int *h_stop /* 8 words or NULL */, size_t window, unsigned int flags,
                                           const int *d_ids /* NULL with PFACX_CAPTURE_AT_POS */, const int *d_pos, size_t numPairs, int *d_valStart,
                                           int *d_valLen);
PFAC_status_t PFACX_capturePairsFromHost  (PFAC_handle_t handle, const char *h_input, size_t size, const unsigned int *h_skip /* 8 words or NULL */,
                                           const unsigned int *h_stop /* 8 words or NULL */, size_t window, unsigned int flags,
                                           const int *h_ids /* NULL with PFACX_CAPTURE_AT_POS */, const int *h_pos, size_t numPairs, int *h_valStart,
                                           int *h_valLen);
PFAC_status_t PFACX_matchCapturedFromDevice(PFAC_handle_t handle, char *d_input, size_t size, const unsigned int *h_skip /* 8 words or NULL */,
                                            const unsigned int *h_stop /* 8 words or NULL */, size_t window, unsigned int flags, int *d_ids,
                                            int *d_pos /* size entries each */, int *d_valStart, int *d_valLen, size_t capCapacity,
                                            int *h_num_matched);
PFAC_status_t PFACX_matchCapturedFromHost  (PFAC_handle_t handle, char *h_input, size_t size, const unsigned int *h_skip /* 8 words or NULL */,
                                            const unsigned int *h_stop /* 8 words or NULL */, size_t window, unsigned int flags, int *h_ids,
                                            int *h_pos /* size entries each */, int *h_valStart, int *h_valLen, size_t capCapacity,
                                            int *h_num_matched);

#ifdef __cplusplus
}
#endif

#endif /* PFAC_EXT_H_ */
