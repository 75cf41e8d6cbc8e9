/*
 * pfac_module.h -- the plugin seam between libpfac.so (host API, pattern
 * compiler, tables) and the per-architecture kernel module libpfac_gfx950.so.
 *
 * The reference binds the same four C symbols out of libpfac_sm_<NN>.so with
 * dlopen/dlsym at PFAC_create() time (PFAC/include/PFAC_P.h:41-45,
 * PFAC/src/PFAC.cpp:158-201); the names (including the historical spelling
 * "warpper") and argument lists are kept so the seam is recognisable and a
 * module built for another architecture could be dropped in beside this one.
 * The module file name is derived from hipDeviceProp_t::gcnArchName
 * ("gfx950:sramecc+:xnack-" -> "libpfac_gfx950.so") instead of 10*major+minor.
 *
 * The texture-bind mutex the reference module calls back into
 * (PFAC_P.h:217-226) has no gfx950 counterpart: a buffer-resource descriptor
 * is built in SGPRs per launch, there is no process-global binding to guard.
 */
#ifndef PFAC_MODULE_H_
#define PFAC_MODULE_H_

#include "PFAC.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ref PFAC_P.h:41-42 (PFAC_kernel_protoType): full result, one int per input byte. */
typedef PFAC_status_t (*PFAC_kernel_protoType)(PFAC_handle_t handle, char *d_input_string,
                                               size_t input_size, int *d_matched_result);

/* ref PFAC_P.h:44-45 (PFAC_reduce_kernel_protoType): compacted (id, position) output. */
typedef PFAC_status_t (*PFAC_reduce_kernel_protoType)(PFAC_handle_t handle, int *d_input_string,
                                                      int input_size, int *d_match_result,
                                                      int *d_pos, int *h_num_matched,
                                                      int *h_match_result, int *h_pos);

/* Exported by libpfac_gfx950.so.
 * ref PFAC_kernel.cu:90-244 (dense table) and PFAC_kernel_spaceDriven.cu:149-348 (hashed). */
PFAC_status_t PFAC_kernel_timeDriven_warpper(PFAC_handle_t handle, char *d_input_string,
                                             size_t input_size, int *d_matched_result);
PFAC_status_t PFAC_kernel_spaceDriven_warpper(PFAC_handle_t handle, char *d_input_string,
                                              size_t input_size, int *d_matched_result);

/* ref PFAC_reduce_kernel.cu:172-295 and PFAC_reduce_inplace_kernel.cu:155-323. */
PFAC_status_t PFAC_reduce_kernel(PFAC_handle_t handle, int *d_input_string, int input_size,
                                 int *d_match_result, int *d_pos, int *h_num_matched,
                                 int *h_match_result, int *h_pos);
PFAC_status_t PFAC_reduce_inplace_kernel(PFAC_handle_t handle, int *d_input_string, int input_size,
                                         int *d_match_result, int *d_pos, int *h_num_matched,
                                         int *h_match_result, int *h_pos);

/* Batch matching (no reference counterpart; include/pfac_ext.h: PFACX_matchBatch*), scan_batch.hip.  Both run behind a scan of
 * the whole concatenation on the default stream and turn its result into the concatenation of the per-segment results:
 * d_offsets holds numSegments + 1 entries (clamped to [0, size] on the device), d_patternLen the pattern lengths by id.
 * PFACX_batchFixup: full result, asynchronous.  PFACX_batchReduceFixup: the *count (id, position) pairs of a compacted-output
 * scan; pairs that lose their match drop out (order kept), *count is updated, d_segFirst[numSegments + 1] filled; synchronous. */
PFAC_status_t PFACX_batchFixup(PFAC_handle_t handle, const char *d_input, size_t size, const size_t *d_offsets, size_t numSegments,
                               int *d_matched_result, const int *d_patternLen);
PFAC_status_t PFACX_batchReduceFixup(PFAC_handle_t handle, const char *d_input, size_t size, const size_t *d_offsets, size_t numSegments,
                                     int *d_ids, int *d_pos, int *count, int *d_segFirst, const int *d_patternLen);

/* All matches (no reference counterpart; include/pfac_ext.h: PFACX_matchAll*).
 * PFACX_allReduce, scan_module.hip: PFAC_reduce_kernel (hashed == 0) / PFAC_reduce_inplace_kernel (hashed != 0) whose ordering
 * writes the ordered (id, position) pairs into the handle's all-match scratch -- one buffer, pfac::DeviceScratch::allPairs: the ids in its first
 * half, the positions in its second -- instead of into d_match_result / d_pos, which hold `input_size` entries and take only the
 * scan's unordered list; synchronous, *h_num_matched = the number of pairs.
 * PFACX_allExpand, scan_all.hip (its passes and launches are the expansion frame of scan_passes.h): expands `count` ordered longest pairs through d_table (pfac::Int2 {prefixPattern, chainLen} by
 * id) into d_ids / d_pos, every pattern at a position, longest first; slots >= capacity are not written; *h_total = the length
 * of the whole list.  d_segFirst (or null): numSegments + 1 size_t, entry k = d_segFirstPairs[k] (the first longest pair of
 * segment k) through the expansion.  d_table may be null when count == 0 or every chain has length 1 (then only d_segFirst is
 * written).  Synchronous. */
PFAC_status_t PFACX_allReduce(PFAC_handle_t handle, int *d_input_string, int input_size, int *d_match_result, int *d_pos,
                              int *h_num_matched, int hashed);
PFAC_status_t PFACX_allExpand(PFAC_handle_t handle, const int *d_pairIds, const int *d_pairPos, size_t count, const void *d_table,
                              int *d_ids, int *d_pos, size_t capacity, const int *d_segFirstPairs, size_t numSegments, size_t *d_segFirst,
                              size_t *h_total);

/* Caseless pattern sets (no reference counterpart; include/pfac_ext.h: PFACX_READ_NOCASE), scan_fold.hip: the ASCII fold of n bytes
 * of src into dst ('A'-'Z' -> 'a'-'z', every other byte unchanged), any alignment and length, in place (src == dst) or into a buffer
 * that does not overlap src.  Asynchronous, on the default stream: the scan behind it reads dst in stream order. */
PFAC_status_t PFACX_foldInput(PFAC_handle_t handle, const char *src, char *dst, size_t n);

/* Streams (no reference counterpart; include/pfac_ext.h: PFACX_stream*).
 * PFACX_streamSeam, scan_stream.hip: one launch for the seam between the bytes a stream carries and a new piece.  d_carry holds the
 * last `carried` bytes of the stream so far (folded, for a caseless set), d_piece the new piece of `size` bytes (may be null when
 * size == 0: the flush).  The launch walks start positions [0, numFinal) of [carry | first min(size, maxPatternLen - 1) bytes of the
 * piece] -- numFinal <= carried: the carried positions this call makes final -- and writes their (id, position - carried) pairs in
 * position order to d_ids / d_pos; it also writes the next carry, the last nextCarried = min(maxPatternLen - 1, carried + size) bytes
 * of [carry | piece], to d_carryNext (never d_carry: a failed call leaves the stream as it was).  d_stage: device scratch of
 * carried + min(size, maxPatternLen - 1) bytes for a seam that does not fit the LDS, else null.  Synchronous: *h_count = the pairs.
 * PFACX_streamReduce, scan_module.hip: PFAC_reduce_kernel / PFAC_reduce_inplace_kernel (hashed != 0) for positions [0, owned) of an
 * input of `readable` >= owned bytes: the bytes behind `owned` are read-ahead only (their positions belong to the next call). */
PFAC_status_t PFACX_streamSeam(PFAC_handle_t handle, const char *d_carry, size_t carried, const char *d_piece, size_t size, size_t numFinal,
                               char *d_carryNext, char *d_stage, int *d_ids, int *d_pos, int *h_count);
PFAC_status_t PFACX_streamReduce(PFAC_handle_t handle, int *d_input_string, int owned, int readable, int *d_match_result, int *d_pos,
                                 int *h_num_matched, int hashed);

/* Flow sets (no reference counterpart; include/pfac_ext.h: PFACX_flows*), scan_flows.hip: the seams of many streams in one launch and
 * the merge of their pairs with the pairs of ONE compacted scan over the whole buffer.  A piece is described on the host:
 * its bytes are d_input[start, start + len), its flow's carry is buffer `cur` of flow `flow` (buffer b of flow f lies at
 * d_carries + (2 f + b) * carryStride) and holds `carried` bytes, of which the first numFinal start positions become final with this
 * piece; the launch stages their (id, position - carried) pairs at d_seamIds / d_seamPos + seamOff (numFinal entries of room) and
 * writes the flow's next carry, the last min(maxPatternLen - 1, carried + len) bytes of [carry | piece], into the flow's OTHER buffer.
 * d_scanIds / d_scanPos: the scanCount ordered pairs of the compacted scan over d_input as one buffer (a copy: d_ids / d_pos are
 * written); of piece k those at [start, start + len - (maxPatternLen - 1)) count.  Output: the pairs of piece k -- seam, then scan,
 * positions relative to `start` -- at [d_pieceFirst[k], d_pieceFirst[k + 1]) of d_ids / d_pos; nothing at or beyond `capacity` or
 * the total.  d_stage: numPieces * stageStride bytes where 2 (maxPatternLen - 1) bytes do not fit the LDS, else null.  The
 * unsigned arrays hold numPieces entries (d_blockSums: one per 256 pieces, + 2).  Synchronous: *h_total = the number of pairs. */
typedef struct {
    unsigned int start, len, flow, carried, numFinal, seamOff, cur, reserved;
} PFACX_flowPiece_t;
typedef struct {
    const char *d_input;
    const PFACX_flowPiece_t *d_pieces;
    size_t numPieces;
    char *d_carries;
    size_t carryStride;
    char *d_stage;
    size_t stageStride;
    int *d_seamIds, *d_seamPos;
    unsigned int *d_seamCount, *d_pairLo, *d_counts, *d_blockSums;
    const int *d_scanIds, *d_scanPos;
    size_t scanCount;
    int *d_ids, *d_pos;
    size_t capacity;
    int *d_pieceFirst;
} PFACX_flowsRun_t;
PFAC_status_t PFACX_flowsRun(PFAC_handle_t handle, const PFACX_flowsRun_t *run, int *h_total);

/* Lines (no reference counterpart; include/pfac_ext.h: PFACX_matchLines* / PFACX_gatherLines*), scan_lines.hip.
 * PFACX_linesSelect: the lines of d_input[0, size) -- 0 < size < 2^31 -- that contain a match (invert != 0: that contain none).  d_scan is what the
 * compacted scan reads: d_input, or its folded copy for a caseless set; the newline bitmap is made from d_input.  The scan (PFAC_reduce_kernel, hashed
 * != 0: PFAC_reduce_inplace_kernel, with its pairs left unordered) uses d_lineStart / d_lineLen (`size` entries at least) as its pair list; the
 * select pass then overwrites them -- and d_lineIndex unless null -- with the selected lines in ascending order.  Synchronous.
 * PFACX_linesGather: the text of numSelected lines (start, len) of d_input, each clamped to [0, size], a '\n' behind every line, into d_out; nothing is
 * written at or beyond outCapacity; *h_outBytes = the size of the whole text.  Synchronous. */
PFAC_status_t PFACX_linesSelect(PFAC_handle_t handle, const char *d_input, char *d_scan, size_t size, int invert, int hashed, int *d_lineStart,
                                int *d_lineLen, int *d_lineIndex, size_t *h_numLines, size_t *h_numSelected);
PFAC_status_t PFACX_linesGather(PFAC_handle_t handle, const char *d_input, size_t size, const int *d_lineStart, const int *d_lineLen,
                                size_t numSelected, char *d_out, size_t outCapacity, size_t *h_outBytes);
/* PFACX_linesSelectContext (include/pfac_ext.h: PFACX_matchLinesContext*): PFACX_linesSelect with the lines up to `before` in front of and `after`
 * behind each line that call would select.  The same launches with the context stage between the marks and the select passes: the hit bitmap
 * becomes that of the lines the plain call selects, is widened by line number, and the select passes run over the widened bitmap; d_lineTag (unless
 * null) gets group << 1 | (the line is one the plain call selects).  *h_numMatching = the lines the plain call selects, *h_numGroups = the runs of
 * consecutive selected lines.  Scratch of the stage: the handle's context scratch (scan_lines.hip has the formula).  Synchronous. */
PFAC_status_t PFACX_linesSelectContext(PFAC_handle_t handle, const char *d_input, char *d_scan, size_t size, int invert, int hashed,
                                       unsigned int before, unsigned int after, int *d_lineStart, int *d_lineLen, int *d_lineIndex, int *d_lineTag,
                                       size_t *h_numLines, size_t *h_numSelected, size_t *h_numMatching, size_t *h_numGroups);

/* Measurement only: the newline pass of PFACX_linesSelect alone (pfac_lines_bitmap: one read of the input, size / 8 + size / 8 + size / 16 bytes written
 * into the handle's lines scratch).  Returns the average milliseconds of `launches` launches over the first n < 2^31 bytes of d_in, or a negative
 * value on an error.  tools/lines_sweep.py reports it next to the fold kernel's rate. */
double PFACX_linesBitmapProbe(PFAC_handle_t handle, const void *d_in, size_t n, int launches);

/* Test only: the four ordering launches of a compacted-output call (scan_order.inc) alone, on a caller's pairs.  Orders (d_ids[k], d_pos[k]), k < count,
 * in place by ascending position, with the bin layout and through the scratch of a call over an input of n bytes -- 0 < n < 2^31, count <= n -- on a
 * handle of PFAC_create: the sequence of PFAC_reduce_kernel's second round (more pairs than the scratch held), which grows the handle's ordering
 * scratch to `count` pairs where it holds fewer.  The arrays hold `count` entries and nothing beyond them is written.  The positions must be DISTINCT
 * and below n: the kernels trust them as they trust the scan's, and a list that breaks this has them write outside the arrays.  Synchronous; the
 * handle's next compacted-output call clears its counters itself.  count == 0 succeeds and launches nothing; PFAC_STATUS_INVALID_PARAMETER for n == 0,
 * n >= 2^31, count > n, or a null array with count > 0.  tests/test_order_edges_gpu.py runs every bin width and bin edge through it. */
PFAC_status_t PFACX_orderPairsProbe(PFAC_handle_t handle, int *d_ids, int *d_pos, size_t count, size_t n);

/* Covered spans and redaction (no reference counterpart; include/pfac_ext.h: PFACX_matchSpans* / PFACX_redactSpansFromDevice), scan_spans.hip.
 * PFACX_spansSelect: the maximal runs of bytes of d_scan[0, size) -- 0 < size < 2^31; the caller's bytes, or their folded copy for a caseless set --
 * that belong to a match.  The scan (PFAC_reduce_kernel, hashed != 0: PFAC_reduce_inplace_kernel, WITH its ordering launches) uses d_spanStart /
 * d_spanLen (`size` entries at least) as its pair list; the passes behind it work on the pairs alone, through d_patternLen (the pattern lengths by id,
 * numIds entries) and the handle's spans scratch, and then overwrite the arrays with the spans in ascending order.  Synchronous: *h_numSpans, and
 * *h_coveredBytes = the sum of the lengths.
 * PFACX_spansRedact: d_out[b] = fill where b lies in one of the numSpans spans (start, len) -- each clamped to [0, size] --, d_input[b] elsewhere;
 * d_out == d_input (then only covered bytes are written) or ranges that do not overlap, any alignment of either.  Asynchronous, on the default stream. */
PFAC_status_t PFACX_spansSelect(PFAC_handle_t handle, char *d_scan, size_t size, int hashed, const int *d_patternLen, size_t numIds, int *d_spanStart,
                                int *d_spanLen, size_t *h_numSpans, size_t *h_coveredBytes);
PFAC_status_t PFACX_spansRedact(PFAC_handle_t handle, const char *d_input, size_t size, const int *d_spanStart, const int *d_spanLen, size_t numSpans,
                                unsigned char fill, char *d_out);

/* Occurrence counts (no reference counterpart; include/pfac_ext.h: PFACX_count*), scan_count.hip.
 * PFACX_countPairs: d_counts[id] (numIds + 1 entries, 64-bit) = how often pattern id occurs, from a list of LONGEST pairs.  d_scan != null: the list is
 * made here -- the compacted scan of d_scan[0, size), 0 < size < 2^31 (PFAC_reduce_kernel, hashed != 0: PFAC_reduce_inplace_kernel, pairs left
 * unordered) into the handle's pair scratch (pfac::DeviceScratch::allPairs) -- and d_ids / numPairs are not read; d_scan == null: the list is
 * d_ids[0, numPairs), numPairs < 2^31, any 4-byte alignment, an id outside [1, numIds] ignored.  d_table (pfac::Int2 {prefixPattern, chainLen} by id,
 * or null): every pair also counts for the patterns on its prefix chain; null: the longest histogram alone.  flags: PFACX_COUNT_ACCUMULATE adds to
 * d_counts[1, numIds] and leaves entry 0 alone, else entries [0, numIds] are overwritten.  h_total (or null): what the call added -- chainLen per
 * pair with a table, else 1; given, the call is synchronous, else asynchronous on the default stream.
 * PFACX_countNonzero: (i, d_counts[i]) for every non-zero entry of d_counts[0, numCounts), 0 < numCounts < 2^31, ascending, into d_ids / d_outCounts;
 * nothing at or beyond `capacity`; *h_numDistinct and *h_total (the sum of all entries) are the full values.  Synchronous. */
PFAC_status_t PFACX_countPairs(PFAC_handle_t handle, char *d_scan, size_t size, int hashed, const int *d_ids, size_t numPairs, const void *d_table,
                               unsigned int flags, unsigned long long *d_counts, size_t *h_total);
PFAC_status_t PFACX_countNonzero(PFAC_handle_t handle, const unsigned long long *d_counts, size_t numCounts, int *d_ids,
                                 unsigned long long *d_outCounts, size_t capacity, size_t *h_numDistinct, unsigned long long *h_total);

/* Disjoint matches and their replacement (no reference counterpart; include/pfac_ext.h: PFACX_matchDisjoint* / PFACX_replace*), scan_disjoint.hip.
 * PFACX_disjointSelect: the disjoint leftmost-longest list of d_scan[0, size) -- 0 < size < 2^31; the caller's bytes, or their folded copy for a
 * caseless set.  The scan (PFAC_reduce_kernel, hashed != 0: PFAC_reduce_inplace_kernel, WITH its ordering launches) uses d_ids / d_pos (`size` entries
 * at least) as its pair list; the passes behind it work on the pairs alone, through d_patternLen (the pattern lengths by id, numIds entries) and the
 * handle's disjoint scratch, and then overwrite the arrays with the tokens in ascending order.  Synchronous: *h_numTokens, and *h_coveredBytes = the sum
 * of the lengths.
 * PFACX_replaceRun: the text of d_input[0, size), 0 < size < 2^31, with each of the numTokens tokens (d_ids[k], d_pos[k]), 0 < numTokens < 2^31,
 * replaced by d_replBytes[d_replOff[id], d_replOff[id + 1]) into d_out; every start is clamped to [0, size], every length is d_patternLen[id] clipped
 * to the buffer, every offset clamped to [0, replBytes], an id outside [1, min(numIds, numOff - 1)) a token that does nothing.  Nothing is written
 * at or beyond outCapacity; *h_outBytes = the size of the whole text (more than outCapacity: PFACX_STATUS_OUTPUT_TRUNCATED).  d_out must not overlap
 * d_input (the caller checks).  Synchronous. */
PFAC_status_t PFACX_disjointSelect(PFAC_handle_t handle, char *d_scan, size_t size, int hashed, const int *d_patternLen, size_t numIds, int *d_ids,
                                   int *d_pos, size_t *h_numTokens, size_t *h_coveredBytes);
PFAC_status_t PFACX_replaceRun(PFAC_handle_t handle, const char *d_input, size_t size, const int *d_ids, const int *d_pos, size_t numTokens,
                               const int *d_patternLen, size_t numIds, const int *d_replOff, size_t numOff, const char *d_replBytes, size_t replBytes,
                               char *d_out, size_t outCapacity, size_t *h_outBytes);

/* Rule sets (no reference counterpart; include/pfac_ext.h: PFACX_rules*), scan_rules.hip.
 * PFACX_rulesRun: the fired (segment, rule) list of a batch from its ordered LONGEST pairs.  d_pairIds[0, count), count < 2^31, are the ids of the
 * ordered compacted batch scan (in the handle's pair scratch); d_segFirstPairs (numSegments + 1 ints: the first pair of each segment, as
 * PFACX_batchReduceFixup leaves them, clamped to [0, count] where read, a decreasing pair an empty segment), or null: one segment of all pairs.
 * d_table: pfac::Int2 {prefixPattern, chainLen} by id, numIds + 1 entries.  The rule set: d_memberOff[numIds + 2], the memberships of pattern id
 * at d_member[d_memberOff[id], d_memberOff[id + 1]) as rule << 5 | bit, ascending rule; d_need[numRules], the full mask of each rule; 0 < numRules <
 * 2^24.  Output: the pairs in ascending (segment, rule) order into d_firedSeg / d_firedRule, nothing at or beyond `capacity` (0: both may be null);
 * d_segFirst (numSegments + 1 size_t, or null) indexes the whole list; *h_total = its full length.  0 < numSegments < 2^31.  Synchronous.
 * A CONDITIONED set (PFACX_rulesOpenEx) gives d_memberCond, indexed like d_member: {lo, hi} per membership -- lo the window's offset, hi bits 0 .. 30
 * its end offset + depth saturated to 2^31 - 1 (no upper bound: 2^31 - 1), bit 31 PFACX_RULE_FROM_END -- and with it d_pairPos[0, count), the pairs'
 * positions in the buffer, d_patternLen (the pattern lengths by id, numIds + 1 entries), `size` and d_offsets (numSegments + 1 size_t, clamped to
 * [0, size] where read; null: one segment [0, size)).  A membership's bit is set only by an occurrence that lies inside its segment and satisfies the
 * window; d_need holds the positive bits only.  d_memberCond == null: a plain set, none of the five is read.
 * A set WITH CHAINS (PFACX_rulesOpenSeq with a PFACX_RULE_RELATIVE member; conditioned as well) gives d_seqOff[numRules + 1] and d_seqLink, five
 * words per link: the links of rule r at d_seqLink[5 d_seqOff[r], 5 d_seqOff[r + 1]), chain by chain in rule order, as {pattern id | bit 31 on the
 * first link of a chain, lo, hi as in d_memberCond, distance, within (0: no upper bound)}.  A rule with mask == need and links fires only if every
 * chain holds; the call then takes 2 x round256(4 count) bytes more of the handle's rules scratch for its two frontier arrays.  Both null: no rule
 * has a chain, and the launches are those of a conditioned set. */
typedef struct {
    const int *d_pairIds;
    size_t count;
    const int *d_segFirstPairs;
    size_t numSegments;
    const void *d_table;
    size_t numIds;
    const int *d_memberOff;
    const unsigned int *d_member, *d_need;
    size_t numRules;
    int *d_firedSeg, *d_firedRule;
    size_t capacity;
    size_t *d_segFirst;
    const int *d_pairPos;
    const size_t *d_offsets;
    size_t size;
    const int *d_patternLen;
    const unsigned int *d_memberCond;
    const int *d_seqOff;
    const unsigned int *d_seqLink;
} PFACX_rulesRun_t;
PFAC_status_t PFACX_rulesRun(PFAC_handle_t handle, const PFACX_rulesRun_t *run, size_t *h_total);

/* Whole-word and delimiter-bounded matches (no reference counterpart; include/pfac_ext.h: PFACX_matchWords* / PFACX_wordsPairsFromDevice), scan_words.hip.
 * PFACX_wordsRun: the bounded occurrences of an ordered list of LONGEST pairs.  d_input[0, size), 0 < size < 2^31, are the CALLER's bytes (never the
 * folded copy of a caseless set: the class is tested on them); d_pairIds / d_pairPos[0, count), count < 2^31: one pair per position, ascending -- the
 * handle's pair scratch behind PFACX_allReduce, or a caller's list: an id outside [1, numIds] or a position outside [0, size) is a pair that gives
 * nothing, a chain member that does not lie inside the input is not kept.  d_table: pfac::Int2 {prefixPattern, chainLen} by id, numIds + 1 entries, or
 * null: every chain is the pair itself; d_patternLen: the pattern lengths by id, numIds + 1 entries.  cls: the class, bit b & 31 of cls[b >> 5] for
 * byte b.  all == 0: per pair the longest bounded member of its chain; else every bounded member, longest first.  Output: (id, position) into d_ids /
 * d_pos, nothing at or beyond `capacity` (0: both may be null, and nothing is written); *h_total = the full length of the list.  The output arrays must
 * not overlap the pair arrays (the caller checks).  Synchronous. */
typedef struct {
    const char *d_input;
    size_t size;
    const int *d_pairIds, *d_pairPos;
    size_t count;
    const void *d_table;
    const int *d_patternLen;
    size_t numIds;
    unsigned int cls[8];
    unsigned int all;
    int *d_ids, *d_pos;
    size_t capacity;
} PFACX_wordsRun_t;
PFAC_status_t PFACX_wordsRun(PFAC_handle_t handle, const PFACX_wordsRun_t *run, size_t *h_total);

/* Per-segment occurrence counts (no reference counterpart; include/pfac_ext.h: PFACX_countBatch*), scan_segcount.hip.
 * PFACX_segCountRun: the (id, count) list of a batch in CSR form from its ordered LONGEST pairs.  d_pairIds[0, count), count < 2^31, any 4-byte
 * alignment: the ids of the ordered compacted batch scan (in the handle's pair scratch) or a caller's list, an id outside [1, numIds] ignored;
 * d_segFirstPairs (numSegments + 1 ints: the first pair of each segment, as PFACX_batchReduceFixup leaves them, clamped to [0, count] where read, a
 * decreasing pair an empty segment), or null: one segment of all pairs.  d_table: pfac::Int2 {prefixPattern, chainLen} by id, numIds + 1 entries
 * -- every pair also counts for the patterns on its prefix chain --, or null: one count per pair, the table is never read.  Output: the entries with
 * a non-zero count in ascending (segment, id) order into d_ids / d_counts, nothing at or beyond `capacity` (0: both may be null); d_segFirst
 * (numSegments + 1 size_t, required) indexes the whole list; *h_numEntries = its full length, *h_total = the sum of all counts.  0 < numSegments <
 * 2^31.  A segment is one block's work.  Synchronous. */
typedef struct {
    const int *d_pairIds;
    size_t count;
    const int *d_segFirstPairs;
    size_t numSegments;
    const void *d_table;
    size_t numIds;
    int *d_ids;
    unsigned int *d_counts;
    size_t capacity;
    size_t *d_segFirst;
} PFACX_segCountRun_t;
PFAC_status_t PFACX_segCountRun(PFAC_handle_t handle, const PFACX_segCountRun_t *run, size_t *h_numEntries, unsigned long long *h_total);

/* Pattern groups (no reference counterpart; include/pfac_ext.h: PFACX_groups*), scan_groups.hip.
 * PFACX_groupsRun: the group list of a batch from its ordered LONGEST pairs.  d_pairIds / d_pairPos[0, count), count < 2^31: one pair per position,
 * ordered by segment -- the handle's pair scratch behind the ordered compacted batch scan, or a caller's list: an id outside [1, numIds] is a pair
 * that gives nothing, a position is copied through and never used as an index.  d_segFirstPairs (numSegments + 1 ints: the first pair of each
 * segment, clamped to [0, count] and raised to the largest entry in front of it where it is read: a decreasing pair is an empty segment, pairs
 * before the first or behind the last bound belong to no segment), or null with numSegments == 1: one segment of all pairs.  d_segMasks: numSegments
 * 64-bit masks, or null: all bits set.  d_patternMasks: numIds + 1 64-bit masks by id.  d_table: pfac::Int2 {prefixPattern, chainLen} by id,
 * numIds + 1 entries, or null: every chain is the pair itself.  all == 0: per pair the longest member of its chain whose mask meets the segment's;
 * else every such member, longest first.  Output: (id, position) into d_ids / d_pos, nothing at or beyond `capacity` (0: both may be null);
 * d_segFirst (numSegments + 1 size_t, or null) indexes the whole list; d_segGroups (numSegments 64-bit words, or null): the OR of mask & segment
 * mask over every member of every chain of the segment, whatever `all` and `capacity`; *h_total = the full length of the list.  The output arrays
 * must not overlap the pair arrays (the caller checks).  0 < numSegments < 2^31.  Synchronous. */
typedef struct {
    const int *d_pairIds, *d_pairPos;
    size_t count;
    const int *d_segFirstPairs;
    size_t numSegments;
    const unsigned long long *d_segMasks;
    const unsigned long long *d_patternMasks;
    const void *d_table;
    size_t numIds;
    unsigned int all;
    int *d_ids, *d_pos;
    size_t capacity;
    size_t *d_segFirst;
    unsigned long long *d_segGroups;
} PFACX_groupsRun_t;
PFAC_status_t PFACX_groupsRun(PFAC_handle_t handle, const PFACX_groupsRun_t *run, size_t *h_total);

/* Flow-rule sets (no reference counterpart; include/pfac_ext.h: PFACX_flowRules*), scan_flowrules.hip.
 * PFACX_flowRulesRun: the fired (piece, rule) list of one flows call from its LONGEST pairs, against the patterns each flow has seen so far.
 * d_pairIds[0, count), count < 2^31: the ids of a flows call or flush (the caller's array, never written; an id outside [1, numIds] ignored);
 * d_pieceFirst (numPieces + 1 ints: the first pair of each piece, clamped to [0, count] where read, a decreasing pair an empty piece);
 * h_flowIds[numPieces], HOST memory: the flow of each piece, every one below numFlows and no two equal (the caller has validated them; the call
 * uploads them into its scratch).
 * d_table: pfac::Int2 {prefixPattern, chainLen} by id, numIds + 1 entries.  The set: d_memberOff[numIds + 2] and d_member (rule << 5 | bit,
 * ascending rule) as PFACX_rulesRun takes them; d_ruleFirst[numRules + 1]: rule r has d_ruleFirst[r + 1] - d_ruleFirst[r] members, 1 to 32, its
 * full mask that many low bits, and member b of it is bit d_ruleBits[d_ruleFirst[r] + b] of a flow's bitmap; d_bitOf[numIds + 1]: the bit of
 * pattern id in a flow's bitmap, -1 for a pattern no rule names; d_flowBits: numFlows x wordsPerFlow words, flow f at d_flowBits + f *
 * wordsPerFlow, bit set: the pattern has occurred in the flow.  0 < numRules < 2^24.
 * Rule r fires on piece k iff the piece's pairs complete it: (old | new) == full mask and old != full mask, old from the flow's bitmap.  Output:
 * the pairs in ascending (piece, rule) order into d_firedPiece / d_firedRule, nothing at or beyond `capacity` (0: both may be null);
 * d_pieceFiredFirst (numPieces + 1 size_t, or null) indexes the whole list; *h_total = its full length.  Only where *h_total <= capacity does
 * the call then OR the bits of the pieces' pairs into their flows' bitmaps (pfac_flowrules_commit): a longer list leaves d_flowBits as it was.
 * 0 < numPieces < 2^31.  Synchronous. */
typedef struct {
    const int *d_pairIds;
    size_t count;
    const int *d_pieceFirst;
    const unsigned int *h_flowIds;
    size_t numPieces;
    const void *d_table;
    size_t numIds;
    const int *d_memberOff;
    const unsigned int *d_member;
    const int *d_ruleFirst;
    const unsigned int *d_ruleBits;
    const int *d_bitOf;
    size_t numRules;
    unsigned int *d_flowBits;
    size_t numFlows, wordsPerFlow;
    int *d_firedPiece, *d_firedRule;
    size_t capacity;
    size_t *d_pieceFiredFirst;
} PFACX_flowRulesRun_t;
PFAC_status_t PFACX_flowRulesRun(PFAC_handle_t handle, const PFACX_flowRulesRun_t *run, size_t *h_total);

/* Split (no reference counterpart; include/pfac_ext.h: PFACX_split*), scan_split.hip.
 * PFACX_splitRun: the offsets that cut d_input[0, size), size > 0 and any size that has fewer than 2^31 tiles of 16 KiB, at the bytes of the class
 * cls (bit b & 31 of cls[b >> 5] for byte b; the caller's bytes are tested as they are and never written): 0, the cuts of pfac_ext.h's definition
 * under `flags` (PFACX_SPLIT_BEFORE, PFACX_SPLIT_RUNS) ascending, `size`, as 64-bit values into d_offsets -- entries [0, capacity) of them, nothing at
 * or beyond `capacity` (0: the array may be null, nothing is written).  *h_numSegments = the cuts + 1 and *h_longest (or null) = the longest segment
 * in bytes are the full values whatever the capacity.  Two reads of the input; scratch: the handle's split scratch, sized by the tiles alone
 * (scan_split.hip has the formula).  Synchronous. */
typedef struct {
    const char *d_input;
    size_t size;
    unsigned int cls[8];
    unsigned int flags;
    size_t *d_offsets;
    size_t capacity;
} PFACX_splitRun_t;
PFAC_status_t PFACX_splitRun(PFAC_handle_t handle, const PFACX_splitRun_t *run, size_t *h_numSegments, size_t *h_longest);

/* Locate (no reference counterpart; include/pfac_ext.h: PFACX_locate*), scan_locate.hip.
 * PFACX_locateRun: for the positions d_pos[0, numPairs) (non-decreasing; 0 <= numPairs < 2^31) in d_input[0, size), 0 < size < 2^31, the record
 * and the column by the cuts that PFACX_splitRun makes of the same class and flags: d_record[i] = the number of cuts <= d_pos[i], d_column[i]
 * (the array may be null) = d_pos[i] - the largest such cut (0: none); both -1 for a position outside [0, size).  *h_numRecords = the cuts + 1.
 * numPairs == 0: only the count, no array is touched.  The list is never trusted: a list that is not non-decreasing gets unspecified values and
 * no access outside the input, the list and the outputs' numPairs entries.  One read of the input and a second of the tiles of 16 KiB that hold
 * a position; scratch: the handle's locate scratch, sized by the tiles alone (scan_locate.hip has the formula).  Synchronous. */
typedef struct {
    const char *d_input;
    size_t size;
    unsigned int cls[8];
    unsigned int flags;
    const int *d_pos;
    size_t numPairs;
    int *d_record;
    int *d_column;
} PFACX_locateRun_t;
PFAC_status_t PFACX_locateRun(PFAC_handle_t handle, const PFACX_locateRun_t *run, size_t *h_numRecords);

/* Capture (no reference counterpart; include/pfac_ext.h: PFACX_capture*), scan_capture.hip.
 * PFACX_captureRun: for the pairs (d_ids[i], d_pos[i]), i < numPairs (positions non-decreasing; 0 < numPairs < 2^31) in d_input[0, size),
 * 0 < size < 2^31, the value behind the match by the six rules of the header: b = the position + d_patternLen[id] (PFACX_CAPTURE_AT_POS: the
 * position itself; d_ids and d_patternLen may then be null), never beyond size; w = size, or min(size, b + window) for window != 0; d_valStart[i]
 * = the first position of [b, w) whose byte is not in `skip`, d_valStart[i] + d_valLen[i] = the first position from there on whose byte is in
 * `stop`; w where there is none.  (-1, 0) for a position outside [0, size) and, without the flag, for an id outside [1, numLens - 1].  `skip` is
 * S \ D already: the caller takes the stop bytes out of it.  d_patternLen: numLens = F + 1 lengths by id (the handle's device copy).
 * *h_slowPairs = the pairs that left the bitmap of their tile and finished on the input itself.  The list is never trusted: a list that is not
 * non-decreasing gets unspecified values and no access outside the input, the list, the lengths and the outputs' numPairs entries.  Only tiles of
 * 16 KiB that hold a position are read; scratch: the handle's capture scratch, sized by the tiles alone (scan_capture.hip has the formula).
 * Synchronous. */
#define PFACX_CAPTURE_REACH 1024u      /* bytes behind a tile that its bitmap covers (scan_capture.hip: kCaptureReach; pfac_amd/api.py) */
typedef struct {
    const char *d_input;
    size_t size;
    unsigned int skip[8];
    unsigned int stop[8];
    size_t window;
    unsigned int flags;
    const int *d_ids;
    const int *d_pos;
    size_t numPairs;
    const int *d_patternLen;
    size_t numLens;
    int *d_valStart;
    int *d_valLen;
} PFACX_captureRun_t;
PFAC_status_t PFACX_captureRun(PFAC_handle_t handle, const PFACX_captureRun_t *run, size_t *h_slowPairs);

/* The six verify runs below (PFACX_caseRun ... PFACX_clsigRun) start with the same fields: the first member of each run struct, filled by one host
 * function (pfac_amd/csrc/verify_calls.h: fillRunFrame) and checked and turned into the expansion frame by one function of the module
 * (pfac_amd/csrc/scan_verify.h: verifyRunOk, verifyFrame).  The text of each run says what they mean there. */
typedef struct {
    const char *d_input;
    size_t size;
    const int *d_pairIds, *d_pairPos;
    size_t count;
    const void *d_table;
    size_t numIds;
    const unsigned int *d_blob;
    size_t blobWords;
    int *d_ids, *d_pos;
    size_t capacity;
} PFACX_verifyRun_t;

/* Per-pattern case sensitivity over a caseless set (no reference counterpart; include/pfac_ext.h: PFACX_case*), scan_case.hip.
 * PFACX_caseRun: the cased occurrences of an ordered list of LONGEST pairs of a caseless set.  d_input[0, size), 0 < size < 2^31, are the CALLER's
 * bytes at any alignment (never the folded copy: the sensitive patterns are compared with them, and no load leaves [0, size)); d_pairIds /
 * d_pairPos[0, count), count < 2^31: one pair per position, ascending -- the handle's pair scratch behind PFACX_allReduce, or a caller's list: an
 * id outside [1, numIds] or a position outside [0, size) is a pair that gives nothing, a chain member that does not lie inside the input is not
 * kept.  d_table: pfac::Int2 {prefixPattern, chainLen} by id, numIds + 1 entries, or null: every chain is the pair itself; d_patternLen: the
 * pattern lengths by id, numIds + 1 entries.  The variants of automaton id q are d_vars[d_varOff[q] & 0x7FFFFFFF, d_varOff[q + 1] & 0x7FFFFFFF)
 * (d_varOff: numIds + 2 entries), pfac::Int2 {line id, dword index of the pattern's original bytes in d_blob; -1: a caseless variant}, by line id
 * descending; bit 31 of d_varOff[q]: the class is one caseless variant, reported as q without a look at the tables or the input.  d_blob: blobWords
 * dwords, every pattern padded to a multiple of 4 bytes.  all == 0: per pair the first variant that holds, longest member first; else every
 * variant that holds.  Output: (line id, position) into d_ids / d_pos, nothing at or beyond `capacity` (0: both may be null); *h_total = the full
 * length of the list.  The output arrays must not overlap the pair arrays (the caller checks).  Synchronous. */
typedef struct {
    PFACX_verifyRun_t v;            /* the input, the pairs, the chain table, the blob, the caller's arrays */
    const int *d_patternLen;
    const unsigned int *d_varOff;
    const void *d_vars;
    size_t numVars;
    unsigned int all;
} PFACX_caseRun_t;
PFAC_status_t PFACX_caseRun(PFAC_handle_t handle, const PFACX_caseRun_t *run, size_t *h_total);

/* Masked byte signatures (no reference counterpart; include/pfac_ext.h: PFACX_sig*), scan_sig.hip.
 * PFACX_sigRun: the signatures that occur around an ordered list of LONGEST pairs of the anchor set.  d_input[0, size), 0 < size < 2^31, are the
 * caller's bytes at any alignment (no load leaves [0, size)); d_pairIds / d_pairPos[0, count), count < 2^31: one pair per position, ascending --
 * the handle's pair scratch behind PFACX_allReduce, or a caller's list: an id outside [1, numIds] or a position outside [0, size) is a pair that
 * gives nothing.  d_table: pfac::Int2 {prefixPattern, chainLen} by id, numIds + 1 entries, or null: every chain is the pair itself.  The
 * signatures anchored by pattern q are d_sigs[d_sigOff[q], d_sigOff[q + 1]) (d_sigOff: numIds + 2 entries; the range is clamped to numSigs), four
 * ints each: {signature id, offset of the anchor in the signature, length of the signature, dword index of its bytes in d_blob}, by signature id
 * descending.  d_blob, blobWords dwords: per signature (len + 3) / 4 value dwords, then as many mask dwords, values already ANDed with their
 * masks, the bytes behind len with mask 0; an entry whose dwords do not lie inside the blob is skipped.  A signature of a chain member at pair
 * position p starts at s = p - offset; it is kept iff 0 <= s, s + len <= size and (in[s + k] ^ value[k]) & mask[k] == 0 for every k.
 * Output: (signature id, s) into d_ids / d_pos in pair order, chain order, table order; nothing at or beyond `capacity` (0: both may be null);
 * *h_total = the full length of the list.  The output arrays must not overlap the pair arrays (the caller checks).  Synchronous. */
typedef struct {
    PFACX_verifyRun_t v;            /* the input, the pairs, the chain table, the blob, the caller's arrays */
    const unsigned int *d_sigOff;
    const void *d_sigs;
    size_t numSigs;
} PFACX_sigRun_t;
PFAC_status_t PFACX_sigRun(PFAC_handle_t handle, const PFACX_sigRun_t *run, size_t *h_total);

/* Patterns matched within k mismatches (no reference counterpart; include/pfac_ext.h: PFACX_approx*), scan_approx.hip.
 * PFACX_approxRun: the patterns that occur within their budgets around an ordered list of LONGEST pairs of the piece set.  d_input, size, the pair
 * arrays, count, d_table and numIds are those of PFACX_sigRun.  The (pattern, piece) entries of piece string q are d_entries[d_entryOff[q],
 * d_entryOff[q + 1]) (d_entryOff: numIds + 2 entries; the range is clamped to numEntries), 16 bytes each (pfac_context.h: ApproxEntry): {pattern
 * id, dword index of the pattern's bytes in d_blob, start of the piece in the pattern | length L of the pattern << 16, budget k | piece index j
 * << 8}, by pattern id descending, then piece index descending.  d_blob, blobWords dwords: per pattern (L + 3) / 4 dwords of its bytes; an entry
 * whose dwords do not lie inside the blob, or with k > 7, j > k or L < k + 1, is skipped; the start is j L / (k + 1).  maxPieceLen >= 1: the
 * piece of part j' of a pattern is the first min(part length, maxPieceLen) bytes at j' L / (k + 1).  An entry of a chain member at pair position p
 * starts at s = p - start; it is kept iff 0 <= s, s + L <= size, d = #{t : in[s + t] != pattern[t]} <= k and no piece j' < j of the pattern equals
 * the input at s + j' L / (k + 1): every occurrence once, by its lowest exact piece.
 * Output: (pattern id, s) into d_ids / d_pos and d into d_mis (may be null) in pair order, chain order, table order; nothing at or beyond
 * `capacity` (0: all three may be null); *h_total = the full length of the list.  The output arrays must not overlap the pair arrays (the caller
 * checks).  Synchronous. */
typedef struct {
    PFACX_verifyRun_t v;            /* the input, the pairs, the chain table, the blob, the caller's arrays */
    const unsigned int *d_entryOff;
    const void *d_entries;
    size_t numEntries;
    size_t maxPieceLen;
    int *d_mis;
} PFACX_approxRun_t;
PFAC_status_t PFACX_approxRun(PFAC_handle_t handle, const PFACX_approxRun_t *run, size_t *h_total);

/* Signatures with bounded gaps between parts (no reference counterpart; include/pfac_ext.h: PFACX_gapsig*), scan_gapsig.hip.
 * PFACX_gapsigRun: the gapped signatures that occur around an ordered list of LONGEST pairs of the anchor set.  d_input, size, the pair arrays,
 * count, d_table and numIds are those of PFACX_sigRun.  The signatures anchored by pattern q are d_sigs[d_sigOff[q], d_sigOff[q + 1]) (d_sigOff:
 * numIds + 2 entries; the range is clamped to numSigs), 16 bytes each (pfac_context.h: GapSigEntry): {signature id, first part, number of parts |
 * anchor part << 16, offset of the anchor inside that part}, by signature id descending.  d_parts, numParts entries of 16 bytes (GapSigPart):
 * {len, dword index of its bytes in d_blob, lo, hi}, the gap behind the part.  d_blob, blobWords dwords: per part (len + 3) / 4 value dwords, then
 * as many mask dwords, values already ANDed with their masks, the bytes behind len with mask 0.  An entry with no part or more than 64, parts
 * outside the table or an anchor part outside the entry is skipped; so is, wherever it is met, a part that is empty, has hi < lo or hi - lo > 63,
 * or whose dwords do not lie inside the blob: nothing lies there.  Only each gap is tested, not the sum over a signature: where a table's slack
 * exceeds 63 the distances past bit 63 are dropped without a word -- fewer entries, nothing out of bounds; the library's own tables never do.  Part a of a chain member at pair position p lies at x = p - offset; (id, s,
 * end) is kept iff an embedding of the signature at s has part a at x, no embedding at s has it at a smaller offset (every occurrence once, by
 * the smallest offset of its anchor part), and end is the smallest end over all embeddings at s (include/pfac_ext.h says what an embedding is).
 * Output: (signature id, s) into d_ids / d_pos and end into d_end (may be null) in pair order, chain order, table order, s ascending; nothing at
 * or beyond `capacity` (0: all three may be null); *h_total = the full length of the list.  The output arrays must not overlap the pair arrays
 * (the caller checks).  Synchronous. */
typedef struct {
    PFACX_verifyRun_t v;            /* the input, the pairs, the chain table, the blob, the caller's arrays */
    const unsigned int *d_sigOff;
    const void *d_sigs;
    size_t numSigs;
    const void *d_parts;
    size_t numParts;
    int *d_end;
} PFACX_gapsigRun_t;
PFAC_status_t PFACX_gapsigRun(PFAC_handle_t handle, const PFACX_gapsigRun_t *run, size_t *h_total);

/* Patterns matched within k edits (no reference counterpart; include/pfac_ext.h: PFACX_edit*), scan_edit.hip.
 * PFACX_editRun: the ends at which the patterns occur within their budgets around an ordered list of LONGEST pairs of the piece set.  d_input,
 * size, the pair arrays, count, d_table and numIds are those of PFACX_sigRun; d_entryOff, d_entries (pfac_context.h: EditEntry), numEntries,
 * d_blob, blobWords and maxPieceLen those of PFACX_approxRun.  maxBudget, 0 .. 7, is the largest k of the table: it selects the instantiation of
 * the passes (k <= 1, k <= 3, k <= 7), and an entry with k > maxBudget, j > k or L <= k, or whose dwords leave the blob, is skipped.  bestEnds:
 * the three-point rule of PFACX_EDIT_BEST_ENDS.  An entry of a chain member at pair position p is the candidate with the diagonal d0 = p - start;
 * it is verified by the banded dynamic program of DESIGN.md 5y and lists the ends e with |e - L - d0| <= k, 0 <= e <= size, at which the pattern
 * occurs (and which pass the three-point rule where bestEnds) and which no candidate with a smaller piece index, or the same piece at a smaller
 * position, covers: every occurrence once.
 * Output: (pattern id, start) into d_ids / d_pos, the end into d_end and the distance into d_dist (each may be null) in pair order, chain order,
 * table order, ends ascending; nothing at or beyond `capacity` (0: all four may be null); *h_total = the full length of the list.  The output
 * arrays must not overlap the pair arrays (the caller checks).  Synchronous. */
typedef struct {
    PFACX_verifyRun_t v;            /* the input, the pairs, the chain table, the blob, the caller's arrays */
    const unsigned int *d_entryOff;
    const void *d_entries;
    size_t numEntries;
    size_t maxPieceLen;
    unsigned int maxBudget;
    int bestEnds;
    int *d_end, *d_dist;
} PFACX_editRun_t;
PFAC_status_t PFACX_editRun(PFAC_handle_t handle, const PFACX_editRun_t *run, size_t *h_total);

/* Signatures of byte classes with bounded repeats (no reference counterpart; include/pfac_ext.h: PFACX_clsig*), scan_clsig.hip.
 * PFACX_clsigRun: the class signatures that occur around an ordered list of LONGEST pairs of the anchor set.  d_input, size, the pair arrays,
 * count, d_table and numIds are those of PFACX_gapsigRun.  The signatures anchored by pattern q are d_sigs[d_sigOff[q], d_sigOff[q + 1]) (d_sigOff:
 * numIds + 2 entries; the range is clamped to numSigs), 32 bytes each (pfac_context.h: ClSigEntry): {signature id, first part, number of parts |
 * anchor part << 16, offset of the anchor inside that part}, then {notBefore, notAfter, 0, 0}, by signature id descending.  d_parts, numParts
 * entries of 16 bytes (ClSigPart): {0, len, dword index of its bytes in d_blob, 0} for a literal part, {1, class, lo, hi} for a class part.
 * d_blob, blobWords dwords: per literal part (len + 3) / 4 value dwords.  d_classes: numClasses classes of eight dwords, byte b a member iff bit
 * b & 31 of dword b >> 5 is set.  An entry with no part or more than 64, parts outside the table, an anchor part outside the entry or one that is
 * no literal part is skipped; so is, wherever it is met, a literal part that is empty or whose dwords do not lie inside the blob, and a class part
 * with a class outside the table, hi < lo, hi > 65 535 or hi - lo > 63: nothing lies there.  A boundary class outside the table (other than -1)
 * forbids nothing.  Only each part is tested, not the sum over a signature: where a table's slack exceeds 63 the distances past bit 63 are dropped
 * -- fewer entries, nothing out of bounds; the library's own tables never do.  Part a of a chain member at pair position p lies at x = p -
 * offset; (id, s, end) is kept iff a valid embedding of the signature at s has part a at x, no valid embedding at s has it at a smaller offset,
 * and end is the largest -- with PFACX_CLSIG_SHORTEST_END in `flags` the smallest -- valid end over all embeddings at s (include/pfac_ext.h says
 * what a valid embedding is).  Output as for PFACX_gapsigRun.  Synchronous.
 * A BATCH (PFACX_clsigBatch*): d_offsets, numSegments + 1 values of the caller's in device memory, 1 <= numSegments < 2^31 - 1; null: the plain
 * call, and d_segFirst must be null too.  A launch in front of the passes makes a 32-bit copy of them, each clamped to [0, size] and raised to the
 * largest entry in front of it, in the call's scratch; the passes read only that copy.  A pair belongs to the segment that holds its POSITION (one
 * that lies in none owns nothing), and "the input" of every sentence above is that segment's bytes: starts and ends count from d_input all the
 * same.  d_segFirst (may be null): numSegments + 1 entries, the list index of each segment's first entry and the length of the list, written
 * whatever the capacity; right for a list that ascends by position, unspecified (but inside the array) for any other; all zero for no pairs. */
typedef struct {
    PFACX_verifyRun_t v;            /* the input, the pairs, the chain table, the blob, the caller's arrays */
    const unsigned int *d_sigOff;
    const void *d_sigs;
    size_t numSigs;
    const void *d_parts;
    size_t numParts;
    const unsigned int *d_classes;
    size_t numClasses;
    unsigned int flags;
    int *d_end;
    const size_t *d_offsets;
    size_t numSegments;
    size_t *d_segFirst;
} PFACX_clsigRun_t;
PFAC_status_t PFACX_clsigRun(PFAC_handle_t handle, const PFACX_clsigRun_t *run, size_t *h_total);

/* Covered spans of an unsorted interval list (no reference counterpart; include/pfac_ext.h: PFACX_coverSpans*), scan_cover.hip.
 * PFACX_coverRun: the maximal runs of the bytes of [0, size), 0 < size < 2^31, that one of the intervals [d_start[i], e_i), i < numIntervals,
 * 0 < numIntervals < 2^31, holds -- e_i = d_end[i], or d_start[i] + d_end[i] in 64-bit arithmetic with PFACX_COVER_LENGTHS in `flags` --, each
 * clamped to [0, size] where it is read, an interval that is then empty ignored; any order, duplicates, nesting, overlap.  The interval arrays are
 * only read.  Output: (start, length) of the spans, ascending, into d_spanStart / d_spanLen, nothing at or beyond `capacity` (0: both may be
 * null); *h_numSpans and *h_coveredBytes are the full values whatever the capacity.  The span arrays must not overlap the interval arrays (the
 * caller checks).  No input buffer: `size` only bounds the positions.  Scratch: the handle's cover scratch, sized by `size` alone (scan_cover.hip
 * has the formula).  Synchronous. */
#define PFACX_COVER_BLOCK_BYTES 32768u   /* positions one block of the extract passes covers (scan_cover.hip: kCoverBlockBits; pfac_amd/api.py) */
typedef struct {
    const int *d_start, *d_end;
    size_t numIntervals;
    size_t size;
    unsigned int flags;
    int *d_spanStart, *d_spanLen;
    size_t capacity;
} PFACX_coverRun_t;
PFAC_status_t PFACX_coverRun(PFAC_handle_t handle, const PFACX_coverRun_t *run, size_t *h_numSpans, size_t *h_coveredBytes);

/* Hit lists in start order (no reference counterpart; include/pfac_ext.h: PFACX_orderHits*), scan_order_hits.hip.
 * PFACX_orderRun: the entries (d_start[k], d_ids[k], d_end[k], d_aux[k]), k < numHits, 0 < numHits < 2^31, of the columns that are given, permuted
 * in place so that d_start is non-decreasing as signed ints, stably -- with PFACX_ORDER_TIES_BY_ID (d_ids given) entries of one start ascending by
 * signed id first.  d_perm (null: none) receives the incoming index of the entry now at k.  *h_wasOrdered = 1: the list was in that order already,
 * no column was written and d_perm is the identity.  No two of the arrays overlap (the caller checks).  Column values are keys and nothing else;
 * no index that reaches a store comes from the caller.  Scratch: the handle's order scratch (scan_order_hits.hip has the formula), not allocated
 * by a call that finds the list ordered.  No memory: the allocation status, no array written.  Synchronous. */
#define PFACX_ORDER_TILE 2048u      /* entries of one tile of the count and scatter launches (scan_order_hits.hip: kOrderTile; pfac_amd/api.py) */
#define PFACX_ORDER_THREADS 256u    /* threads of a block of those launches: four waves, each with a contiguous quarter of the tile in rounds of 64 */
typedef struct {
    int *d_start;
    int *d_ids, *d_end, *d_aux;     /* each may be null */
    size_t numHits;
    unsigned int flags;
    int *d_perm;                    /* may be null */
} PFACX_orderRun_t;
PFAC_status_t PFACX_orderRun(PFAC_handle_t handle, const PFACX_orderRun_t *run, int *h_wasOrdered);

/* Every entry point libpfac.so binds out of the module, as X(member of PFAC_context, exported symbol): the one list behind the pointer
 * members (pfac_context.h: each has the type of its prototype above) and behind loadModule (pfac_api.cpp), which binds all of them or
 * none.  The first four keep the reference's member names and typedefs (PFAC_P.h:136-146). */
#define PFAC_MODULE_ENTRIES(X) \
    X(kernel_time_driven_ptr, PFAC_kernel_timeDriven_warpper) X(kernel_space_driven_ptr, PFAC_kernel_spaceDriven_warpper) \
    X(reduce_kernel_ptr, PFAC_reduce_kernel) X(reduce_inplace_kernel_ptr, PFAC_reduce_inplace_kernel) \
    X(batch_fixup_ptr, PFACX_batchFixup) X(batch_reduce_fixup_ptr, PFACX_batchReduceFixup) \
    X(all_reduce_ptr, PFACX_allReduce) X(all_expand_ptr, PFACX_allExpand) X(fold_input_ptr, PFACX_foldInput) \
    X(stream_seam_ptr, PFACX_streamSeam) X(stream_reduce_ptr, PFACX_streamReduce) X(flows_run_ptr, PFACX_flowsRun) \
    X(lines_select_ptr, PFACX_linesSelect) X(lines_select_context_ptr, PFACX_linesSelectContext) X(lines_gather_ptr, PFACX_linesGather) \
    X(spans_select_ptr, PFACX_spansSelect) X(spans_redact_ptr, PFACX_spansRedact) \
    X(count_pairs_ptr, PFACX_countPairs) X(count_nonzero_ptr, PFACX_countNonzero) \
    X(disjoint_select_ptr, PFACX_disjointSelect) X(replace_run_ptr, PFACX_replaceRun) \
    X(rules_run_ptr, PFACX_rulesRun) X(words_run_ptr, PFACX_wordsRun) X(segcount_run_ptr, PFACX_segCountRun) \
    X(groups_run_ptr, PFACX_groupsRun) X(flowrules_run_ptr, PFACX_flowRulesRun) X(split_run_ptr, PFACX_splitRun) \
    X(locate_run_ptr, PFACX_locateRun) X(capture_run_ptr, PFACX_captureRun) X(case_run_ptr, PFACX_caseRun) \
    X(sig_run_ptr, PFACX_sigRun) X(approx_run_ptr, PFACX_approxRun) X(gapsig_run_ptr, PFACX_gapsigRun) \
    X(edit_run_ptr, PFACX_editRun) X(clsig_run_ptr, PFACX_clsigRun) X(cover_run_ptr, PFACX_coverRun) \
    X(order_run_ptr, PFACX_orderRun)

/* Measurement only (no reference counterpart): the traffic shape of the match path with nothing else in it -- every
 * wave reads 1 KiB of d_in and writes 4 KiB of zeros to d_out, non-temporal.  Returns the average milliseconds of
 * `launches` launches over the first n bytes (a multiple of 4096) of d_in, or a negative value on a HIP error.
 * bench.py reports it next to the scan as "what this part sustains for 1 B read : 4 B written" (SURVEY 8d). */
double PFACX_streamProbe(const void *d_in, void *d_out, size_t n, int launches);

/* Measurement only: the compile-time shape of this module (block size, writer waves, walk sets, queue and list capacity,
 * front geometry, ablation / timing builds) as one static string for the bench record. */
const char *PFACX_buildInfo(void);

#ifdef __cplusplus
}
#endif

#endif /* PFAC_MODULE_H_ */
