"""ctypes mirror of the PFAC C ABI (``include/PFAC.h`` + ``include/pfac_ext.h``).

Method names, argument meaning and status codes are those of the reference API
(``/root/reference/PFAC/include/PFAC.h:27-215``) so the tests read like the
reference's own example programs (``PFAC/test/simple_example.cpp``):

    h = PFAC.create()
    h.readPatternFromFile(path)
    h.matchFromDevice(d_in_ptr, n, d_out_ptr)

Pointers are plain integers (``tensor.data_ptr()`` / ``ndarray.ctypes.data``);
this layer never touches torch.  Functions return the ``PFAC_status_t`` value;
the ``check=True`` default raises :class:`PFACError` on a non-zero status.
"""

from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

# enum values, include/PFAC.h
PFAC_PLATFORM_GPU, PFAC_PLATFORM_CPU, PFAC_PLATFORM_CPU_OMP = 0, 1, 2
PFAC_AUTOMATIC, PFAC_TEXTURE_ON, PFAC_TEXTURE_OFF = 0, 1, 2
PFAC_TIME_DRIVEN, PFAC_SPACE_DRIVEN = 0, 1

PFACX_KERNEL_FILTER, PFACX_KERNEL_NAIVE, PFACX_KERNEL_AUTO, PFACX_KERNEL_REFTABLE = 0, 1, 2, 3
PFACX_WALKER_AUTO, PFACX_WALKER_WINDOW, PFACX_WALKER_STAGE, PFACX_WALKER_VETO = 0, 1, 2, 3
PFACX_READ_STRICT, PFACX_READ_STRIP_CR, PFACX_READ_NOCASE = 1, 2, 8
PFACX_LINES_INVERT = 1                          # pfac_ext.h: PFACX_matchLines* select the lines that do NOT match
PFACX_COUNT_LONGEST = 1                         # pfac_ext.h: PFACX_count* count one pattern per position, the longest
PFACX_COUNT_ACCUMULATE = 2                      # ... add to counts[] instead of overwriting it
PFACX_WORDS_ALL = 1                             # pfac_ext.h: PFACX_matchWords* report every bounded occurrence, not the longest per position
PFACX_GROUPS_ALL = 1                            # pfac_ext.h: PFACX_groups* report every enabled occurrence, not the longest enabled one per position
PFACX_CASE_ALL = 1                              # pfac_ext.h: PFACX_case* report every distinct occurring pattern, not the longest one per position
PFACX_CASE_BLOCK = 256                          # scan_case.hip: kCaseBlock, the pairs one block of the case passes takes (never more than eight blocks per CU)
PFACX_SIG_BLOCK = 256                           # scan_sig.hip: kSigBlock, the pairs one block of the signature passes takes (never more than eight blocks per CU)
PFACX_SIG_BLOCKS_PER_CU = 8                     # scan_passes.h: offsetBlocks, as for the case passes
PFACX_SIG_DEFAULT_ANCHOR = 32                   # pfac_ext.h: PFACX_sigOpen cuts an anchor to this many bytes where maxAnchorLen is 0
PFACX_CASE_BLOCKS_PER_CU = 8                    # scan_passes.h: offsetBlocks, the most blocks per compute unit a pass of the expansion frame launches
PFACX_APPROX_BLOCK = 256                        # scan_approx.hip: kApproxBlock, the pairs one block of the approximate passes takes (never more than eight blocks per CU)
PFACX_APPROX_BLOCKS_PER_CU = 8                  # scan_passes.h: offsetBlocks, as for the case passes
PFACX_APPROX_MAX_MISMATCHES = 7                 # pfac_ext.h: the largest budget of a pattern of PFACX_approxOpen
PFACX_GAPSIG_BLOCK = 256                        # scan_gapsig.hip: kGapSigBlock, the pairs one block of the gapped-signature passes takes (never more than eight blocks per CU)
PFACX_GAPSIG_BLOCKS_PER_CU = 8                  # scan_passes.h: offsetBlocks, as for the case passes
PFACX_EDIT_BLOCK = 256                          # scan_edit.hip: kEditBlock, the pairs one block of the edit-distance passes takes (never more than eight blocks per CU)
PFACX_EDIT_BLOCKS_PER_CU = 8                    # scan_passes.h: offsetBlocks, as for the case passes
PFACX_EDIT_MAX_EDITS = 7                        # pfac_ext.h: the largest budget of a pattern of PFACX_editOpen
PFACX_EDIT_BEST_ENDS = 1                        # pfac_ext.h: the open-time flag that keeps only the ends the three-point rule on D passes
PFACX_GAPSIG_MAX_SLACK = 63                     # pfac_ext.h: the largest sum of hi - lo over the gaps of one signature of PFACX_gapsigOpen
PFACX_CLSIG_BLOCK = 256                         # scan_clsig.hip: kClSigBlock, the pairs one block of the class-signature passes takes (never more than eight blocks per CU)
PFACX_CLSIG_BLOCKS_PER_CU = 8                   # scan_passes.h: offsetBlocks, as for the case passes
PFACX_CLSIG_MAX_SLACK = 63                      # pfac_ext.h: the largest sum of hi - lo over the elements of one signature of PFACX_clsigOpen
PFACX_CLSIG_SHORTEST_END = 1                    # pfac_ext.h: the open-time flag that lists the smallest end instead of the largest
PFACX_CLSIG_BOUNDS_BLOCK = 8192                 # scan_clsig.hip: kBoundsBlock, the offsets one block of the batch forms' bounds launch takes
PFACX_CLSIG_STAGED_CLASSES = 64                 # scan_clsig.hip: kClSigStaged, the classes every block stages in LDS; the others are read from device memory
PFACX_GROUPS_BLOCK = 256                        # scan_groups.hip: kGroupsBlock, the pairs one block of the group passes takes (never more than eight blocks per CU)
PFACX_WORDS_BLOCK = 256                         # scan_words.hip: kWordsBlock, the pairs one block of the boundary passes takes (never more than eight blocks per CU)
PFACX_SPLIT_BEFORE = 1                          # pfac_ext.h: PFACX_split* a delimiter opens the segment behind it instead of closing the one in front
PFACX_SPLIT_RUNS = 2                            # ... a maximal run of delimiters cuts once
PFACX_SPLIT_TILE = 16384                        # scan_split.hip: kSplitTile, the input bytes one block of the split passes takes at a time (never more than eight blocks per CU a pass)
PFACX_SPLIT_SCAN_STEP = 1024                    # scan_passes.h: pfac_array_scan, the per-tile counts its one block takes per step
PFACX_LOCATE_CARRY_STEP = 1024                  # scan_locate.hip: pfac_locate_carry, the tiles its one block takes per step (the step of pfac_array_scan)
PFACX_PAIRS_MARK_BLOCK = 256                    # scan_locate.hip, scan_capture.hip: pfac_locate_mark, pfac_capture_mark, the pairs one block of a mark pass takes (scan_passes.h: gridFor)
PFACX_GRID_BLOCKS_PER_CU = 8                    # scan_passes.h: gridCap(c, 8) in gridFor and scan_cuts.h: tileGrid, the most blocks per compute unit of a mark pass and of a block-per-tile pass
PFACX_CAPTURE_AT_POS = 1                        # pfac_ext.h: PFACX_capture* the value starts at the position itself: no ids, no pattern set
PFACX_CAPTURE_REACH = 1024                      # scan_capture.hip: kCaptureReach, the bytes behind a tile of PFACX_SPLIT_TILE bytes that the tile's bitmaps cover; behind them the slow path
PFACX_SPLIT_LONGEST_STEP = 4096                 # scan_split.hip: pfac_split_longest, the tiles its one block takes per step (kSplitPerThread a thread)
PFACX_DISJOINT_BLOCK = 512                      # scan_disjoint.hip: kDisjointBlock, the pairs one block of the selection takes
PFACX_REPLACE_TILE = 4096                       # scan_disjoint.hip: kReplaceTile, the output bytes of one tile of the replacement
PFACX_GATHER_TILE = 4096                        # scan_passes.h: kOutTile, the output bytes of one tile of pfac_lines_gather_copy (the tile of the redaction and the replacement)
PFACX_GATHER_THREADS = 256                      # scan_lines.hip: kLinesThreads, the threads of a block of the gather's passes: 16 output bytes a thread of a tile, a line a thread of the offsets
PFACX_RULES_WINDOW = 8192                       # scan_rules.hip: kRulesWindow, the rules whose masks a block keeps in LDS at a time
PFACX_RULES_TOUCHED = 1024                      # scan_rules.hip: kRulesTouched, the touched-list length; a segment that touches more rules of a window sweeps the whole table
PFACX_RULE_NOT = 1                              # PFACX_rule_member_t.flags: the member holds if NO occurrence satisfies its window
PFACX_RULE_FROM_END = 2                         # the window is measured from the segment's end
RULE_MEMBER_FIELDS = [("pattern", "<i4"), ("flags", "<u4"), ("offset", "<u4"), ("depth", "<u4")]     # PFACX_rule_member_t as a numpy structured dtype: rule_member_dtype()
PFACX_RULE_RELATIVE = 4                         # PFACX_rule_seq_member_t.flags: distance / within tie the member to the one in front of it (PFACX_rulesOpenSeq)
RULE_SEQ_MEMBER_FIELDS = RULE_MEMBER_FIELDS + [("distance", "<u4"), ("within", "<u4")]                # PFACX_rule_seq_member_t: rule_seq_member_dtype()
PFACX_BATCH_BLOCK = 256                         # scan_batch.hip: kBatchBlock, the lanes of a block of every batch fix-up kernel (a block of pairs of the compacted form)
PFACX_BATCH_SEGS_PER_TRIP = 8                   # scan_batch.hip: kSegsPerTrip, the consecutive segments a group of pfac_batch_fixup takes per trip
PFACX_BATCH_MAX_GROUP_LOG2 = 6                  # scan_batch.hip: the `groupLog2 < 6` loop of PFACX_batchFixup, at most 64 lanes per segment
PFACX_FLOWS_PIECE_BLOCK = 256                   # scan_flows.hip: kPieceBlock, the pieces one block of pfac_flows_count / pfac_flows_first takes (and the block sums pfac_flows_sums takes per trip)
PFACX_FLOWS_WAVE_SEAM_MAX = 64                  # scan_flows.hip: kWaveSeamMax, M - 1 up to here takes the wave-per-piece seam, above it the block-per-piece seam
PFACX_FLOWS_WAVE_SEAM_PIECES = 4                # scan_flows.hip: kWaveSeamWaves, the pieces (waves) of one block of pfac_flows_seam_wave
PFACX_STREAM_SEAM_BLOCK = 1024                  # scan_flows.hip, scan_stream.hip: kSeamBlock, the most threads of a seam block: the carried positions seamBlock takes per trip
PFACX_STREAM_SEAM_LDS = 49152                   # pfac_context.h: pfac::kStreamSeamLdsBytes, a seam of more than this many bytes (2 (M - 1)) is staged in device scratch
PFACX_RULES_BLOCK_PAIRS = 256                   # scan_rules.hip: kRulesBlockPairs, the pairs a block takes from a segment in one go
PFACX_FLOWRULES_WINDOW = 8192                   # scan_flowrules.hip: kFlowRulesWindow, the rules whose masks a block keeps in LDS at a time
PFACX_FLOWRULES_TOUCHED = 1024                  # scan_flowrules.hip: kFlowRulesTouched, the touched-list length; a piece that touches more rules of a window sweeps the whole table
PFACX_FLOWRULES_BLOCK_PAIRS = 256               # scan_flowrules.hip: kFlowRulesBlockPairs, the pairs a block takes from a piece in one go
PFACX_SEGCOUNT_WINDOW = 8192                    # scan_segcount.hip: kSegWindow, the pattern ids whose counters a block keeps in LDS at a time
PFACX_SEGCOUNT_TOUCHED = 1024                   # scan_segcount.hip: kSegTouched, the touched-list length; a segment that touches more ids of a window sweeps the whole window
PFACX_SEGCOUNT_BLOCK_PAIRS = 256                # scan_segcount.hip: kSegBlockPairs, the pairs a block takes from a segment in one go
PFACX_COVER_LENGTHS = 1                         # pfac_ext.h: PFACX_coverSpans* the second interval array holds lengths, not ends
PFACX_COVER_BLOCK_BYTES = 32768                 # pfac_module.h: PFACX_COVER_BLOCK_BYTES = scan_cover.hip: kCoverBlockBits, the positions one block of the extract passes covers
PFACX_COVER_MARK_BLOCK = 256                    # scan_cover.hip: kCoverThreads, the intervals one block of pfac_cover_mark takes per trip (scan_passes.h: gridFor, PFACX_GRID_BLOCKS_PER_CU)
PFACX_ORDER_TIES_BY_ID = 1                      # pfac_ext.h: PFACX_orderHits* among equal starts ascending id, then incoming order
PFACX_ORDER_TILE = 2048                         # pfac_module.h: PFACX_ORDER_TILE = scan_order_hits.hip: kOrderTile, the entries of one tile of the count and scatter launches (a block owns contiguous tiles; PFACX_GRID_BLOCKS_PER_CU blocks per compute unit at most)
PFACX_ORDER_THREADS = 256                       # pfac_module.h: PFACX_ORDER_THREADS = scan_order_hits.hip: kOrderThreads: four waves, each with a contiguous quarter of the tile in rounds of 64
PFACX_COUNT_LDS_DIRECT = 16384                  # scan_count.hip: kCountDirect -- sets with F + 1 <= this count into a counter per id in LDS, larger ones into a tagged cache
(PFACX_TABLE_DENSE, PFACX_TABLE_HASH_ROWPTR, PFACX_TABLE_HASH_VALPTR, PFACX_TABLE_INITIAL_ROW,
 PFACX_TABLE_FILTER_GRAM3, PFACX_TABLE_FILTER_SHORT, PFACX_TABLE_FILTER_LADDER, PFACX_TABLE_FILTER_FINAL3,
 PFACX_TABLE_CHAIN) = range(9)
PFACX_TABLE_FILTER_GRAM1, PFACX_TABLE_FILTER_PREFIX4, PFACX_TABLE_FILTER_TAIL, PFACX_TABLE_FILTER_TAIL_GLOBAL, PFACX_TABLE_FILTER_SKIP = 9, 10, 11, 12, 13
PFACX_TABLE_PREFIX_PATTERN = 14


class STATUS:
    SUCCESS = 0
    BASE = 10000
    ALLOC_FAILED = 10001
    CUDA_ALLOC_FAILED = 10002
    INVALID_HANDLE = 10003
    INVALID_PARAMETER = 10004
    PATTERNS_NOT_READY = 10005
    FILE_OPEN_ERROR = 10006
    LIB_NOT_EXIST = 10007
    ARCH_MISMATCH = 10008
    MUTEX_ERROR = 10009
    INTERNAL_ERROR = 10010
    OUTPUT_TRUNCATED = 10100     # pfac_ext.h: PFACX_STATUS_OUTPUT_TRUNCATED (PFACX_matchAll*)


class PFACError(RuntimeError):
    def __init__(self, status: int, where: str, message: str):
        super().__init__(f"{where}: status {status}: {message}")
        self.status = status


class PFACX_info(C.Structure):
    _fields_ = [
        ("structSize", C.c_size_t),
        ("numOfPatterns", C.c_int), ("numOfStates", C.c_int), ("numOfFinalStates", C.c_int),
        ("initialState", C.c_int), ("maxPatternLen", C.c_int), ("numOfLeaves", C.c_int),
        ("perfMode", C.c_int), ("textureMode", C.c_int), ("platform", C.c_int), ("hasDevice", C.c_int),
        ("numOfTableEntry", C.c_size_t), ("sizeOfTableEntry", C.c_size_t), ("sizeOfTableInBytes", C.c_size_t),
        ("filterLog2Bits", C.c_int), ("filterHasShort", C.c_int), ("filterBitsSet", C.c_size_t),
        ("kernelVariant", C.c_int), ("multiProcessorCount", C.c_int),
        ("filterLog2BitsLadder", C.c_int), ("filterLog2BitsFinal3", C.c_int), ("filterBitsSetLadder", C.c_size_t),
        ("chainJumpLog2", C.c_int), ("chainSlots", C.c_size_t),
        ("ladderStops", C.c_size_t), ("ladderGoOns", C.c_size_t), ("ladderThin", C.c_int), ("ladderExtend", C.c_int),
        ("trailingBytesIgnored", C.c_size_t), ("deviceTableBytes", C.c_size_t), ("deviceScratchBytes", C.c_size_t),
        ("streamNearMisses", C.c_int), ("streamDense", C.c_int), ("filterLadderLast", C.c_int), ("filterTailEntries", C.c_size_t),
        ("filterTailGlobalEntries", C.c_size_t), ("filterLog2TailGlobal", C.c_int), ("filterLadderSalt", C.c_uint), ("filterSkipTags", C.c_int),
        ("maxMatchesPerPosition", C.c_int),
    ]


class PFACX_info_nocase(PFACX_info):
    """PFACX_info_t as it is now: PFACX_info plus the field appended with PFACX_READ_NOCASE (a ctypes subclass lays its fields out
    behind its base's, as the header does).  PFAC.caseInsensitive() reads it; PFAC.info() keeps the shorter struct, and the library
    fills as much as structSize says."""
    _fields_ = [("caseInsensitive", C.c_int)]


class PFACX_scan_stats(C.Structure):
    _fields_ = [("structSize", C.c_size_t), ("walkerRounds", C.c_ulonglong), ("laneSteps", C.c_ulonglong), ("walksStarted", C.c_ulonglong),
                ("level1Hits", C.c_ulonglong), ("tilesPerChunk", C.c_int), ("walksPerLane", C.c_int),
                ("ladderCandidates", C.c_ulonglong), ("denseChunks", C.c_ulonglong), ("filterKernelMs", C.c_double),
                ("stageModeWaves", C.c_ulonglong), ("walker", C.c_int), ("veto", C.c_int)]


_LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")
_lib: Optional[C.CDLL] = None

EXPORTED_SYMBOLS = (
    # include/PFAC.h
    "PFAC_create", "PFAC_destroy", "PFAC_setPlatform", "PFAC_setTextureMode", "PFAC_setPerfMode",
    "PFAC_getErrorString", "PFAC_dumpTransitionTable", "PFAC_readPatternFromFile",
    "PFAC_matchFromDevice", "PFAC_matchFromHost", "PFAC_matchFromDeviceReduce", "PFAC_matchFromHostReduce",
    # include/pfac_ext.h
    "PFACX_createHostOnly", "PFACX_getInfo", "PFACX_getTable", "PFACX_setKernelVariant",
    "PFACX_readPatternFromMemory", "PFACX_getScanStats", "PFACX_saveCompiled", "PFACX_loadCompiled",
    "PFACX_matchFromHostMultiGPU", "PFACX_matchFromHostReduceMultiGPU", "PFACX_readPatternFromFileEx", "PFACX_readPatternFromMemoryEx", "PFACX_trim",
    "PFACX_setKernelTiming", "PFACX_setWalker", "PFACX_prepare",
    "PFACX_matchBatchFromDevice", "PFACX_matchBatchFromHost", "PFACX_matchBatchFromDeviceReduce",
    "PFACX_matchAllFromDevice", "PFACX_matchAllFromHost", "PFACX_matchAllBatchFromDevice",
    "PFACX_streamOpen", "PFACX_streamReset", "PFACX_streamClose", "PFACX_streamMatchFromDevice", "PFACX_streamMatchFromHost", "PFACX_streamFlush",
    "PFACX_flowsOpen", "PFACX_flowsClose", "PFACX_flowsReset", "PFACX_flowsMatchFromDevice", "PFACX_flowsMatchFromHost", "PFACX_flowsFlush",
    "PFACX_matchLinesFromDevice", "PFACX_matchLinesFromHost", "PFACX_gatherLinesFromDevice",
    "PFACX_matchLinesContextFromDevice", "PFACX_matchLinesContextFromHost",
    "PFACX_matchSpansFromDevice", "PFACX_matchSpansFromHost", "PFACX_redactSpansFromDevice",
    "PFACX_countFromDevice", "PFACX_countFromHost", "PFACX_countPairsFromDevice", "PFACX_countNonzeroFromDevice",
    "PFACX_matchDisjointFromDevice", "PFACX_matchDisjointFromHost", "PFACX_replaceFromDevice", "PFACX_replaceFromHost",
    "PFACX_rulesOpen", "PFACX_rulesOpenEx", "PFACX_rulesOpenSeq", "PFACX_rulesClose", "PFACX_rulesMatchFromDevice", "PFACX_rulesMatchFromHost",
    "PFACX_flowRulesOpen", "PFACX_flowRulesClose", "PFACX_flowRulesReset", "PFACX_flowRulesPairsFromDevice", "PFACX_flowRulesPairsFromHost",
    "PFACX_matchWordsFromDevice", "PFACX_matchWordsFromHost", "PFACX_wordsPairsFromDevice",
    "PFACX_countBatchFromDevice", "PFACX_countBatchFromHost", "PFACX_countBatchPairsFromDevice",
    "PFACX_groupsOpen", "PFACX_groupsClose", "PFACX_groupsMatchFromDevice", "PFACX_groupsMatchFromHost", "PFACX_groupsPairsFromDevice",
    "PFACX_splitFromDevice", "PFACX_splitFromHost",
    "PFACX_locatePairsFromDevice", "PFACX_locatePairsFromHost", "PFACX_matchLocatedFromDevice", "PFACX_matchLocatedFromHost",
    "PFACX_capturePairsFromDevice", "PFACX_capturePairsFromHost", "PFACX_matchCapturedFromDevice", "PFACX_matchCapturedFromHost",
    "PFACX_caseOpen", "PFACX_caseClose", "PFACX_caseMatchFromDevice", "PFACX_caseMatchFromHost", "PFACX_casePairsFromDevice",
    "PFACX_sigOpen", "PFACX_sigOpenText", "PFACX_sigGetAnchors", "PFACX_sigClose", "PFACX_sigMatchFromDevice", "PFACX_sigMatchFromHost",
    "PFACX_sigPairsFromDevice",
    "PFACX_approxOpen", "PFACX_approxGetPieces", "PFACX_approxClose", "PFACX_approxMatchFromDevice", "PFACX_approxMatchFromHost",
    "PFACX_approxPairsFromDevice",
    "PFACX_gapsigOpen", "PFACX_gapsigOpenText", "PFACX_gapsigGetAnchors", "PFACX_gapsigClose", "PFACX_gapsigMatchFromDevice",
    "PFACX_gapsigMatchFromHost", "PFACX_gapsigPairsFromDevice",
    "PFACX_editOpen", "PFACX_editGetPieces", "PFACX_editClose", "PFACX_editMatchFromDevice", "PFACX_editMatchFromHost",
    "PFACX_editPairsFromDevice",
    "PFACX_clsigOpen", "PFACX_clsigOpenText", "PFACX_clsigGetAnchors", "PFACX_clsigClose", "PFACX_clsigMatchFromDevice",
    "PFACX_clsigMatchFromHost", "PFACX_clsigPairsFromDevice", "PFACX_clsigBatchMatchFromDevice", "PFACX_clsigBatchMatchFromHost",
    "PFACX_clsigBatchPairsFromDevice",
    "PFACX_coverSpansFromDevice", "PFACX_coverSpansFromHost",
    "PFACX_orderHitsFromDevice", "PFACX_orderHitsFromHost",
)
MODULE_SYMBOLS = (  # include/pfac_module.h, exported by libpfac_gfx950.so
    "PFAC_kernel_timeDriven_warpper", "PFAC_kernel_spaceDriven_warpper",
    "PFAC_reduce_kernel", "PFAC_reduce_inplace_kernel", "PFACX_streamProbe", "PFACX_buildInfo",
    "PFACX_batchFixup", "PFACX_batchReduceFixup",
    "PFACX_allReduce", "PFACX_allExpand", "PFACX_foldInput",
    "PFACX_streamSeam", "PFACX_streamReduce", "PFACX_flowsRun",
    "PFACX_linesSelect", "PFACX_linesSelectContext", "PFACX_linesGather", "PFACX_linesBitmapProbe", "PFACX_orderPairsProbe",
    "PFACX_spansSelect", "PFACX_spansRedact",
    "PFACX_countPairs", "PFACX_countNonzero",
    "PFACX_disjointSelect", "PFACX_replaceRun",
    "PFACX_rulesRun",
    "PFACX_wordsRun",
    "PFACX_segCountRun",
    "PFACX_groupsRun",
    "PFACX_flowRulesRun",
    "PFACX_splitRun",
    "PFACX_locateRun",
    "PFACX_captureRun",
    "PFACX_caseRun",
    "PFACX_sigRun",
    "PFACX_approxRun",
    "PFACX_gapsigRun",
    "PFACX_editRun",
    "PFACX_clsigRun",
    "PFACX_coverRun",
    "PFACX_orderRun",
)


def library_paths() -> Tuple[str, str]:
    # PFAC_HOST_LIB: another build of the HOST library (the sanitizer builds of `make -C pfac_amd/csrc san`: tests/test_sanitizers.py)
    return os.environ.get("PFAC_HOST_LIB") or os.path.join(_LIB_DIR, "libpfac.so"), os.path.join(_LIB_DIR, "libpfac_gfx950.so")


def load_library() -> C.CDLL:
    """Load libpfac.so.  There is no fallback: a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    host, module = library_paths()
    for p in (host, module):
        if not os.path.exists(p):
            raise ImportError(
                f"{p} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"or `make -C pfac_amd/csrc`. pfac_amd has no non-HIP fallback.")
    lib = C.CDLL(host)
    H = C.c_void_p
    lib.PFAC_create.argtypes = [C.POINTER(H)]
    lib.PFACX_createHostOnly.argtypes = [C.POINTER(H)]
    lib.PFAC_destroy.argtypes = [H]
    lib.PFAC_setPlatform.argtypes = [H, C.c_int]
    lib.PFAC_setTextureMode.argtypes = [H, C.c_int]
    lib.PFAC_setPerfMode.argtypes = [H, C.c_int]
    lib.PFAC_getErrorString.argtypes = [C.c_int]
    lib.PFAC_getErrorString.restype = C.c_char_p
    lib.PFAC_dumpTransitionTable.argtypes = [H, C.c_void_p]
    lib.PFAC_readPatternFromFile.argtypes = [H, C.c_char_p]
    lib.PFAC_matchFromDevice.argtypes = [H, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.PFAC_matchFromHost.argtypes = [H, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.PFAC_matchFromDeviceReduce.argtypes = [H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    lib.PFAC_matchFromHostReduce.argtypes = [H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    lib.PFACX_getInfo.argtypes = [H, C.POINTER(PFACX_info)]           # (PFACX_info_nocase is one: a subclass)
    lib.PFACX_getTable.argtypes = [H, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.PFACX_setKernelVariant.argtypes = [H, C.c_int]
    if hasattr(lib, "PFACX_setWalker"):                  # (tools/ab.py also loads the libraries of earlier revisions)
        lib.PFACX_setWalker.argtypes = [H, C.c_int]
    lib.PFACX_readPatternFromMemory.argtypes = [H, C.c_char_p, C.c_size_t]
    lib.PFACX_trim.argtypes = [H]
    if hasattr(lib, "PFACX_prepare"):
        lib.PFACX_prepare.argtypes = [H, C.c_size_t]
    lib.PFACX_setKernelTiming.argtypes = [H, C.c_int]
    lib.PFACX_readPatternFromFileEx.argtypes = [H, C.c_char_p, C.c_uint]
    lib.PFACX_readPatternFromMemoryEx.argtypes = [H, C.c_char_p, C.c_size_t, C.c_uint]
    lib.PFACX_getScanStats.argtypes = [H, C.POINTER(PFACX_scan_stats)]
    lib.PFACX_saveCompiled.argtypes = [H, C.c_char_p]
    lib.PFACX_loadCompiled.argtypes = [H, C.c_char_p]
    lib.PFACX_matchFromHostMultiGPU.argtypes = [H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    if hasattr(lib, "PFACX_matchFromHostReduceMultiGPU"):
        lib.PFACX_matchFromHostReduceMultiGPU.argtypes = [H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    if hasattr(lib, "PFACX_matchBatchFromDevice"):
        lib.PFACX_matchBatchFromDevice.argtypes = [H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.PFACX_matchBatchFromHost.argtypes = [H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.PFACX_matchBatchFromDeviceReduce.argtypes = [H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                         C.c_void_p, C.POINTER(C.c_int)]
    if hasattr(lib, "PFACX_matchAllFromDevice"):
        SZ = C.POINTER(C.c_size_t)
        lib.PFACX_matchAllFromDevice.argtypes = [H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, SZ]
        lib.PFACX_matchAllFromHost.argtypes = [H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, SZ]
        lib.PFACX_matchAllBatchFromDevice.argtypes = [H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                      C.c_size_t, C.c_void_p, SZ]
    if hasattr(lib, "PFACX_streamOpen"):
        lib.PFACX_streamOpen.argtypes = [H, C.POINTER(C.c_void_p)]
        lib.PFACX_streamReset.argtypes = [C.c_void_p]
        lib.PFACX_streamClose.argtypes = [C.c_void_p]
        piece = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]
        lib.PFACX_streamMatchFromDevice.argtypes = piece
        lib.PFACX_streamMatchFromHost.argtypes = piece
        lib.PFACX_streamFlush.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
    if hasattr(lib, "PFACX_flowsOpen"):
        lib.PFACX_flowsOpen.argtypes = [H, C.c_size_t, C.POINTER(C.c_void_p)]
        lib.PFACX_flowsClose.argtypes = [C.c_void_p]
        lib.PFACX_flowsReset.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        pieces = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                  C.c_void_p, C.POINTER(C.c_int)]
        lib.PFACX_flowsMatchFromDevice.argtypes = pieces
        lib.PFACX_flowsMatchFromHost.argtypes = pieces
        lib.PFACX_flowsFlush.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_int)]
    if hasattr(lib, "PFACX_matchLinesFromDevice"):
        SZ = C.POINTER(C.c_size_t)
        lines = [H, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, SZ, SZ]
        lib.PFACX_matchLinesFromDevice.argtypes = lines
        lib.PFACX_matchLinesFromHost.argtypes = lines
        lib.PFACX_gatherLinesFromDevice.argtypes = [H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, SZ]
    if hasattr(lib, "PFACX_matchLinesContextFromDevice"):
        SZ = C.POINTER(C.c_size_t)
        context = [H, C.c_void_p, C.c_size_t, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, SZ, SZ, SZ, SZ]
        lib.PFACX_matchLinesContextFromDevice.argtypes = context
        lib.PFACX_matchLinesContextFromHost.argtypes = context
    if hasattr(lib, "PFACX_matchSpansFromDevice"):
        SZ = C.POINTER(C.c_size_t)
        spans = [H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, SZ, SZ]
        lib.PFACX_matchSpansFromDevice.argtypes = spans
        lib.PFACX_matchSpansFromHost.argtypes = spans
        lib.PFACX_redactSpansFromDevice.argtypes = [H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_ubyte, C.c_void_p]
    if hasattr(lib, "PFACX_coverSpansFromDevice"):
        SZ = C.POINTER(C.c_size_t)
        cover = [H, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint, C.c_void_p, C.c_void_p, C.c_size_t, SZ, SZ]
        lib.PFACX_coverSpansFromDevice.argtypes = cover
        lib.PFACX_coverSpansFromHost.argtypes = cover
    if hasattr(lib, "PFACX_orderHitsFromDevice"):
        order = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p, C.POINTER(C.c_int)]
        lib.PFACX_orderHitsFromDevice.argtypes = order
        lib.PFACX_orderHitsFromHost.argtypes = order
    if hasattr(lib, "PFACX_countFromDevice"):
        SZ = C.POINTER(C.c_size_t)
        count = [H, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p, C.c_size_t, SZ]
        lib.PFACX_countFromDevice.argtypes = count
        lib.PFACX_countFromHost.argtypes = count
        lib.PFACX_countPairsFromDevice.argtypes = [H, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p, C.c_size_t]
        lib.PFACX_countNonzeroFromDevice.argtypes = [H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, SZ, C.POINTER(C.c_ulonglong)]
    if hasattr(lib, "PFACX_matchDisjointFromDevice"):
        SZ = C.POINTER(C.c_size_t)
        disjoint = [H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, SZ, SZ]
        lib.PFACX_matchDisjointFromDevice.argtypes = disjoint
        lib.PFACX_matchDisjointFromHost.argtypes = disjoint
        replace = [H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, SZ]
        lib.PFACX_replaceFromDevice.argtypes = replace
        lib.PFACX_replaceFromHost.argtypes = replace
    if hasattr(lib, "PFACX_rulesOpen"):
        SZ = C.POINTER(C.c_size_t)
        lib.PFACX_rulesOpen.argtypes = [H, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        if hasattr(lib, "PFACX_rulesOpenEx"):
            lib.PFACX_rulesOpenEx.argtypes = [H, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        if hasattr(lib, "PFACX_rulesOpenSeq"):
            lib.PFACX_rulesOpenSeq.argtypes = [H, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        lib.PFACX_rulesClose.argtypes = [C.c_void_p]
        rules = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, SZ]
        lib.PFACX_rulesMatchFromDevice.argtypes = rules
        lib.PFACX_rulesMatchFromHost.argtypes = rules
    if hasattr(lib, "PFACX_flowRulesOpen"):
        SZ = C.POINTER(C.c_size_t)
        lib.PFACX_flowRulesOpen.argtypes = [H, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p)]
        lib.PFACX_flowRulesClose.argtypes = [C.c_void_p]
        lib.PFACX_flowRulesReset.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        pairs = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, SZ]
        lib.PFACX_flowRulesPairsFromDevice.argtypes = pairs
        lib.PFACX_flowRulesPairsFromHost.argtypes = pairs
    if hasattr(lib, "PFACX_matchWordsFromDevice"):
        SZ = C.POINTER(C.c_size_t)
        CLS = C.POINTER(C.c_uint)
        words = [H, C.c_void_p, C.c_size_t, CLS, C.c_uint, C.c_void_p, C.c_void_p, C.c_size_t, SZ]
        lib.PFACX_matchWordsFromDevice.argtypes = words
        lib.PFACX_matchWordsFromHost.argtypes = words
        lib.PFACX_wordsPairsFromDevice.argtypes = [H, C.c_void_p, C.c_size_t, CLS, C.c_uint, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                   C.c_size_t, SZ]
    if hasattr(lib, "PFACX_countBatchFromDevice"):
        SZ = C.POINTER(C.c_size_t)
        batch = [H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, SZ, C.POINTER(C.c_ulonglong)]
        lib.PFACX_countBatchFromDevice.argtypes = batch
        lib.PFACX_countBatchFromHost.argtypes = batch
        lib.PFACX_countBatchPairsFromDevice.argtypes = batch
    if hasattr(lib, "PFACX_groupsOpen"):
        SZ = C.POINTER(C.c_size_t)
        lib.PFACX_groupsOpen.argtypes = [H, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        lib.PFACX_groupsClose.argtypes = [C.c_void_p]
        groups = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                  C.c_void_p, SZ]
        lib.PFACX_groupsMatchFromDevice.argtypes = groups
        lib.PFACX_groupsMatchFromHost.argtypes = groups
        lib.PFACX_groupsPairsFromDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint,
                                                    C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, SZ]
    if hasattr(lib, "PFACX_splitFromDevice"):
        SZ = C.POINTER(C.c_size_t)
        split = [H, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint), C.c_uint, C.c_void_p, C.c_size_t, SZ, SZ]
        lib.PFACX_splitFromDevice.argtypes = split
        lib.PFACX_splitFromHost.argtypes = split
    if hasattr(lib, "PFACX_locatePairsFromDevice"):
        SZ = C.POINTER(C.c_size_t)
        pairs = [H, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint), C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, SZ]
        lib.PFACX_locatePairsFromDevice.argtypes = pairs
        lib.PFACX_locatePairsFromHost.argtypes = pairs
        located = [H, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint), C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                   C.POINTER(C.c_int)]
        lib.PFACX_matchLocatedFromDevice.argtypes = located
        lib.PFACX_matchLocatedFromHost.argtypes = located
    if hasattr(lib, "PFACX_capturePairsFromDevice"):
        CLS = C.POINTER(C.c_uint)
        pairs = [H, C.c_void_p, C.c_size_t, CLS, CLS, C.c_size_t, C.c_uint, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.PFACX_capturePairsFromDevice.argtypes = pairs
        lib.PFACX_capturePairsFromHost.argtypes = pairs
        captured = [H, C.c_void_p, C.c_size_t, CLS, CLS, C.c_size_t, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                    C.POINTER(C.c_int)]
        lib.PFACX_matchCapturedFromDevice.argtypes = captured
        lib.PFACX_matchCapturedFromHost.argtypes = captured
    if hasattr(lib, "PFACX_caseOpen"):
        SZ = C.POINTER(C.c_size_t)
        lib.PFACX_caseOpen.argtypes = [H, C.c_char_p, C.c_size_t, C.c_uint, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
        lib.PFACX_caseClose.argtypes = [C.c_void_p]
        cased = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p, C.c_void_p, C.c_size_t, SZ]
        lib.PFACX_caseMatchFromDevice.argtypes = cased
        lib.PFACX_caseMatchFromHost.argtypes = cased
        lib.PFACX_casePairsFromDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                  C.c_size_t, SZ]
    if hasattr(lib, "PFACX_sigOpen"):
        SZ = C.POINTER(C.c_size_t)
        lib.PFACX_sigOpen.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
        lib.PFACX_sigOpenText.argtypes = [H, C.c_char_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
        lib.PFACX_sigGetAnchors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.PFACX_sigClose.argtypes = [C.c_void_p]
        masked = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, SZ]
        lib.PFACX_sigMatchFromDevice.argtypes = masked
        lib.PFACX_sigMatchFromHost.argtypes = masked
        lib.PFACX_sigPairsFromDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, SZ]
    if hasattr(lib, "PFACX_approxOpen"):
        SZ = C.POINTER(C.c_size_t)
        lib.PFACX_approxOpen.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_int)]
        lib.PFACX_approxGetPieces.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.PFACX_approxClose.argtypes = [C.c_void_p]
        within = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, SZ]
        lib.PFACX_approxMatchFromDevice.argtypes = within
        lib.PFACX_approxMatchFromHost.argtypes = within
        lib.PFACX_approxPairsFromDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_size_t, SZ]
    if hasattr(lib, "PFACX_gapsigOpen"):
        SZ = C.POINTER(C.c_size_t)
        lib.PFACX_gapsigOpen.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                         C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
        lib.PFACX_gapsigOpenText.argtypes = [H, C.c_char_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
        lib.PFACX_gapsigGetAnchors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.PFACX_gapsigClose.argtypes = [C.c_void_p]
        gapped = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, SZ]
        lib.PFACX_gapsigMatchFromDevice.argtypes = gapped
        lib.PFACX_gapsigMatchFromHost.argtypes = gapped
        lib.PFACX_gapsigPairsFromDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_size_t, SZ]
    if hasattr(lib, "PFACX_editOpen"):
        SZ = C.POINTER(C.c_size_t)
        lib.PFACX_editOpen.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint, C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_int)]
        lib.PFACX_editGetPieces.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.PFACX_editClose.argtypes = [C.c_void_p]
        edits = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, SZ]
        lib.PFACX_editMatchFromDevice.argtypes = edits
        lib.PFACX_editMatchFromHost.argtypes = edits
        lib.PFACX_editPairsFromDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_size_t, SZ]
    if hasattr(lib, "PFACX_clsigOpen"):
        SZ = C.POINTER(C.c_size_t)
        lib.PFACX_clsigOpen.argtypes = [H, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_size_t, C.c_uint, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
        lib.PFACX_clsigOpenText.argtypes = [H, C.c_char_p, C.c_size_t, C.c_size_t, C.c_uint, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
        lib.PFACX_clsigGetAnchors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.PFACX_clsigClose.argtypes = [C.c_void_p]
        classed = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, SZ]
        lib.PFACX_clsigMatchFromDevice.argtypes = classed
        lib.PFACX_clsigMatchFromHost.argtypes = classed
        lib.PFACX_clsigPairsFromDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_size_t, SZ]
    if hasattr(lib, "PFACX_clsigBatchMatchFromDevice"):
        SZ = C.POINTER(C.c_size_t)
        batched = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, SZ]
        lib.PFACX_clsigBatchMatchFromDevice.argtypes = batched
        lib.PFACX_clsigBatchMatchFromHost.argtypes = batched
        lib.PFACX_clsigBatchPairsFromDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, SZ]
    for name in EXPORTED_SYMBOLS:
        if os.environ.get("PFAC_AB_OLD_LIBS") and not hasattr(lib, name):     # tools/ab.py: the library of an earlier revision
            continue
        fn = getattr(lib, name)
        if name != "PFAC_getErrorString":
            fn.restype = C.c_int
    _lib = lib
    return lib


def word_class(members=None):
    """The eight words of a byte class for PFACX_matchWords*: byte b is in the class iff bit b & 31 of word b >> 5 is set.  `members`: bytes (or any
    iterable of byte values); None: the default class [0-9A-Za-z_]."""
    if members is None:
        members = b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz_"
    words = [0] * 8
    for b in bytes(members):
        words[b >> 5] |= 1 << (b & 31)
    return (C.c_uint * 8)(*words)


def word_class_except(excluded):
    """... of every byte but `excluded`: word_class_except(b"\n") is grep -x, word_class_except(b",\n") whole CSV fields."""
    return word_class(bytes(set(range(256)) - set(bytes(excluded))))


def _class_arg(cls):
    if cls is None or isinstance(cls, C.Array):
        return cls
    return word_class(cls)


_libc = C.CDLL(None)
_libc.fopen.restype = C.c_void_p
_libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
_libc.fclose.argtypes = [C.c_void_p]


def error_string(status: int) -> str:
    s = load_library().PFAC_getErrorString(int(status))
    return s.decode("latin1") if s else ""


class PFAC:
    """One PFAC handle (``PFAC_handle_t``)."""

    def __init__(self, handle: C.c_void_p):
        self._h = handle
        self._lib = load_library()

    # -- lifecycle -----------------------------------------------------------------
    @classmethod
    def create(cls, check: bool = True) -> "PFAC":
        """``PFAC_create``: binds the current HIP device and loads the gfx950 module."""
        lib = load_library()
        h = C.c_void_p()
        st = lib.PFAC_create(C.byref(h))
        if st != 0:
            if h:
                lib.PFAC_destroy(h)
            if check:
                raise PFACError(st, "PFAC_create", error_string(st))
            obj = cls(C.c_void_p())
            obj.create_status = st
            return obj
        obj = cls(h)
        obj.create_status = 0
        # test harness: PFAC_TEST_WALKER=window|stage runs a whole test session with one walker of the full-result kernel
        forced = {"window": PFACX_WALKER_WINDOW, "stage": PFACX_WALKER_STAGE, "veto": PFACX_WALKER_VETO}.get(os.environ.get("PFAC_TEST_WALKER", "").lower())
        if forced is not None:
            obj.setWalker(forced)
        return obj

    @classmethod
    def createHostOnly(cls) -> "PFAC":
        """``PFACX_createHostOnly``: pattern compiler + CPU platforms, no device."""
        lib = load_library()
        h = C.c_void_p()
        st = lib.PFACX_createHostOnly(C.byref(h))
        if st != 0:
            raise PFACError(st, "PFACX_createHostOnly", error_string(st))
        obj = cls(h)
        obj.create_status = 0
        return obj

    def destroy(self) -> int:
        st = self._lib.PFAC_destroy(self._h)
        self._h = C.c_void_p()
        return st

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self._h:
            self.destroy()

    def _ret(self, st: int, where: str, check: bool) -> int:
        if check and st != 0:
            raise PFACError(st, where, error_string(st))
        return st

    # -- configuration -------------------------------------------------------------
    def setPlatform(self, platform: int, check: bool = True) -> int:
        return self._ret(self._lib.PFAC_setPlatform(self._h, platform), "PFAC_setPlatform", check)

    def setTextureMode(self, mode: int, check: bool = True) -> int:
        return self._ret(self._lib.PFAC_setTextureMode(self._h, mode), "PFAC_setTextureMode", check)

    def setPerfMode(self, mode: int, check: bool = True) -> int:
        return self._ret(self._lib.PFAC_setPerfMode(self._h, mode), "PFAC_setPerfMode", check)

    def setKernelVariant(self, variant: int, check: bool = True) -> int:
        return self._ret(self._lib.PFACX_setKernelVariant(self._h, variant), "PFACX_setKernelVariant", check)

    def setWalker(self, walker: int, check: bool = True) -> int:
        """PFACX_WALKER_AUTO / _WINDOW / _STAGE: the walker of the full-result filter kernel (include/pfac_ext.h)"""
        return self._ret(self._lib.PFACX_setWalker(self._h, walker), "PFACX_setWalker", check)

    def readPatternFromFile(self, filename, check: bool = True) -> int:
        name = None if filename is None else os.fsencode(filename)
        return self._ret(self._lib.PFAC_readPatternFromFile(self._h, name), "PFAC_readPatternFromFile", check)

    def readPatternFromMemory(self, data: bytes, check: bool = True) -> int:
        """``PFACX_readPatternFromMemory``: the pattern-file bytes without a file."""
        return self._ret(self._lib.PFACX_readPatternFromMemory(self._h, data, len(data)), "PFACX_readPatternFromMemory", check)

    def prepare(self, max_bytes: int = 0, check: bool = True) -> int:
        """``PFACX_prepare``: staging, scratch and code objects of the host paths ahead of the first call."""
        return self._ret(self._lib.PFACX_prepare(self._h, max_bytes), "PFACX_prepare", check)

    def trim(self, check: bool = True) -> int:
        """``PFACX_trim``: free the handle's grow-only device temporaries."""
        return self._ret(self._lib.PFACX_trim(self._h), "PFACX_trim", check)

    def setKernelTiming(self, on: bool, check: bool = True) -> int:
        """``PFACX_setKernelTiming``: HIP events around the filter kernel's launch; ``scanStats().filterKernelMs``."""
        return self._ret(self._lib.PFACX_setKernelTiming(self._h, 1 if on else 0), "PFACX_setKernelTiming", check)

    def readPatternFromFileEx(self, filename, flags: int, check: bool = True) -> int:
        """``PFACX_readPatternFromFileEx``: flags = PFACX_READ_STRICT | PFACX_READ_STRIP_CR | PFACX_READ_NOCASE."""
        name = None if filename is None else os.fsencode(filename)
        return self._ret(self._lib.PFACX_readPatternFromFileEx(self._h, name, flags), "PFACX_readPatternFromFileEx", check)

    def readPatternFromMemoryEx(self, data: bytes, flags: int, check: bool = True) -> int:
        return self._ret(self._lib.PFACX_readPatternFromMemoryEx(self._h, data, len(data), flags), "PFACX_readPatternFromMemoryEx", check)

    def saveCompiled(self, filename, check: bool = True) -> int:
        """``PFACX_saveCompiled``: the compiled pattern set (trie, tables, prefilter) to a file."""
        return self._ret(self._lib.PFACX_saveCompiled(self._h, os.fsencode(filename)), "PFACX_saveCompiled", check)

    def loadCompiled(self, filename, check: bool = True) -> int:
        """``PFACX_loadCompiled``: replaces the pattern set with a saved one."""
        return self._ret(self._lib.PFACX_loadCompiled(self._h, os.fsencode(filename)), "PFACX_loadCompiled", check)

    def matchFromHostMultiGPU(self, h_input: int, size: int, h_result: int, devices=None, check: bool = True) -> int:
        """``PFACX_matchFromHostMultiGPU``: `devices` = list of device ordinals (None = every visible device)."""
        if devices is None:
            st = self._lib.PFACX_matchFromHostMultiGPU(self._h, h_input, size, h_result, 0, None)
        else:
            arr = (C.c_int * len(devices))(*devices)
            st = self._lib.PFACX_matchFromHostMultiGPU(self._h, h_input, size, h_result, len(devices), arr)
        return self._ret(st, "PFACX_matchFromHostMultiGPU", check)

    def matchFromHostReduceMultiGPU(self, h_input: int, size: int, h_result: int, h_pos: int, devices=None, check: bool = True):
        """``PFACX_matchFromHostReduceMultiGPU`` -> (status, number of pairs)."""
        n = C.c_int(0)
        if devices is None:
            st = self._lib.PFACX_matchFromHostReduceMultiGPU(self._h, h_input, size, h_result, h_pos, C.byref(n), 0, None)
        else:
            arr = (C.c_int * len(devices))(*devices)
            st = self._lib.PFACX_matchFromHostReduceMultiGPU(self._h, h_input, size, h_result, h_pos, C.byref(n), len(devices), arr)
        return self._ret(st, "PFACX_matchFromHostReduceMultiGPU", check), n.value

    def dumpTransitionTable(self, path: str, check: bool = True) -> int:
        fp = _libc.fopen(os.fsencode(path), b"w")
        if not fp:
            raise OSError(f"cannot open {path}")
        try:
            st = self._lib.PFAC_dumpTransitionTable(self._h, fp)
        finally:
            _libc.fclose(fp)
        return self._ret(st, "PFAC_dumpTransitionTable", check)

    # -- matching ------------------------------------------------------------------
    def matchFromDevice(self, d_input: int, size: int, d_result: int, check: bool = True) -> int:
        return self._ret(self._lib.PFAC_matchFromDevice(self._h, d_input, size, d_result),
                         "PFAC_matchFromDevice", check)

    def matchFromHost(self, h_input: int, size: int, h_result: int, check: bool = True) -> int:
        return self._ret(self._lib.PFAC_matchFromHost(self._h, h_input, size, h_result),
                         "PFAC_matchFromHost", check)

    def matchFromDeviceReduce(self, d_input: int, size: int, d_result: int, d_pos: int, check: bool = True):
        n = C.c_int(0)
        st = self._lib.PFAC_matchFromDeviceReduce(self._h, d_input, size, d_result, d_pos, C.byref(n))
        return self._ret(st, "PFAC_matchFromDeviceReduce", check), n.value

    def matchFromHostReduce(self, h_input: int, size: int, h_result: int, h_pos: int, check: bool = True):
        n = C.c_int(0)
        st = self._lib.PFAC_matchFromHostReduce(self._h, h_input, size, h_result, h_pos, C.byref(n))
        return self._ret(st, "PFAC_matchFromHostReduce", check), n.value

    # -- batches of independent segments (include/pfac_ext.h: PFACX_matchBatch*) ------
    def matchBatchFromDevice(self, d_input: int, size: int, d_offsets: int, num_segments: int, d_result: int, check: bool = True) -> int:
        """``PFACX_matchBatchFromDevice``: `d_offsets` = device address of num_segments + 1 size_t offsets."""
        return self._ret(self._lib.PFACX_matchBatchFromDevice(self._h, d_input, size, d_offsets, num_segments, d_result),
                         "PFACX_matchBatchFromDevice", check)

    def matchBatchFromHost(self, h_input: int, size: int, h_offsets: int, num_segments: int, h_result: int, check: bool = True) -> int:
        """``PFACX_matchBatchFromHost``: `h_offsets` = host address of num_segments + 1 size_t offsets (validated)."""
        return self._ret(self._lib.PFACX_matchBatchFromHost(self._h, h_input, size, h_offsets, num_segments, h_result),
                         "PFACX_matchBatchFromHost", check)

    def matchBatchFromDeviceReduce(self, d_input: int, size: int, d_offsets: int, num_segments: int, d_result: int, d_pos: int,
                                   d_seg_first: int, check: bool = True):
        """``PFACX_matchBatchFromDeviceReduce`` -> (status, number of pairs); `d_seg_first` receives num_segments + 1 ints."""
        n = C.c_int(0)
        st = self._lib.PFACX_matchBatchFromDeviceReduce(self._h, d_input, size, d_offsets, num_segments, d_result, d_pos, d_seg_first, C.byref(n))
        return self._ret(st, "PFACX_matchBatchFromDeviceReduce", check), n.value

    def match_batch_host_array(self, data, offsets):
        """matchBatchFromHost over numpy arrays: `offsets` = the num_segments + 1 segment offsets."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        out = np.full(data.size, -7, dtype=np.int32)   # poison: every element must be written
        if data.size:
            self.matchBatchFromHost(data.ctypes.data, data.size, offs.ctypes.data, offs.size - 1, out.ctypes.data)
        return out

    # -- every pattern at a position (include/pfac_ext.h: PFACX_matchAll*) ---------------
    def matchAllFromDevice(self, d_input: int, size: int, d_ids: int, d_pos: int, capacity: int, check: bool = True):
        """``PFACX_matchAllFromDevice`` -> (status, full length of the list).  OUTPUT_TRUNCATED is returned, not raised."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_matchAllFromDevice(self._h, d_input, size, d_ids, d_pos, capacity, C.byref(n))
        return self._ret(st, "PFACX_matchAllFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def matchAllFromHost(self, h_input: int, size: int, h_ids: int, h_pos: int, capacity: int, check: bool = True):
        """``PFACX_matchAllFromHost`` -> (status, full length of the list).  OUTPUT_TRUNCATED is returned, not raised."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_matchAllFromHost(self._h, h_input, size, h_ids, h_pos, capacity, C.byref(n))
        return self._ret(st, "PFACX_matchAllFromHost", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def matchAllBatchFromDevice(self, d_input: int, size: int, d_offsets: int, num_segments: int, d_ids: int, d_pos: int, capacity: int,
                                d_seg_first: int, check: bool = True):
        """``PFACX_matchAllBatchFromDevice`` -> (status, full length); `d_seg_first` receives num_segments + 1 size_t."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_matchAllBatchFromDevice(self._h, d_input, size, d_offsets, num_segments, d_ids, d_pos, capacity, d_seg_first,
                                                     C.byref(n))
        return self._ret(st, "PFACX_matchAllBatchFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def match_all_host_array(self, data, capacity=None):
        """matchAllFromHost over a numpy array -> (pos, ids) of every match, ascending position, longest first within one.
        capacity=None: size * maxMatchesPerPosition (never truncates); a smaller capacity that truncates raises PFACError."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if data.size == 0:
            return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
        cap = data.size * max(1, int(self.info().maxMatchesPerPosition)) if capacity is None else int(capacity)
        ids = np.full(cap, -7, dtype=np.int32)
        pos = np.full(cap, -7, dtype=np.int32)
        st, n = self.matchAllFromHost(data.ctypes.data, data.size, ids.ctypes.data, pos.ctypes.data, cap, check=False)
        self._ret(st, "PFACX_matchAllFromHost", True)
        return pos[:n].copy(), ids[:n].copy()

    # -- the lines that contain a pattern (include/pfac_ext.h: PFACX_matchLines*) ------------
    def matchLinesFromDevice(self, d_input: int, size: int, flags: int, d_line_start: int, d_line_len: int, d_line_index, capacity: int,
                             check: bool = True):
        """``PFACX_matchLinesFromDevice`` -> (status, number of lines, number of selected lines); `d_line_index` may be None."""
        nl, ns = C.c_size_t(0), C.c_size_t(0)
        st = self._lib.PFACX_matchLinesFromDevice(self._h, d_input, size, flags, d_line_start, d_line_len, d_line_index, capacity,
                                                  C.byref(nl), C.byref(ns))
        return self._ret(st, "PFACX_matchLinesFromDevice", check), nl.value, ns.value

    def matchLinesFromHost(self, h_input: int, size: int, flags: int, h_line_start: int, h_line_len: int, h_line_index, capacity: int,
                           check: bool = True):
        """``PFACX_matchLinesFromHost`` -> (status, number of lines, number of selected lines); `h_line_index` may be None."""
        nl, ns = C.c_size_t(0), C.c_size_t(0)
        st = self._lib.PFACX_matchLinesFromHost(self._h, h_input, size, flags, h_line_start, h_line_len, h_line_index, capacity,
                                                C.byref(nl), C.byref(ns))
        return self._ret(st, "PFACX_matchLinesFromHost", check), nl.value, ns.value

    def gatherLinesFromDevice(self, d_input: int, size: int, d_line_start: int, d_line_len: int, num_selected: int, d_out, out_capacity: int,
                              check: bool = True):
        """``PFACX_gatherLinesFromDevice`` -> (status, size of the whole text).  OUTPUT_TRUNCATED is returned, not raised."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_gatherLinesFromDevice(self._h, d_input, size, d_line_start, d_line_len, num_selected, d_out, out_capacity, C.byref(n))
        return self._ret(st, "PFACX_gatherLinesFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def match_lines_host_array(self, data, invert: bool = False):
        """matchLinesFromHost over a numpy array -> (number of lines, line_start, line_len, line_index) of the lines that contain a
        pattern (invert: that contain none), ascending."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        cap = max(1, data.size)
        start = np.full(cap, -7, dtype=np.int32)
        length = np.full(cap, -7, dtype=np.int32)
        index = np.full(cap, -7, dtype=np.int32)
        _, nl, ns = self.matchLinesFromHost(data.ctypes.data if data.size else start.ctypes.data, data.size, PFACX_LINES_INVERT if invert else 0,
                                            start.ctypes.data, length.ctypes.data, index.ctypes.data, cap)
        return nl, start[:ns].copy(), length[:ns].copy(), index[:ns].copy()

    # -- the lines around the selected lines (include/pfac_ext.h: PFACX_matchLinesContext*) ------------
    def _lines_context(self, name, input_, size, flags, before, after, line_start, line_len, line_index, line_tag, capacity, check):
        nl, ns, nm, ng = (C.c_size_t(0) for _ in range(4))
        st = getattr(self._lib, name)(self._h, input_, size, flags, before, after, line_start, line_len, line_index, line_tag, capacity,
                                      C.byref(nl), C.byref(ns), C.byref(nm), C.byref(ng))
        return self._ret(st, name, check), nl.value, ns.value, nm.value, ng.value

    def matchLinesContextFromDevice(self, d_input: int, size: int, flags: int, before: int, after: int, d_line_start: int, d_line_len: int,
                                    d_line_index, d_line_tag, capacity: int, check: bool = True):
        """``PFACX_matchLinesContextFromDevice`` -> (status, lines, selected lines, matching lines, groups); `d_line_index` and
        `d_line_tag` may be None."""
        return self._lines_context("PFACX_matchLinesContextFromDevice", d_input, size, flags, before, after, d_line_start, d_line_len,
                                   d_line_index, d_line_tag, capacity, check)

    def matchLinesContextFromHost(self, h_input: int, size: int, flags: int, before: int, after: int, h_line_start: int, h_line_len: int,
                                  h_line_index, h_line_tag, capacity: int, check: bool = True):
        """``PFACX_matchLinesContextFromHost`` -> (status, lines, selected lines, matching lines, groups); `h_line_index` and
        `h_line_tag` may be None."""
        return self._lines_context("PFACX_matchLinesContextFromHost", h_input, size, flags, before, after, h_line_start, h_line_len,
                                   h_line_index, h_line_tag, capacity, check)

    def match_lines_context_host_array(self, data, before: int = 0, after: int = 0, invert: bool = False):
        """matchLinesContextFromHost over a numpy array -> (line_start, line_len, line_index, line_tag, (lines, selected, matching, groups)):
        the lines within `before` in front of and `after` behind a line that contains a pattern (invert: that contains none), ascending;
        line_tag = group << 1 | (1 for such a line itself, 0 for context)."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        cap = max(1, data.size)
        start, length, index, tag = (np.full(cap, -7, dtype=np.int32) for _ in range(4))
        _, nl, ns, nm, ng = self.matchLinesContextFromHost(data.ctypes.data if data.size else start.ctypes.data, data.size,
                                                           PFACX_LINES_INVERT if invert else 0, before, after, start.ctypes.data,
                                                           length.ctypes.data, index.ctypes.data, tag.ctypes.data, cap)
        return start[:ns].copy(), length[:ns].copy(), index[:ns].copy(), tag[:ns].copy(), (nl, ns, nm, ng)

    # -- the bytes that belong to a match, and their redaction (include/pfac_ext.h: PFACX_matchSpans*) ------------
    def matchSpansFromDevice(self, d_input: int, size: int, d_span_start: int, d_span_len: int, capacity: int, check: bool = True):
        """``PFACX_matchSpansFromDevice`` -> (status, number of spans, covered bytes)."""
        ns, cb = C.c_size_t(0), C.c_size_t(0)
        st = self._lib.PFACX_matchSpansFromDevice(self._h, d_input, size, d_span_start, d_span_len, capacity, C.byref(ns), C.byref(cb))
        return self._ret(st, "PFACX_matchSpansFromDevice", check), ns.value, cb.value

    def matchSpansFromHost(self, h_input: int, size: int, h_span_start: int, h_span_len: int, capacity: int, check: bool = True):
        """``PFACX_matchSpansFromHost`` -> (status, number of spans, covered bytes); follows PFAC_setPlatform."""
        ns, cb = C.c_size_t(0), C.c_size_t(0)
        st = self._lib.PFACX_matchSpansFromHost(self._h, h_input, size, h_span_start, h_span_len, capacity, C.byref(ns), C.byref(cb))
        return self._ret(st, "PFACX_matchSpansFromHost", check), ns.value, cb.value

    def redactSpansFromDevice(self, d_input: int, size: int, d_span_start, d_span_len, num_spans: int, fill: int, d_out: int,
                              check: bool = True) -> int:
        """``PFACX_redactSpansFromDevice``: asynchronous on the default stream; ``d_out == d_input`` redacts in place."""
        return self._ret(self._lib.PFACX_redactSpansFromDevice(self._h, d_input, size, d_span_start, d_span_len, num_spans, fill & 0xFF, d_out),
                         "PFACX_redactSpansFromDevice", check)

    def match_spans_host_array(self, data):
        """matchSpansFromHost over a numpy array -> (span_start, span_len, covered bytes), ascending."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        cap = max(1, data.size)
        start = np.full(cap, -7, dtype=np.int32)
        length = np.full(cap, -7, dtype=np.int32)
        _, ns, cb = self.matchSpansFromHost(data.ctypes.data if data.size else start.ctypes.data, data.size, start.ctypes.data, length.ctypes.data, cap)
        return start[:ns].copy(), length[:ns].copy(), cb

    # -- an unsorted interval list as covered spans (include/pfac_ext.h: PFACX_coverSpans*) ------------
    def coverSpansFromDevice(self, d_start, d_end, num_intervals: int, size: int, flags: int, d_span_start, d_span_len, capacity: int,
                             check: bool = True):
        """``PFACX_coverSpansFromDevice`` -> (status, number of spans, covered bytes); the interval arrays may be None with no interval, the
        span arrays with capacity 0 (the count query).  ``PFACX_STATUS_OUTPUT_TRUNCATED`` is returned, not raised: both counts are complete."""
        ns, cb = C.c_size_t(0), C.c_size_t(0)
        st = self._lib.PFACX_coverSpansFromDevice(self._h, d_start, d_end, num_intervals, size, flags, d_span_start, d_span_len, capacity,
                                                  C.byref(ns), C.byref(cb))
        return self._ret(st, "PFACX_coverSpansFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), ns.value, cb.value

    def coverSpansFromHost(self, h_start, h_end, num_intervals: int, size: int, flags: int, h_span_start, h_span_len, capacity: int,
                           check: bool = True):
        """``PFACX_coverSpansFromHost`` -> (status, number of spans, covered bytes); runs on the CPU on every platform."""
        ns, cb = C.c_size_t(0), C.c_size_t(0)
        st = self._lib.PFACX_coverSpansFromHost(self._h, h_start, h_end, num_intervals, size, flags, h_span_start, h_span_len, capacity,
                                                C.byref(ns), C.byref(cb))
        return self._ret(st, "PFACX_coverSpansFromHost", check and st != STATUS.OUTPUT_TRUNCATED), ns.value, cb.value

    def cover_spans_host_array(self, starts, ends, size: int, lengths: bool = False):
        """coverSpansFromHost over two numpy arrays -> (span_start, span_len, covered bytes), ascending; `lengths`: `ends` holds lengths."""
        import numpy as np
        starts = np.ascontiguousarray(starts, dtype=np.int32)
        ends = np.ascontiguousarray(ends, dtype=np.int32)
        if starts.shape != ends.shape or starts.ndim != 1:
            raise ValueError("cover_spans_host_array: starts and ends must be one-dimensional and of one length")
        flags = PFACX_COVER_LENGTHS if lengths else 0
        n = int(starts.size)
        _, ns, _ = self.coverSpansFromHost(starts.ctypes.data if n else None, ends.ctypes.data if n else None, n, size, flags, None, None, 0)
        start = np.full(max(1, ns), -7, dtype=np.int32)
        length = np.full(max(1, ns), -7, dtype=np.int32)
        _, ns, cb = self.coverSpansFromHost(starts.ctypes.data if n else None, ends.ctypes.data if n else None, n, size, flags,
                                            start.ctypes.data, length.ctypes.data, ns)
        return start[:ns].copy(), length[:ns].copy(), cb

    # -- a hit list in start order (include/pfac_ext.h: PFACX_orderHits*) ------------
    def orderHitsFromDevice(self, d_start, d_ids, d_end, d_aux, num_hits: int, flags: int, d_perm=None, check: bool = True):
        """``PFACX_orderHitsFromDevice`` -> (status, was_ordered); every array but `d_start` may be None, `d_start` too with no hit.  The given
        columns are permuted in place; `d_perm` receives the incoming index of the entry now at k."""
        was = C.c_int(-1)
        st = self._lib.PFACX_orderHitsFromDevice(self._h, d_start, d_ids, d_end, d_aux, num_hits, flags, d_perm, C.byref(was))
        return self._ret(st, "PFACX_orderHitsFromDevice", check), was.value

    def orderHitsFromHost(self, h_start, h_ids, h_end, h_aux, num_hits: int, flags: int, h_perm=None, check: bool = True):
        """``PFACX_orderHitsFromHost`` -> (status, was_ordered); runs on the CPU on every platform."""
        was = C.c_int(-1)
        st = self._lib.PFACX_orderHitsFromHost(self._h, h_start, h_ids, h_end, h_aux, num_hits, flags, h_perm, C.byref(was))
        return self._ret(st, "PFACX_orderHitsFromHost", check), was.value

    def order_hits_host_array(self, starts, ids=None, ends=None, aux=None, ties_by_id: bool = False):
        """orderHitsFromHost over copies of numpy arrays -> (the given columns in start order ..., perm, was_ordered): `starts` first, then
        whichever of `ids`, `ends`, `aux` is given, in that order."""
        import numpy as np
        cols = [np.array(c, dtype=np.int32, ndmin=1, copy=True) for c in (starts, ids, ends, aux) if c is not None]
        if starts is None or any(c.ndim != 1 or c.shape != cols[0].shape for c in cols):
            raise ValueError("order_hits_host_array: starts is required, and every column must be one-dimensional and of one length")
        n = int(cols[0].size)
        perm = np.full(n, -7, dtype=np.int32)
        ptrs = iter([c.ctypes.data if n else None for c in cols])
        args = [next(ptrs) if c is not None else None for c in (starts, ids, ends, aux)]
        _, was = self.orderHitsFromHost(args[0], args[1], args[2], args[3], n, PFACX_ORDER_TIES_BY_ID if ties_by_id else 0,
                                        perm.ctypes.data if n else None)
        return (*cols, perm, was)

    # -- which patterns occurred, and how often (include/pfac_ext.h: PFACX_count*) ------------
    def countFromDevice(self, d_input: int, size: int, flags: int, d_counts: int, num_counts: int, check: bool = True):
        """``PFACX_countFromDevice`` -> (status, what the call added); `d_counts`: num_counts >= F + 1 ``unsigned long long`` by pattern id."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_countFromDevice(self._h, d_input, size, flags, d_counts, num_counts, C.byref(n))
        return self._ret(st, "PFACX_countFromDevice", check), n.value

    def countFromHost(self, h_input: int, size: int, flags: int, h_counts: int, num_counts: int, check: bool = True):
        """``PFACX_countFromHost`` -> (status, what the call added); follows PFAC_setPlatform."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_countFromHost(self._h, h_input, size, flags, h_counts, num_counts, C.byref(n))
        return self._ret(st, "PFACX_countFromHost", check), n.value

    def countPairsFromDevice(self, d_ids, num_pairs: int, flags: int, d_counts: int, num_counts: int, check: bool = True) -> int:
        """``PFACX_countPairsFromDevice``: the counts of a LONGEST id list (with PFACX_COUNT_LONGEST: of any id list); asynchronous on the
        default stream."""
        return self._ret(self._lib.PFACX_countPairsFromDevice(self._h, d_ids, num_pairs, flags, d_counts, num_counts), "PFACX_countPairsFromDevice", check)

    def countNonzeroFromDevice(self, d_counts, num_counts: int, d_ids, d_out_counts, capacity: int, check: bool = True):
        """``PFACX_countNonzeroFromDevice`` -> (status, distinct ids, sum of the counts).  OUTPUT_TRUNCATED is returned, not raised."""
        nd, total = C.c_size_t(0), C.c_ulonglong(0)
        st = self._lib.PFACX_countNonzeroFromDevice(self._h, d_counts, num_counts, d_ids, d_out_counts, capacity, C.byref(nd), C.byref(total))
        return self._ret(st, "PFACX_countNonzeroFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), nd.value, total.value

    def count_host_array(self, data, longest: bool = False):
        """countFromHost over a numpy array -> (counts by pattern id as uint64[F + 1], what the call added): every occurrence of every
        pattern (longest: one pattern per position)."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        counts = np.full(int(self.info().numOfPatterns) + 1, 0xDEAD, dtype=np.uint64)
        buf = data if data.size else np.zeros(1, dtype=np.uint8)
        _, total = self.countFromHost(buf.ctypes.data, data.size, PFACX_COUNT_LONGEST if longest else 0, counts.ctypes.data, counts.size)
        return counts, total

    # -- how often each pattern occurred in each segment, in CSR form (include/pfac_ext.h: PFACX_countBatch*) ------------
    def _count_batch(self, name: str, items, num_items: int, offsets, num_segments: int, flags: int, ids, counts, capacity: int, seg_first,
                     check: bool):
        n, total = C.c_size_t(0), C.c_ulonglong(0)
        st = getattr(self._lib, name)(self._h, items, num_items, offsets, num_segments, flags, ids, counts, capacity, seg_first, C.byref(n),
                                      C.byref(total))
        return self._ret(st, name, check and st != STATUS.OUTPUT_TRUNCATED), n.value, total.value

    def countBatchFromDevice(self, d_input: int, size: int, d_offsets, num_segments: int, flags: int, d_ids, d_counts, capacity: int, d_seg_first,
                             check: bool = True):
        """``PFACX_countBatchFromDevice`` -> (status, full length of the count list, sum of all counts): `d_offsets` (num_segments + 1 ``size_t``,
        device) may be None with one segment, `d_ids` (int) / `d_counts` (unsigned int) may be None with capacity 0, `d_seg_first`
        (num_segments + 1 ``size_t``, device) is the row pointer.  OUTPUT_TRUNCATED is returned, not raised."""
        return self._count_batch("PFACX_countBatchFromDevice", d_input, size, d_offsets, num_segments, flags, d_ids, d_counts, capacity, d_seg_first, check)

    def countBatchFromHost(self, h_input: int, size: int, h_offsets, num_segments: int, flags: int, h_ids, h_counts, capacity: int, h_seg_first,
                           check: bool = True):
        """``PFACX_countBatchFromHost``: the same over host memory; follows PFAC_setPlatform."""
        return self._count_batch("PFACX_countBatchFromHost", h_input, size, h_offsets, num_segments, flags, h_ids, h_counts, capacity, h_seg_first, check)

    def countBatchPairsFromDevice(self, d_pair_ids, num_pairs: int, d_seg_first_pairs, num_segments: int, flags: int, d_ids, d_counts, capacity: int,
                                  d_seg_first, check: bool = True):
        """``PFACX_countBatchPairsFromDevice``: the same list from a LONGEST id list the caller already has and the first pair of each segment
        (num_segments + 1 ``int``, device): the output of matchBatchFromDeviceReduce or of a flows call."""
        return self._count_batch("PFACX_countBatchPairsFromDevice", d_pair_ids, num_pairs, d_seg_first_pairs, num_segments, flags, d_ids, d_counts,
                                 capacity, d_seg_first, check)

    def count_batch_host_array(self, data, offsets=None, longest: bool = False):
        """countBatchFromHost over numpy arrays -> (segFirst, ids, counts, total) of the whole count list: the count query first, then arrays of
        exactly that length; offsets=None: the buffer is one segment."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uintp)
        segments = 1 if off is None else off.size - 1
        first = np.full(segments + 1, 0xDEAD, dtype=np.uintp)
        buf = data if data.size else np.zeros(1, dtype=np.uint8)
        optr = None if off is None else off.ctypes.data
        flags = PFACX_COUNT_LONGEST if longest else 0
        st, n, total = self.countBatchFromHost(buf.ctypes.data, data.size, optr, segments, flags, None, None, 0, first.ctypes.data)    # the count query
        if st not in (0, STATUS.OUTPUT_TRUNCATED):                                 # (a list that does not fit capacity 0: what a query returns)
            raise PFACError(st, "PFACX_countBatchFromHost", error_string(st))
        ids = np.full(max(1, n), -7, dtype=np.int32)
        counts = np.full(max(1, n), 0xDEAD, dtype=np.uint32)
        st, n2, total2 = self.countBatchFromHost(buf.ctypes.data, data.size, optr, segments, flags, ids.ctypes.data, counts.ctypes.data, n,
                                                 first.ctypes.data)
        if st != 0 or n2 != n or total2 != total:                                  # (truncated now: the list grew between the two calls)
            raise PFACError(st, "PFACX_countBatchFromHost", f"{n2} entries and a total of {total2} behind a count query that said {n} and {total}")
        return first, ids[:n].copy(), counts[:n].copy(), total

    # -- disjoint leftmost-longest matches and their replacement (include/pfac_ext.h: PFACX_matchDisjoint* / PFACX_replace*) ----
    def matchDisjointFromDevice(self, d_input: int, size: int, d_ids: int, d_pos: int, capacity: int, check: bool = True):
        """``PFACX_matchDisjointFromDevice`` -> (status, number of tokens, covered bytes)."""
        nt, cb = C.c_size_t(0), C.c_size_t(0)
        st = self._lib.PFACX_matchDisjointFromDevice(self._h, d_input, size, d_ids, d_pos, capacity, C.byref(nt), C.byref(cb))
        return self._ret(st, "PFACX_matchDisjointFromDevice", check), nt.value, cb.value

    def matchDisjointFromHost(self, h_input: int, size: int, h_ids: int, h_pos: int, capacity: int, check: bool = True):
        """``PFACX_matchDisjointFromHost`` -> (status, number of tokens, covered bytes); follows PFAC_setPlatform."""
        nt, cb = C.c_size_t(0), C.c_size_t(0)
        st = self._lib.PFACX_matchDisjointFromHost(self._h, h_input, size, h_ids, h_pos, capacity, C.byref(nt), C.byref(cb))
        return self._ret(st, "PFACX_matchDisjointFromHost", check), nt.value, cb.value

    def replaceFromDevice(self, d_input: int, size: int, d_ids, d_pos, num_tokens: int, d_repl_off, num_off: int, d_repl_bytes, repl_bytes: int,
                          d_out, out_capacity: int, check: bool = True):
        """``PFACX_replaceFromDevice`` -> (status, size of the whole text).  OUTPUT_TRUNCATED is returned, not raised."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_replaceFromDevice(self._h, d_input, size, d_ids, d_pos, num_tokens, d_repl_off, num_off, d_repl_bytes, repl_bytes,
                                               d_out, out_capacity, C.byref(n))
        return self._ret(st, "PFACX_replaceFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def replaceFromHost(self, h_input: int, size: int, h_ids, h_pos, num_tokens: int, h_repl_off, num_off: int, h_repl_bytes, repl_bytes: int,
                        h_out, out_capacity: int, check: bool = True):
        """``PFACX_replaceFromHost`` -> (status, size of the whole text).  OUTPUT_TRUNCATED is returned, not raised."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_replaceFromHost(self._h, h_input, size, h_ids, h_pos, num_tokens, h_repl_off, num_off, h_repl_bytes, repl_bytes,
                                             h_out, out_capacity, C.byref(n))
        return self._ret(st, "PFACX_replaceFromHost", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    # -- whole-word and delimiter-bounded matches (include/pfac_ext.h: PFACX_matchWords*) ----------------
    def matchWordsFromDevice(self, d_input: int, size: int, cls, flags: int, d_ids: int, d_pos: int, capacity: int, check: bool = True):
        """``PFACX_matchWordsFromDevice`` -> (status, full length of the list); `cls`: word_class(...), bytes, or None for [0-9A-Za-z_].
        OUTPUT_TRUNCATED is returned, not raised."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_matchWordsFromDevice(self._h, d_input, size, _class_arg(cls), flags, d_ids, d_pos, capacity, C.byref(n))
        return self._ret(st, "PFACX_matchWordsFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def matchWordsFromHost(self, h_input: int, size: int, cls, flags: int, h_ids: int, h_pos: int, capacity: int, check: bool = True):
        """``PFACX_matchWordsFromHost`` -> (status, full length of the list); follows PFAC_setPlatform.  OUTPUT_TRUNCATED is returned, not raised."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_matchWordsFromHost(self._h, h_input, size, _class_arg(cls), flags, h_ids, h_pos, capacity, C.byref(n))
        return self._ret(st, "PFACX_matchWordsFromHost", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def wordsPairsFromDevice(self, d_input: int, size: int, cls, flags: int, d_pair_ids, d_pair_pos, num_pairs: int, d_ids, d_pos, capacity: int,
                             check: bool = True):
        """``PFACX_wordsPairsFromDevice`` -> (status, full length of the list): the bounded occurrences of a LONGEST pair list the caller
        already has.  OUTPUT_TRUNCATED is returned, not raised."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_wordsPairsFromDevice(self._h, d_input, size, _class_arg(cls), flags, d_pair_ids, d_pair_pos, num_pairs, d_ids, d_pos,
                                                  capacity, C.byref(n))
        return self._ret(st, "PFACX_wordsPairsFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def match_words_host_array(self, data, cls=None, all_matches: bool = False, capacity=None):
        """matchWordsFromHost over a numpy array -> (pos, ids), ascending position.  capacity=None: size * maxMatchesPerPosition (never
        truncates); a smaller capacity that truncates raises PFACError."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if data.size == 0:
            return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
        cap = data.size * max(1, int(self.info().maxMatchesPerPosition)) if capacity is None else int(capacity)
        ids = np.full(cap, -7, dtype=np.int32)
        pos = np.full(cap, -7, dtype=np.int32)
        st, n = self.matchWordsFromHost(data.ctypes.data, data.size, cls, PFACX_WORDS_ALL if all_matches else 0, ids.ctypes.data, pos.ctypes.data, cap,
                                        check=False)
        self._ret(st, "PFACX_matchWordsFromHost", True)
        return pos[:n].copy(), ids[:n].copy()

    # -- the offsets that cut a buffer into segments at a delimiter class (include/pfac_ext.h: PFACX_split*) ----------------
    def _split(self, name: str, input_, size: int, cls, flags: int, offsets, capacity: int, want_longest: bool, check: bool):
        n, longest = C.c_size_t(0), C.c_size_t(0)
        st = getattr(self._lib, name)(self._h, input_, size, _class_arg(cls), flags, offsets, capacity, C.byref(n),
                                      C.byref(longest) if want_longest else None)
        return self._ret(st, name, check and st != STATUS.OUTPUT_TRUNCATED), n.value, longest.value

    def splitFromDevice(self, d_input: int, size: int, cls, flags: int, d_offsets, capacity: int, want_longest: bool = True, check: bool = True):
        """``PFACX_splitFromDevice`` -> (status, number of segments, longest segment); `cls`: word_class(...), bytes, or None for {'\n'};
        `d_offsets` (``size_t``, device) may be None with capacity 0: the count query.  OUTPUT_TRUNCATED is returned, not raised."""
        return self._split("PFACX_splitFromDevice", d_input, size, cls, flags, d_offsets, capacity, want_longest, check)

    def splitFromHost(self, h_input: int, size: int, cls, flags: int, h_offsets, capacity: int, want_longest: bool = True, check: bool = True):
        """``PFACX_splitFromHost``: the same over host memory, a host loop on every platform."""
        return self._split("PFACX_splitFromHost", h_input, size, cls, flags, h_offsets, capacity, want_longest, check)

    def split_host_array(self, data, cls=None, before: bool = False, runs: bool = False):
        """splitFromHost over a numpy array -> (offsets as a numpy ``uint64`` array of numSegments + 1 entries -- empty for empty data --, the longest
        segment): the count query first, then an array of exactly that length."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        buf = data if data.size else np.zeros(1, dtype=np.uint8)
        flags = (PFACX_SPLIT_BEFORE if before else 0) | (PFACX_SPLIT_RUNS if runs else 0)
        st, n, longest = self.splitFromHost(buf.ctypes.data, data.size, cls, flags, None, 0)                   # the count query
        if data.size == 0:
            return np.zeros(0, dtype=np.uint64), longest
        offsets = np.full(n + 1, 0xDEAD, dtype=np.uint64)
        st, n2, longest2 = self.splitFromHost(buf.ctypes.data, data.size, cls, flags, offsets.ctypes.data, offsets.size)
        if st != 0 or n2 != n or longest2 != longest:
            raise PFACError(st, "PFACX_splitFromHost", f"{n2} segments, the longest {longest2}, behind a count query that said {n} and {longest}")
        return offsets, longest

    # -- the record and the column of every match (include/pfac_ext.h: PFACX_locatePairs*, PFACX_matchLocated*) ----------------
    def _locate_pairs(self, name: str, input_, size: int, cls, flags: int, pos, num_pairs: int, record, column, want_records: bool, check: bool):
        n = C.c_size_t(0)
        st = getattr(self._lib, name)(self._h, input_, size, _class_arg(cls), flags, pos, num_pairs, record, column,
                                      C.byref(n) if want_records else None)
        return self._ret(st, name, check), n.value

    def locatePairsFromDevice(self, d_input: int, size: int, cls, flags: int, d_pos, num_pairs: int, d_record, d_column,
                              want_records: bool = True, check: bool = True):
        """``PFACX_locatePairsFromDevice`` -> (status, number of records); `cls`: word_class(...), bytes, or None for {'\n'}; `d_pos`,
        `d_record`, `d_column` (``int``, device; `d_column` may be None): num_pairs entries each."""
        return self._locate_pairs("PFACX_locatePairsFromDevice", d_input, size, cls, flags, d_pos, num_pairs, d_record, d_column, want_records, check)

    def locatePairsFromHost(self, h_input: int, size: int, cls, flags: int, h_pos, num_pairs: int, h_record, h_column,
                            want_records: bool = True, check: bool = True):
        """``PFACX_locatePairsFromHost``: the same over host memory, a host loop on every platform."""
        return self._locate_pairs("PFACX_locatePairsFromHost", h_input, size, cls, flags, h_pos, num_pairs, h_record, h_column, want_records, check)

    def _match_located(self, name: str, input_, size: int, cls, flags: int, ids, pos, record, column, loc_capacity: int, check: bool):
        n = C.c_int(0)
        st = getattr(self._lib, name)(self._h, input_, size, _class_arg(cls), flags, ids, pos, record, column, loc_capacity, C.byref(n))
        return self._ret(st, name, check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def matchLocatedFromDevice(self, d_input: int, size: int, cls, flags: int, d_ids, d_pos, d_record, d_column, loc_capacity: int,
                               check: bool = True):
        """``PFACX_matchLocatedFromDevice`` -> (status, number of pairs): `d_ids`, `d_pos` size entries each as for matchFromDeviceReduce,
        `d_record`, `d_column` (may be None) loc_capacity entries each.  OUTPUT_TRUNCATED is returned, not raised."""
        return self._match_located("PFACX_matchLocatedFromDevice", d_input, size, cls, flags, d_ids, d_pos, d_record, d_column, loc_capacity, check)

    def matchLocatedFromHost(self, h_input: int, size: int, cls, flags: int, h_ids, h_pos, h_record, h_column, loc_capacity: int,
                             check: bool = True):
        """``PFACX_matchLocatedFromHost``: the same over host memory; follows PFAC_setPlatform."""
        return self._match_located("PFACX_matchLocatedFromHost", h_input, size, cls, flags, h_ids, h_pos, h_record, h_column, loc_capacity, check)

    def locate_host_array(self, data, positions, cls=None, before: bool = False, runs: bool = False):
        """locatePairsFromHost over numpy arrays -> (records, columns, number of records): `positions` non-decreasing ``int32``."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        pos = np.ascontiguousarray(positions, dtype=np.int32)
        buf = data if data.size else np.zeros(1, dtype=np.uint8)
        flags = (PFACX_SPLIT_BEFORE if before else 0) | (PFACX_SPLIT_RUNS if runs else 0)
        record = np.full(max(pos.size, 1), -7, dtype=np.int32)
        column = np.full(max(pos.size, 1), -7, dtype=np.int32)
        st, n = self.locatePairsFromHost(buf.ctypes.data, data.size, cls, flags, pos.ctypes.data if pos.size else None, pos.size,
                                         record.ctypes.data, column.ctypes.data)
        return record[:pos.size], column[:pos.size], n

    # -- the value behind every match (include/pfac_ext.h: PFACX_capturePairs*, PFACX_matchCaptured*) ----------------
    def _capture_pairs(self, name: str, input_, size: int, skip, stop, window: int, flags: int, ids, pos, num_pairs: int, val_start, val_len, check: bool):
        st = getattr(self._lib, name)(self._h, input_, size, _class_arg(skip), _class_arg(stop), window, flags, ids, pos, num_pairs, val_start, val_len)
        return self._ret(st, name, check)

    def capturePairsFromDevice(self, d_input: int, size: int, skip, stop, window: int, flags: int, d_ids, d_pos, num_pairs: int, d_val_start,
                               d_val_len, check: bool = True) -> int:
        """``PFACX_capturePairsFromDevice`` -> status; `skip`, `stop`: word_class(...), bytes, or None (the empty class; {'\n'}); `window` 0:
        unbounded; `d_ids` (may be None with PFACX_CAPTURE_AT_POS), `d_pos`, `d_val_start`, `d_val_len` (``int``, device): num_pairs entries each."""
        return self._capture_pairs("PFACX_capturePairsFromDevice", d_input, size, skip, stop, window, flags, d_ids, d_pos, num_pairs, d_val_start,
                                   d_val_len, check)

    def capturePairsFromHost(self, h_input: int, size: int, skip, stop, window: int, flags: int, h_ids, h_pos, num_pairs: int, h_val_start,
                             h_val_len, check: bool = True) -> int:
        """``PFACX_capturePairsFromHost``: the same over host memory, a host loop on every platform."""
        return self._capture_pairs("PFACX_capturePairsFromHost", h_input, size, skip, stop, window, flags, h_ids, h_pos, num_pairs, h_val_start,
                                   h_val_len, check)

    def _match_captured(self, name: str, input_, size: int, skip, stop, window: int, flags: int, ids, pos, val_start, val_len, cap_capacity: int,
                        check: bool):
        n = C.c_int(0)
        st = getattr(self._lib, name)(self._h, input_, size, _class_arg(skip), _class_arg(stop), window, flags, ids, pos, val_start, val_len,
                                      cap_capacity, C.byref(n))
        return self._ret(st, name, check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def matchCapturedFromDevice(self, d_input: int, size: int, skip, stop, window: int, flags: int, d_ids, d_pos, d_val_start, d_val_len,
                                cap_capacity: int, check: bool = True):
        """``PFACX_matchCapturedFromDevice`` -> (status, number of pairs): `d_ids`, `d_pos` size entries each as for matchFromDeviceReduce,
        `d_val_start`, `d_val_len` cap_capacity entries each.  OUTPUT_TRUNCATED is returned, not raised."""
        return self._match_captured("PFACX_matchCapturedFromDevice", d_input, size, skip, stop, window, flags, d_ids, d_pos, d_val_start, d_val_len,
                                    cap_capacity, check)

    def matchCapturedFromHost(self, h_input: int, size: int, skip, stop, window: int, flags: int, h_ids, h_pos, h_val_start, h_val_len,
                              cap_capacity: int, check: bool = True):
        """``PFACX_matchCapturedFromHost``: the same over host memory; follows PFAC_setPlatform."""
        return self._match_captured("PFACX_matchCapturedFromHost", h_input, size, skip, stop, window, flags, h_ids, h_pos, h_val_start, h_val_len,
                                    cap_capacity, check)

    # -- input that arrives in pieces (include/pfac_ext.h: PFACX_stream*) ----------------
    def streamOpen(self, check: bool = True) -> "Stream":
        """``PFACX_streamOpen`` -> a :class:`Stream` of this handle (``.status`` holds the call's status)."""
        s = C.c_void_p()
        st = self._lib.PFACX_streamOpen(self._h, C.byref(s))
        self._ret(st, "PFACX_streamOpen", check)
        return Stream(self, s, st)

    # -- many streams advanced by one call (include/pfac_ext.h: PFACX_flows*) ----------------
    def flowsOpen(self, num_flows: int, check: bool = True) -> "Flows":
        """``PFACX_flowsOpen`` -> a :class:`Flows` set of ``num_flows`` flows of this handle (``.status`` holds the call's status)."""
        s = C.c_void_p()
        st = self._lib.PFACX_flowsOpen(self._h, num_flows, C.byref(s))
        self._ret(st, "PFACX_flowsOpen", check)
        return Flows(self, s, num_flows, st)

    # -- which segments contain every pattern of a rule (include/pfac_ext.h: PFACX_rules*) ----------------
    def rulesOpen(self, rule_off, rule_patterns, check: bool = True) -> "Rules":
        """``PFACX_rulesOpen`` -> a :class:`Rules` set of this handle (``.status`` holds the call's status): rule r is the pattern ids
        ``rule_patterns[rule_off[r]:rule_off[r + 1]]``; the arrays are copied."""
        import numpy as np
        off = np.ascontiguousarray(rule_off, dtype=np.int32)
        pats = np.ascontiguousarray(rule_patterns, dtype=np.int32)
        buf = pats if pats.size else np.zeros(1, dtype=np.int32)
        s = C.c_void_p()
        st = self._lib.PFACX_rulesOpen(self._h, off.ctypes.data if off.size else None, buf.ctypes.data, max(0, off.size - 1), C.byref(s))
        self._ret(st, "PFACX_rulesOpen", check)
        return Rules(self, s, max(0, off.size - 1), st)

    def rulesOpenEx(self, rule_off, members, check: bool = True) -> "Rules":
        """``PFACX_rulesOpenEx`` -> a :class:`Rules` set whose members carry a polarity and a position window: rule r is
        ``members[rule_off[r]:rule_off[r + 1]]``, an array of :func:`rule_member_dtype` (or a sequence of ``(pattern, flags, offset, depth)``
        tuples); the arrays are copied."""
        import numpy as np
        off = np.ascontiguousarray(rule_off, dtype=np.int32)
        if not isinstance(members, np.ndarray):
            members = [tuple(m) for m in members]
        mem = np.ascontiguousarray(np.asarray(members, dtype=rule_member_dtype()))
        buf = mem if mem.size else np.zeros(1, dtype=rule_member_dtype())
        s = C.c_void_p()
        st = self._lib.PFACX_rulesOpenEx(self._h, off.ctypes.data if off.size else None, buf.ctypes.data, max(0, off.size - 1), C.byref(s))
        self._ret(st, "PFACX_rulesOpenEx", check)
        return Rules(self, s, max(0, off.size - 1), st)

    def rulesOpenSeq(self, rule_off, members, check: bool = True) -> "Rules":
        """``PFACX_rulesOpenSeq`` -> a :class:`Rules` set whose members also carry ``distance`` / ``within`` relative to the member in front
        (``PFACX_RULE_RELATIVE``): rule r is ``members[rule_off[r]:rule_off[r + 1]]``, an array of :func:`rule_seq_member_dtype` (or a sequence
        of ``(pattern, flags, offset, depth, distance, within)`` tuples); the arrays are copied."""
        import numpy as np
        off = np.ascontiguousarray(rule_off, dtype=np.int32)
        if not isinstance(members, np.ndarray):
            members = [tuple(m) for m in members]
        mem = np.ascontiguousarray(np.asarray(members, dtype=rule_seq_member_dtype()))
        buf = mem if mem.size else np.zeros(1, dtype=rule_seq_member_dtype())
        s = C.c_void_p()
        st = self._lib.PFACX_rulesOpenSeq(self._h, off.ctypes.data if off.size else None, buf.ctypes.data, max(0, off.size - 1), C.byref(s))
        self._ret(st, "PFACX_rulesOpenSeq", check)
        return Rules(self, s, max(0, off.size - 1), st)

    rules_open_seq = rulesOpenSeq

    # -- rules whose patterns arrive in different pieces of a flow (include/pfac_ext.h: PFACX_flowRules*) ----------------
    def flowRulesOpen(self, rule_off, rule_patterns, num_flows: int, check: bool = True) -> "FlowRules":
        """``PFACX_flowRulesOpen`` -> a :class:`FlowRules` set of ``num_flows`` flows of this handle (``.status`` holds the call's status): rule r
        is the pattern ids ``rule_patterns[rule_off[r]:rule_off[r + 1]]``, as ``rulesOpen`` takes them; the arrays are copied."""
        import numpy as np
        off = np.ascontiguousarray(rule_off, dtype=np.int32)
        pats = np.ascontiguousarray(rule_patterns, dtype=np.int32)
        buf = pats if pats.size else np.zeros(1, dtype=np.int32)
        s = C.c_void_p()
        st = self._lib.PFACX_flowRulesOpen(self._h, off.ctypes.data if off.size else None, buf.ctypes.data, max(0, off.size - 1), num_flows, C.byref(s))
        self._ret(st, "PFACX_flowRulesOpen", check)
        return FlowRules(self, s, max(0, off.size - 1), num_flows, st)

    # -- pattern groups: each segment sees only its own patterns (include/pfac_ext.h: PFACX_groups*) ----------------
    def groupsOpen(self, pattern_masks, check: bool = True) -> "Groups":
        """``PFACX_groupsOpen`` -> a :class:`Groups` table of this handle (``.status`` holds the call's status): ``pattern_masks[id]`` is the
        64-bit group mask of pattern id (entry 0 ignored; at least F + 1 entries); the array is copied."""
        import numpy as np
        masks = np.ascontiguousarray(pattern_masks, dtype=np.uint64)
        buf = masks if masks.size else np.zeros(1, dtype=np.uint64)
        g = C.c_void_p()
        st = self._lib.PFACX_groupsOpen(self._h, buf.ctypes.data, masks.size, C.byref(g))
        self._ret(st, "PFACX_groupsOpen", check)
        return Groups(self, g, st)

    def match_groups_host_array(self, data, pattern_masks, offsets=None, seg_masks=None, all_matches: bool = False):
        """groupsOpen, groupsMatchFromHost over numpy arrays and groupsClose -> (pos, ids, segFirst, segGroups) of the whole group list: the count
        query first, then arrays of exactly that length; offsets=None: the buffer is one segment, seg_masks=None: every segment has all bits."""
        g = self.groupsOpen(pattern_masks)
        try:
            return g.match_host_array(data, offsets, seg_masks, all_matches)
        finally:
            g.close(check=False)

    # -- per-pattern case sensitivity over a caseless set (include/pfac_ext.h: PFACX_case*) ----------------
    def caseOpen(self, patterns: bytes, sensitive, read_flags: int = 0, check: bool = True) -> "CaseSet":
        """``PFACX_caseOpen`` -> a :class:`CaseSet` of this handle (``.status`` holds the call's status, ``.max_matches_per_position`` the
        longest ALL list of one position): `patterns` is the unfolded text of the set the handle read with PFACX_READ_NOCASE, `read_flags` the
        STRICT / STRIP_CR bits of that read, ``sensitive[id]`` non-zero for a case-sensitive line (entry 0 ignored; at least F + 1 entries);
        both are copied."""
        import numpy as np
        flags = np.ascontiguousarray(sensitive, dtype=np.uint8)
        buf = flags if flags.size else np.zeros(1, dtype=np.uint8)
        s, most = C.c_void_p(), C.c_int(0)
        st = self._lib.PFACX_caseOpen(self._h, bytes(patterns), len(patterns), read_flags, buf.ctypes.data, flags.size, C.byref(s), C.byref(most))
        self._ret(st, "PFACX_caseOpen", check)
        return CaseSet(self, s, most.value, st)

    # -- masked byte signatures with wildcards (include/pfac_ext.h: PFACX_sig*) ----------------
    def sigOpen(self, values, masks, sig_off, max_anchor_len: int = 0, check: bool = True) -> "SigSet":
        """``PFACX_sigOpen`` -> a :class:`SigSet` of this handle (``.status`` holds the call's status, ``.bad`` the id of a refused signature):
        the signatures in CSR form, `values` / `masks` uint8, `sig_off` numSigs + 1 offsets; all are copied.  The handle's pattern set is
        REPLACED by the distinct anchors."""
        import numpy as np
        values = np.ascontiguousarray(values, dtype=np.uint8)
        masks = np.ascontiguousarray(masks, dtype=np.uint8)
        off = np.ascontiguousarray(sig_off, dtype=np.uint64)
        pad = np.zeros(1, dtype=np.uint8)
        s, bad = C.c_void_p(), C.c_int(0)
        st = self._lib.PFACX_sigOpen(self._h, (values if values.size else pad).ctypes.data, (masks if masks.size else pad).ctypes.data,
                                     off.ctypes.data if off.size else None, max(0, int(off.size) - 1), max_anchor_len, C.byref(s), C.byref(bad))
        self._ret(st, "PFACX_sigOpen", check)
        return SigSet(self, s, max(0, int(off.size) - 1) if st == 0 else 0, bad.value, st)

    def sigOpenText(self, text: bytes, max_anchor_len: int = 0, check: bool = True) -> "SigSet":
        """``PFACX_sigOpenText`` -> a :class:`SigSet` (``.bad``: the 1-based line that was refused): one signature per line of hex digit pairs,
        a byte may be ``??``, ``x?`` or ``?x``."""
        text = bytes(text)
        s, bad = C.c_void_p(), C.c_int(0)
        st = self._lib.PFACX_sigOpenText(self._h, text, len(text), max_anchor_len, C.byref(s), C.byref(bad))
        self._ret(st, "PFACX_sigOpenText", check)
        return SigSet(self, s, text.count(b"\n") if st == 0 else 0, bad.value, st)

    # -- patterns matched within k mismatches (include/pfac_ext.h: PFACX_approx*) ----------------
    def approxOpen(self, patterns, budgets, min_piece_len: int = 0, max_piece_len: int = 0, check: bool = True) -> "ApproxSet":
        """``PFACX_approxOpen`` -> an :class:`ApproxSet` of this handle (``.status`` holds the call's status, ``.bad`` the id of a refused
        pattern): `patterns` is a list of bytes-likes, or the CSR pair ``(bytes uint8, offsets)``; `budgets` one k per pattern; all are copied.
        The handle's pattern set is REPLACED by the distinct pieces."""
        import numpy as np
        if isinstance(patterns, tuple):
            blob = np.ascontiguousarray(patterns[0], dtype=np.uint8)
            off = np.ascontiguousarray(patterns[1], dtype=np.uint64)
        else:
            patterns = [bytes(p) for p in patterns]
            blob = np.frombuffer(b"".join(patterns), dtype=np.uint8)
            off = np.zeros(len(patterns) + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(p) for p in patterns])
        budgets = np.ascontiguousarray(budgets, dtype=np.int32)
        count = max(0, int(off.size) - 1)
        if budgets.size != count:
            raise ValueError(f"{budgets.size} budgets for {count} patterns")
        pad = np.zeros(1, dtype=np.uint8)
        a, bad = C.c_void_p(), C.c_int(0)
        st = self._lib.PFACX_approxOpen(self._h, (blob if blob.size else pad).ctypes.data, off.ctypes.data if off.size else None,
                                        budgets.ctypes.data if budgets.size else None, count, min_piece_len, max_piece_len, C.byref(a), C.byref(bad))
        self._ret(st, "PFACX_approxOpen", check)
        return ApproxSet(self, a, count if st == 0 else 0, int(budgets.sum()) + count if st == 0 else 0, bad.value, st)

    # -- patterns matched within k edits, indels included (include/pfac_ext.h: PFACX_edit*) ----------------
    def editOpen(self, patterns, budgets, min_piece_len: int = 0, max_piece_len: int = 0, flags: int = 0, check: bool = True) -> "EditSet":
        """``PFACX_editOpen`` -> an :class:`EditSet` of this handle (``.status`` holds the call's status, ``.bad`` the id of a refused pattern):
        `patterns` is a list of bytes-likes, or the CSR pair ``(bytes uint8, offsets)``; `budgets` one k per pattern; `flags` 0 or
        ``PFACX_EDIT_BEST_ENDS``; all are copied.  The handle's pattern set is REPLACED by the distinct pieces."""
        import numpy as np
        if isinstance(patterns, tuple):
            blob = np.ascontiguousarray(patterns[0], dtype=np.uint8)
            off = np.ascontiguousarray(patterns[1], dtype=np.uint64)
        else:
            patterns = [bytes(p) for p in patterns]
            blob = np.frombuffer(b"".join(patterns), dtype=np.uint8)
            off = np.zeros(len(patterns) + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(p) for p in patterns])
        budgets = np.ascontiguousarray(budgets, dtype=np.int32)
        count = max(0, int(off.size) - 1)
        if budgets.size != count:
            raise ValueError(f"{budgets.size} budgets for {count} patterns")
        pad = np.zeros(1, dtype=np.uint8)
        e, bad = C.c_void_p(), C.c_int(0)
        st = self._lib.PFACX_editOpen(self._h, (blob if blob.size else pad).ctypes.data, off.ctypes.data if off.size else None,
                                      budgets.ctypes.data if budgets.size else None, count, min_piece_len, max_piece_len, flags, C.byref(e),
                                      C.byref(bad))
        self._ret(st, "PFACX_editOpen", check)
        return EditSet(self, e, count if st == 0 else 0, int(budgets.sum()) + count if st == 0 else 0, bad.value, st)

    # -- signatures with bounded gaps between parts (include/pfac_ext.h: PFACX_gapsig*) ----------------
    def gapsigOpen(self, values, masks, part_off, sig_part, gap_lo, gap_hi, max_anchor_len: int = 0, check: bool = True) -> "GapSigSet":
        """``PFACX_gapsigOpen`` -> a :class:`GapSigSet` of this handle (``.status`` holds the call's status, ``.bad`` the id of a refused
        signature): the parts in CSR form, `values` / `masks` uint8, `part_off` numParts + 1 byte offsets, `sig_part` numSigs + 1 part indices,
        `gap_lo` / `gap_hi` one entry per part (the gap behind it; a signature's last is ignored); all are copied.  The handle's pattern set
        is REPLACED by the distinct anchors."""
        import numpy as np
        values = np.ascontiguousarray(values, dtype=np.uint8)
        masks = np.ascontiguousarray(masks, dtype=np.uint8)
        part_off = np.ascontiguousarray(part_off, dtype=np.uint64)
        sig_part = np.ascontiguousarray(sig_part, dtype=np.uint64)
        gap_lo = np.ascontiguousarray(gap_lo, dtype=np.uint32)
        gap_hi = np.ascontiguousarray(gap_hi, dtype=np.uint32)
        parts = max(0, int(part_off.size) - 1)
        if gap_lo.size != parts or gap_hi.size != parts:
            raise ValueError(f"{gap_lo.size} / {gap_hi.size} gaps for {parts} parts")
        if sig_part.size and int(sig_part.max()) > parts:
            raise ValueError(f"sig_part reaches part {int(sig_part.max())} of {parts}")
        pad, pad32 = np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint32)
        s, bad = C.c_void_p(), C.c_int(0)
        count = max(0, int(sig_part.size) - 1)
        st = self._lib.PFACX_gapsigOpen(self._h, (values if values.size else pad).ctypes.data, (masks if masks.size else pad).ctypes.data,
                                        part_off.ctypes.data if part_off.size else None, sig_part.ctypes.data if sig_part.size else None,
                                        (gap_lo if parts else pad32).ctypes.data, (gap_hi if parts else pad32).ctypes.data, count, max_anchor_len,
                                        C.byref(s), C.byref(bad))
        self._ret(st, "PFACX_gapsigOpen", check)
        return GapSigSet(self, s, count if st == 0 else 0, bad.value, st)

    def gapsigOpenText(self, text: bytes, max_anchor_len: int = 0, check: bool = True) -> "GapSigSet":
        """``PFACX_gapsigOpenText`` -> a :class:`GapSigSet` (``.bad``: the 1-based line that was refused): one signature per line of hex digit
        pairs (``??``, ``x?``, ``?x``) with gap tokens ``{n}``, ``{n-m}``, ``{-m}``, ``[n]``, ``[n-m]``, ``[-m]`` between them."""
        text = bytes(text)
        s, bad = C.c_void_p(), C.c_int(0)
        st = self._lib.PFACX_gapsigOpenText(self._h, text, len(text), max_anchor_len, C.byref(s), C.byref(bad))
        self._ret(st, "PFACX_gapsigOpenText", check)
        return GapSigSet(self, s, text.count(b"\n") if st == 0 else 0, bad.value, st)

    # -- signatures of byte classes with bounded repeats (include/pfac_ext.h: PFACX_clsig*) ----------------
    def clsigOpen(self, classes, elem_class, elem_lo, elem_hi, sig_elem, not_before=None, not_after=None, max_anchor_len: int = 0,
                  flags: int = 0, check: bool = True) -> "ClSigSet":
        """``PFACX_clsigOpen`` -> a :class:`ClSigSet` of this handle (``.status`` holds the call's status, ``.bad`` the id of a refused
        signature): `classes` uint32 of shape (numClasses, 8) as :func:`word_class` makes them, the elements (class, lo, hi) in three uint32
        arrays, `sig_elem` numSigs + 1 element indices, `not_before` / `not_after` numSigs class indices each (-1: none) or None; all are copied.
        The handle's pattern set is REPLACED by the distinct anchors."""
        import numpy as np
        classes = np.ascontiguousarray(classes, dtype=np.uint32).reshape(-1)
        elem_class = np.ascontiguousarray(elem_class, dtype=np.uint32)
        elem_lo = np.ascontiguousarray(elem_lo, dtype=np.uint32)
        elem_hi = np.ascontiguousarray(elem_hi, dtype=np.uint32)
        sig_elem = np.ascontiguousarray(sig_elem, dtype=np.uint64)
        if classes.size % 8:
            raise ValueError(f"{classes.size} class words: not a multiple of 8")
        if elem_lo.size != elem_class.size or elem_hi.size != elem_class.size:
            raise ValueError(f"{elem_class.size} / {elem_lo.size} / {elem_hi.size} entries of the element arrays")
        if sig_elem.size and int(sig_elem.max()) > elem_class.size:
            raise ValueError(f"sig_elem reaches element {int(sig_elem.max())} of {elem_class.size}")
        count = max(0, int(sig_elem.size) - 1)
        bounds = []
        for b in (not_before, not_after):
            b = None if b is None else np.ascontiguousarray(b, dtype=np.int32)
            if b is not None and b.size != count:
                raise ValueError(f"{b.size} boundary classes for {count} signatures")
            bounds.append(b)
        pad32 = np.zeros(8, dtype=np.uint32)
        s, bad = C.c_void_p(), C.c_int(0)
        st = self._lib.PFACX_clsigOpen(self._h, (classes if classes.size else pad32).ctypes.data, classes.size // 8,
                                       (elem_class if elem_class.size else pad32).ctypes.data, (elem_lo if elem_lo.size else pad32).ctypes.data,
                                       (elem_hi if elem_hi.size else pad32).ctypes.data, sig_elem.ctypes.data if sig_elem.size else None,
                                       bounds[0].ctypes.data if bounds[0] is not None and count else None,
                                       bounds[1].ctypes.data if bounds[1] is not None and count else None, count, max_anchor_len, flags,
                                       C.byref(s), C.byref(bad))
        self._ret(st, "PFACX_clsigOpen", check)
        return ClSigSet(self, s, count if st == 0 else 0, bad.value, st)

    def clsigOpenText(self, text: bytes, max_anchor_len: int = 0, flags: int = 0, check: bool = True) -> "ClSigSet":
        """``PFACX_clsigOpenText`` -> a :class:`ClSigSet` (``.bad``: the 1-based line that was refused): one signature per line in the subset
        of regular-expression syntax that include/pfac_ext.h lists, such as ``AKIA[0-9A-Z]{16}(?![0-9A-Z])``."""
        text = bytes(text)
        s, bad = C.c_void_p(), C.c_int(0)
        st = self._lib.PFACX_clsigOpenText(self._h, text, len(text), max_anchor_len, flags, C.byref(s), C.byref(bad))
        self._ret(st, "PFACX_clsigOpenText", check)
        return ClSigSet(self, s, text.count(b"\n") if st == 0 else 0, bad.value, st)

    # -- numpy conveniences over matchFromHost (still the C ABI underneath) ----------
    def match_host_array(self, data):
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        out = np.full(data.size, -7, dtype=np.int32)   # poison: every element must be written
        if data.size:
            self.matchFromHost(data.ctypes.data, data.size, out.ctypes.data)
        return out

    # -- extensions ----------------------------------------------------------------
    def info(self) -> PFACX_info:
        info = PFACX_info()
        info.structSize = C.sizeof(PFACX_info)
        self._ret(self._lib.PFACX_getInfo(self._h, C.byref(info)), "PFACX_getInfo", True)
        return info

    def caseInsensitive(self) -> int:
        """``PFACX_info_t::caseInsensitive``: 1 when the set was read with PFACX_READ_NOCASE (or loaded from a caseless compiled file)."""
        info = PFACX_info_nocase()
        info.structSize = C.sizeof(PFACX_info_nocase)
        self._ret(self._lib.PFACX_getInfo(self._h, C.byref(info)), "PFACX_getInfo", True)
        return int(info.caseInsensitive)

    def scanStats(self, positions: int = 0):
        """``PFACX_getScanStats`` of the last filter-kernel launch, plus the derived SURVEY 8(d) C5 figures
        (`positions` = input bytes of that launch)."""
        st = PFACX_scan_stats()
        st.structSize = C.sizeof(PFACX_scan_stats)
        self._ret(self._lib.PFACX_getScanStats(self._h, C.byref(st)), "PFACX_getScanStats", True)
        d = {name: int(getattr(st, name)) for name, _ in PFACX_scan_stats._fields_ if name != "filterKernelMs"}
        if st.filterKernelMs >= 0:
            d["filterKernelMs"] = float(st.filterKernelMs)
        if d["walkerRounds"]:
            d["avg_table_steps_per_walk"] = round(d["laneSteps"] / max(1, d["walksStarted"]), 3)
            d["lane_utilisation"] = round(d["laneSteps"] / (d["walkerRounds"] * 64.0 * d["walksPerLane"]), 4)
            if positions:
                d["early_out_rate"] = round(1.0 - d["walksStarted"] / positions, 6)       # positions that never left LDS
                d["level1_hit_rate"] = round(d["level1Hits"] / positions, 6)
                d["walker_rounds_per_KiB"] = round(d["walkerRounds"] * 64.0 / (positions / 1024.0) / 64.0, 4)
        return d

    def table(self, which: int):
        """Host copy of a compiled table as a numpy array (copy)."""
        import numpy as np
        ptr = C.c_void_p()
        nbytes = C.c_size_t()
        self._ret(self._lib.PFACX_getTable(self._h, which, C.byref(ptr), C.byref(nbytes)), "PFACX_getTable", True)
        dtype = np.uint32 if which >= PFACX_TABLE_FILTER_GRAM3 and which != PFACX_TABLE_PREFIX_PATTERN else np.int32
        if nbytes.value == 0:
            return np.zeros(0, dtype=dtype)
        buf = (C.c_char * nbytes.value).from_address(ptr.value)
        return np.frombuffer(buf, dtype=dtype).copy()


_module: Optional[C.CDLL] = None


def order_pairs_probe(handle: "PFAC", d_ids: int, d_pos: int, count: int, n: int, check: bool = True) -> int:
    """``PFACX_orderPairsProbe`` (include/pfac_module.h, test only; bound from the kernel module as tools/lines_sweep.py binds its probe): the
    ordering launches of a compacted-output call over `n` bytes alone, on the `count` (id, position) pairs at the device addresses d_ids / d_pos;
    in place, by ascending position.  The positions must be distinct and below `n`."""
    global _module
    if _module is None:
        _module = C.CDLL(library_paths()[1])
        _module.PFACX_orderPairsProbe.restype = C.c_int
        _module.PFACX_orderPairsProbe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
    return handle._ret(_module.PFACX_orderPairsProbe(handle._h, d_ids, d_pos, count, n), "PFACX_orderPairsProbe", check)


class Stream:
    """One stream (``PFACX_stream_t``) of a handle: pieces in, the pairs that have become final out.  Every call returns
    ``(status, number of pairs, stream offset of the piece's first byte)``; positions are relative to that byte (negative for a
    pair that starts in bytes carried over from earlier pieces)."""

    def __init__(self, handle: PFAC, stream: C.c_void_p, status: int = 0):
        self._owner = handle
        self._lib = handle._lib
        self._s = stream
        self.status = status

    def _ret(self, st: int, where: str, check: bool) -> int:
        if check and st != 0:
            raise PFACError(st, where, error_string(st))
        return st

    def match_device(self, d_piece: int, size: int, d_ids: int, d_pos: int, capacity: int, check: bool = True):
        """``PFACX_streamMatchFromDevice``: capacity >= size + maxPatternLen entries in each device array."""
        n, off = C.c_int(0), C.c_ulonglong(0)
        st = self._lib.PFACX_streamMatchFromDevice(self._s, d_piece, size, d_ids, d_pos, capacity, C.byref(n), C.byref(off))
        return self._ret(st, "PFACX_streamMatchFromDevice", check), n.value, off.value

    def match_host(self, h_piece: int, size: int, h_ids: int, h_pos: int, capacity: int, check: bool = True):
        """``PFACX_streamMatchFromHost``: follows PFAC_setPlatform (the CPU platforms run on the CPU)."""
        n, off = C.c_int(0), C.c_ulonglong(0)
        st = self._lib.PFACX_streamMatchFromHost(self._s, h_piece, size, h_ids, h_pos, capacity, C.byref(n), C.byref(off))
        return self._ret(st, "PFACX_streamMatchFromHost", check), n.value, off.value

    def flush(self, ids: int, pos: int, capacity: int, check: bool = True):
        """``PFACX_streamFlush`` -> (status, number of pairs): the end of the stream; host arrays on a host-fed stream, device
        arrays on a device-fed one; positions are relative to the stream's end."""
        n = C.c_int(0)
        st = self._lib.PFACX_streamFlush(self._s, ids, pos, capacity, C.byref(n))
        return self._ret(st, "PFACX_streamFlush", check), n.value

    def reset(self, check: bool = True) -> int:
        return self._ret(self._lib.PFACX_streamReset(self._s), "PFACX_streamReset", check)

    def close(self, check: bool = True) -> int:
        st = self._lib.PFACX_streamClose(self._s)
        self._s = C.c_void_p()
        return self._ret(st, "PFACX_streamClose", check)

    def match_host_array(self, piece):
        """match_host over a numpy array -> (ids, pos, piece offset) of the pairs this piece made final."""
        import numpy as np
        piece = np.ascontiguousarray(piece, dtype=np.uint8)
        cap = piece.size + max(1, int(self._owner.info().maxPatternLen))
        ids = np.full(cap, -7, dtype=np.int32)
        pos = np.full(cap, -7, dtype=np.int32)
        buf = piece if piece.size else np.zeros(1, dtype=np.uint8)
        _, n, off = self.match_host(buf.ctypes.data, piece.size, ids.ctypes.data, pos.ctypes.data, cap)
        return ids[:n].copy(), pos[:n].copy(), off

    def flush_host_array(self):
        import numpy as np
        cap = max(1, int(self._owner.info().maxPatternLen))
        ids = np.full(cap, -7, dtype=np.int32)
        pos = np.full(cap, -7, dtype=np.int32)
        _, n = self.flush(ids.ctypes.data, pos.ctypes.data, cap)
        return ids[:n].copy(), pos[:n].copy()


class Flows:
    """One flow set (``PFACX_flows_t``) of a handle: a batch of pieces, each the next piece of one flow, in; per piece the pairs
    that have become final out.  ``offsets`` (numPieces + 1 ``size_t``) and ``flow_ids`` (numPieces ``unsigned int``) are host
    arrays; no flow may be named twice in one call."""

    def __init__(self, handle: PFAC, flows: C.c_void_p, num_flows: int, status: int = 0):
        self._owner = handle
        self._lib = handle._lib
        self._f = flows
        self.num_flows = num_flows
        self.status = status

    def _ret(self, st: int, where: str, check: bool) -> int:
        if check and st != 0:
            raise PFACError(st, where, error_string(st))
        return st

    def match_device(self, d_input: int, size: int, h_offsets: int, h_flow_ids: int, num_pieces: int, d_ids: int, d_pos: int, capacity: int,
                     d_piece_first: int, h_piece_offsets: int, check: bool = True):
        """``PFACX_flowsMatchFromDevice`` -> (status, number of pairs): capacity >= size + num_pieces * (maxPatternLen - 1)."""
        n = C.c_int(0)
        st = self._lib.PFACX_flowsMatchFromDevice(self._f, d_input, size, h_offsets, h_flow_ids, num_pieces, d_ids, d_pos, capacity,
                                                  d_piece_first, h_piece_offsets, C.byref(n))
        return self._ret(st, "PFACX_flowsMatchFromDevice", check), n.value

    def match_host(self, h_input: int, size: int, h_offsets: int, h_flow_ids: int, num_pieces: int, h_ids: int, h_pos: int, capacity: int,
                   h_piece_first: int, h_piece_offsets: int, check: bool = True):
        """``PFACX_flowsMatchFromHost``: follows PFAC_setPlatform (the CPU platforms run on the CPU)."""
        n = C.c_int(0)
        st = self._lib.PFACX_flowsMatchFromHost(self._f, h_input, size, h_offsets, h_flow_ids, num_pieces, h_ids, h_pos, capacity,
                                                h_piece_first, h_piece_offsets, C.byref(n))
        return self._ret(st, "PFACX_flowsMatchFromHost", check), n.value

    def flush(self, h_flow_ids: int, n_flows: int, ids: int, pos: int, capacity: int, first: int, check: bool = True):
        """``PFACX_flowsFlush`` -> (status, number of pairs): the end of the named flows; host arrays on a host-fed set, device
        arrays (``first`` included) on a device-fed one."""
        n = C.c_int(0)
        st = self._lib.PFACX_flowsFlush(self._f, h_flow_ids, n_flows, ids, pos, capacity, first, C.byref(n))
        return self._ret(st, "PFACX_flowsFlush", check), n.value

    def reset(self, flow_ids=None, check: bool = True) -> int:
        """``PFACX_flowsReset``: the named flows, or (None) all flows and adopt the handle's current pattern set."""
        import numpy as np
        if flow_ids is None:
            return self._ret(self._lib.PFACX_flowsReset(self._f, None, 0), "PFACX_flowsReset", check)
        f = np.ascontiguousarray(flow_ids, dtype=np.uint32)
        buf = f if f.size else np.zeros(1, dtype=np.uint32)
        return self._ret(self._lib.PFACX_flowsReset(self._f, buf.ctypes.data, f.size), "PFACX_flowsReset", check)

    def close(self, check: bool = True) -> int:
        st = self._lib.PFACX_flowsClose(self._f)
        self._f = C.c_void_p()
        return self._ret(st, "PFACX_flowsClose", check)

    def match_host_array(self, data, offsets, flow_ids, check: bool = True):
        """match_host over numpy arrays -> (status, ids, pos, pieceFirst, pieceOffsets)."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(offsets, dtype=np.uintp)
        fl = np.ascontiguousarray(flow_ids, dtype=np.uint32)
        pieces = fl.size
        cap = data.size + pieces * max(0, int(self._owner.info().maxPatternLen) - 1) + 1
        ids = np.full(cap, -7, dtype=np.int32)
        pos = np.full(cap, -7, dtype=np.int32)
        first = np.full(pieces + 1, -7, dtype=np.int32)
        offs = np.zeros(max(1, pieces), dtype=np.uint64)
        buf = data if data.size else np.zeros(1, dtype=np.uint8)
        flb = fl if fl.size else np.zeros(1, dtype=np.uint32)
        st, n = self.match_host(buf.ctypes.data, data.size, off.ctypes.data, flb.ctypes.data, pieces, ids.ctypes.data, pos.ctypes.data, cap,
                                first.ctypes.data, offs.ctypes.data, check=check)
        return st, ids[:n].copy(), pos[:n].copy(), first, offs[:pieces].copy()

    def flush_host_array(self, flow_ids, check: bool = True):
        """flush over numpy arrays (a host-fed set) -> (status, ids, pos, first)."""
        import numpy as np
        fl = np.ascontiguousarray(flow_ids, dtype=np.uint32)
        cap = max(1, fl.size * max(0, int(self._owner.info().maxPatternLen) - 1))
        ids = np.full(cap, -7, dtype=np.int32)
        pos = np.full(cap, -7, dtype=np.int32)
        first = np.full(fl.size + 1, -7, dtype=np.int32)
        flb = fl if fl.size else np.zeros(1, dtype=np.uint32)
        st, n = self.flush(flb.ctypes.data, fl.size, ids.ctypes.data, pos.ctypes.data, cap, first.ctypes.data, check=check)
        return st, ids[:n].copy(), pos[:n].copy(), first


class Groups:
    """One group table (``PFACX_groups_t``) of a handle: a batch of segments and a 64-bit mask per segment in, the matches of the patterns
    whose mask meets their segment's out.  Every match call returns ``(status, full length of the list)``; OUTPUT_TRUNCATED is returned, not
    raised."""

    def __init__(self, handle: "PFAC", groups: C.c_void_p, status: int = 0):
        self._owner = handle
        self._lib = handle._lib
        self._g = groups
        self.status = status

    def _ret(self, st: int, where: str, check: bool) -> int:
        if check and st != 0:
            raise PFACError(st, where, error_string(st))
        return st

    def match_device(self, d_input: int, size: int, d_offsets, num_segments: int, d_seg_masks, flags: int, d_ids, d_pos, capacity: int,
                     d_seg_first, d_seg_groups, check: bool = True):
        """``PFACX_groupsMatchFromDevice``: `d_offsets` (num_segments + 1 ``size_t``, device) may be None with one segment, `d_seg_masks`
        (num_segments ``uint64``), `d_seg_first` (num_segments + 1 ``size_t``) and `d_seg_groups` (num_segments ``uint64``) may be None, the two
        pair arrays may be None with capacity 0."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_groupsMatchFromDevice(self._g, d_input, size, d_offsets, num_segments, d_seg_masks, flags, d_ids, d_pos, capacity,
                                                   d_seg_first, d_seg_groups, C.byref(n))
        return self._ret(st, "PFACX_groupsMatchFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def match_host(self, h_input: int, size: int, h_offsets, num_segments: int, h_seg_masks, flags: int, h_ids, h_pos, capacity: int, h_seg_first,
                   h_seg_groups, check: bool = True):
        """``PFACX_groupsMatchFromHost``: follows PFAC_setPlatform (the CPU platforms run on the CPU)."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_groupsMatchFromHost(self._g, h_input, size, h_offsets, num_segments, h_seg_masks, flags, h_ids, h_pos, capacity,
                                                 h_seg_first, h_seg_groups, C.byref(n))
        return self._ret(st, "PFACX_groupsMatchFromHost", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def pairs_device(self, d_pair_ids, d_pair_pos, num_pairs: int, d_seg_first_pairs, num_segments: int, d_seg_masks, flags: int, d_ids, d_pos,
                     capacity: int, d_seg_first, d_seg_groups, check: bool = True):
        """``PFACX_groupsPairsFromDevice``: the same list from a LONGEST pair list the caller already has and the first pair of each segment
        (num_segments + 1 ``int``, device): the output of matchBatchFromDeviceReduce or of a flows call.  It runs no scan."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_groupsPairsFromDevice(self._g, d_pair_ids, d_pair_pos, num_pairs, d_seg_first_pairs, num_segments, d_seg_masks, flags,
                                                   d_ids, d_pos, capacity, d_seg_first, d_seg_groups, C.byref(n))
        return self._ret(st, "PFACX_groupsPairsFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def close(self, check: bool = True) -> int:
        st = self._lib.PFACX_groupsClose(self._g)
        self._g = C.c_void_p()
        return self._ret(st, "PFACX_groupsClose", check)

    def match_host_array(self, data, offsets=None, seg_masks=None, all_matches: bool = False):
        """match_host over numpy arrays -> (pos, ids, segFirst, segGroups) of the whole group list; offsets=None: the buffer is one segment."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uintp)
        segments = 1 if off is None else off.size - 1
        sm = None if seg_masks is None else np.ascontiguousarray(seg_masks, dtype=np.uint64)
        first = np.full(segments + 1, 0xDEAD, dtype=np.uintp)
        hit = np.full(max(1, segments), 0xDEAD, dtype=np.uint64)
        buf = data if data.size else np.zeros(1, dtype=np.uint8)
        optr = None if off is None else off.ctypes.data
        mptr = None if sm is None or sm.size == 0 else sm.ctypes.data
        flags = PFACX_GROUPS_ALL if all_matches else 0
        _, n = self.match_host(buf.ctypes.data, data.size, optr, segments, mptr, flags, None, None, 0, first.ctypes.data, hit.ctypes.data)   # the count query
        ids = np.full(max(1, n), -7, dtype=np.int32)
        pos = np.full(max(1, n), -7, dtype=np.int32)
        st, n2 = self.match_host(buf.ctypes.data, data.size, optr, segments, mptr, flags, ids.ctypes.data, pos.ctypes.data, n, first.ctypes.data,
                                 hit.ctypes.data)
        if st != 0 or n2 != n:
            raise PFACError(st, "PFACX_groupsMatchFromHost", f"{n2} pairs behind a count query that said {n}")
        return pos[:n].copy(), ids[:n].copy(), first, hit[:segments].copy()


class CaseSet:
    """One case object (``PFACX_case_t``) of a caseless handle: per-pattern case sensitivity.  Every match call returns ``(status, full length of
    the list)``; OUTPUT_TRUNCATED is returned, not raised.  A context manager: it closes itself."""

    def __init__(self, handle: "PFAC", cs: C.c_void_p, max_matches_per_position: int = 0, status: int = 0):
        self._owner = handle
        self._lib = handle._lib
        self._c = cs
        self.max_matches_per_position = max_matches_per_position
        self.status = status

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self._c:
            self.close(check=False)

    def _ret(self, st: int, where: str, check: bool) -> int:
        if check and st != 0:
            raise PFACError(st, where, error_string(st))
        return st

    def match_device(self, d_input: int, size: int, flags: int, d_ids, d_pos, capacity: int, check: bool = True):
        """``PFACX_caseMatchFromDevice``: capacity >= size entries in each device array."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_caseMatchFromDevice(self._c, d_input, size, flags, d_ids, d_pos, capacity, C.byref(n))
        return self._ret(st, "PFACX_caseMatchFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def match_host(self, h_input: int, size: int, flags: int, h_ids, h_pos, capacity: int, check: bool = True):
        """``PFACX_caseMatchFromHost``: follows PFAC_setPlatform (the CPU platforms run on the CPU); any capacity, 0 with null arrays: the count."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_caseMatchFromHost(self._c, h_input, size, flags, h_ids, h_pos, capacity, C.byref(n))
        return self._ret(st, "PFACX_caseMatchFromHost", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def pairs_device(self, d_input: int, size: int, flags: int, d_pair_ids, d_pair_pos, num_pairs: int, d_ids, d_pos, capacity: int,
                     check: bool = True):
        """``PFACX_casePairsFromDevice``: the same lists from an ordered LONGEST pair list of the caseless handle over the same input (the output
        of matchFromDeviceReduce).  It runs no scan."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_casePairsFromDevice(self._c, d_input, size, flags, d_pair_ids, d_pair_pos, num_pairs, d_ids, d_pos, capacity, C.byref(n))
        return self._ret(st, "PFACX_casePairsFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def close(self, check: bool = True) -> int:
        st = self._lib.PFACX_caseClose(self._c)
        self._c = C.c_void_p()
        return self._ret(st, "PFACX_caseClose", check)

    def match_host_array(self, data, all_matches: bool = False):
        """match_host over a numpy array -> (pos, ids) of the whole list: the count query first, then arrays of exactly that length."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        buf = data if data.size else np.zeros(1, dtype=np.uint8)
        flags = PFACX_CASE_ALL if all_matches else 0
        _, n = self.match_host(buf.ctypes.data, data.size, flags, None, None, 0)
        ids = np.full(max(1, n), -7, dtype=np.int32)
        pos = np.full(max(1, n), -7, dtype=np.int32)
        st, n2 = self.match_host(buf.ctypes.data, data.size, flags, ids.ctypes.data, pos.ctypes.data, n)
        if st != 0 or n2 != n:
            raise PFACError(st, "PFACX_caseMatchFromHost", f"{n2} pairs behind a count query that said {n}")
        return pos[:n].copy(), ids[:n].copy()


class SigSet:
    """One signature object (``PFACX_sig_t``): masked byte signatures over the anchors it loaded into its handle.  Every match call returns
    ``(status, full length of the list)``; OUTPUT_TRUNCATED is returned, not raised.  The list holds (signature id, start), ordered by anchor
    position, not by start.  A context manager: it closes itself."""

    def __init__(self, handle: "PFAC", sig: C.c_void_p, num_sigs: int = 0, bad: int = 0, status: int = 0):
        self._owner = handle
        self._lib = handle._lib
        self._c = sig
        self.num_sigs = num_sigs
        self.bad = bad
        self.status = status

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self._c:
            self.close(check=False)

    def _ret(self, st: int, where: str, check: bool) -> int:
        if check and st != 0:
            raise PFACError(st, where, error_string(st))
        return st

    def anchors(self, check: bool = True):
        """``PFACX_sigGetAnchors`` -> (anchor_id, anchor_off, anchor_len), int32 arrays of num_sigs + 1 entries indexed by signature id."""
        import numpy as np
        n = self.num_sigs + 1
        out = tuple(np.full(n, -7, dtype=np.int32) for _ in range(3))
        st = self._lib.PFACX_sigGetAnchors(self._c, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, n)
        self._ret(st, "PFACX_sigGetAnchors", check)
        return out

    def match_device(self, d_input: int, size: int, d_ids, d_pos, capacity: int, check: bool = True):
        """``PFACX_sigMatchFromDevice``: capacity >= size entries in each device array."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_sigMatchFromDevice(self._c, d_input, size, d_ids, d_pos, capacity, C.byref(n))
        return self._ret(st, "PFACX_sigMatchFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def match_host(self, h_input: int, size: int, h_ids, h_pos, capacity: int, check: bool = True):
        """``PFACX_sigMatchFromHost``: follows PFAC_setPlatform (the CPU platforms run on the CPU); any capacity, 0 with null arrays: the count."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_sigMatchFromHost(self._c, h_input, size, h_ids, h_pos, capacity, C.byref(n))
        return self._ret(st, "PFACX_sigMatchFromHost", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def pairs_device(self, d_input: int, size: int, d_pair_ids, d_pair_pos, num_pairs: int, d_ids, d_pos, capacity: int, check: bool = True):
        """``PFACX_sigPairsFromDevice``: the same list from an ordered LONGEST pair list of the handle over the same input (the output of
        matchFromDeviceReduce).  It runs no scan."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_sigPairsFromDevice(self._c, d_input, size, d_pair_ids, d_pair_pos, num_pairs, d_ids, d_pos, capacity, C.byref(n))
        return self._ret(st, "PFACX_sigPairsFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def close(self, check: bool = True) -> int:
        st = self._lib.PFACX_sigClose(self._c)
        self._c = C.c_void_p()
        return self._ret(st, "PFACX_sigClose", check)

    def match_host_array(self, data):
        """match_host over a numpy array -> (pos, ids) of the whole list: the count query first, then arrays of exactly that length."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        buf = data if data.size else np.zeros(1, dtype=np.uint8)
        _, n = self.match_host(buf.ctypes.data, data.size, None, None, 0)
        ids = np.full(max(1, n), -7, dtype=np.int32)
        pos = np.full(max(1, n), -7, dtype=np.int32)
        st, n2 = self.match_host(buf.ctypes.data, data.size, ids.ctypes.data, pos.ctypes.data, n)
        if st != 0 or n2 != n:
            raise PFACError(st, "PFACX_sigMatchFromHost", f"{n2} entries behind a count query that said {n}")
        return pos[:n].copy(), ids[:n].copy()


class ApproxSet:
    """One approximate object (``PFACX_approx_t``): patterns matched within k mismatches over the pieces it loaded into its handle.  Every match
    call returns ``(status, full length of the list)``; OUTPUT_TRUNCATED is returned, not raised.  The list holds (pattern id, start) and the
    distance in a third array, ordered by candidate position, not by start.  A context manager: it closes itself."""

    def __init__(self, handle: "PFAC", approx: C.c_void_p, num_patterns: int = 0, num_pieces: int = 0, bad: int = 0, status: int = 0):
        self._owner = handle
        self._lib = handle._lib
        self._c = approx
        self.num_patterns = num_patterns
        self.num_pieces = num_pieces                             # the sum of k + 1
        self.bad = bad
        self.status = status

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self._c:
            self.close(check=False)

    def _ret(self, st: int, where: str, check: bool) -> int:
        if check and st != 0:
            raise PFACError(st, where, error_string(st))
        return st

    def pieces(self, check: bool = True):
        """``PFACX_approxGetPieces`` -> (piece_off, piece_id, piece_start, piece_len): piece_off uint64 with num_patterns + 2 entries in CSR form by
        pattern id, the others int32 with one entry per piece."""
        import numpy as np
        off = np.full(self.num_patterns + 2, 7, dtype=np.uint64)
        out = tuple(np.full(max(1, self.num_pieces), -7, dtype=np.int32) for _ in range(3))
        st = self._lib.PFACX_approxGetPieces(self._c, off.ctypes.data, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, self.num_pieces)
        self._ret(st, "PFACX_approxGetPieces", check)
        return (off,) + tuple(a[:self.num_pieces] for a in out)

    def match_device(self, d_input: int, size: int, d_ids, d_pos, d_mis, capacity: int, check: bool = True):
        """``PFACX_approxMatchFromDevice``: capacity >= size entries in each device array; d_mis may be None."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_approxMatchFromDevice(self._c, d_input, size, d_ids, d_pos, d_mis, capacity, C.byref(n))
        return self._ret(st, "PFACX_approxMatchFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def match_host(self, h_input: int, size: int, h_ids, h_pos, h_mis, capacity: int, check: bool = True):
        """``PFACX_approxMatchFromHost``: follows PFAC_setPlatform (the CPU platforms run on the CPU); any capacity, 0 with null arrays: the count."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_approxMatchFromHost(self._c, h_input, size, h_ids, h_pos, h_mis, capacity, C.byref(n))
        return self._ret(st, "PFACX_approxMatchFromHost", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def pairs_device(self, d_input: int, size: int, d_pair_ids, d_pair_pos, num_pairs: int, d_ids, d_pos, d_mis, capacity: int, check: bool = True):
        """``PFACX_approxPairsFromDevice``: the same list from an ordered LONGEST pair list of the handle over the same input (the output of
        matchFromDeviceReduce).  It runs no scan."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_approxPairsFromDevice(self._c, d_input, size, d_pair_ids, d_pair_pos, num_pairs, d_ids, d_pos, d_mis, capacity, C.byref(n))
        return self._ret(st, "PFACX_approxPairsFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def close(self, check: bool = True) -> int:
        st = self._lib.PFACX_approxClose(self._c)
        self._c = C.c_void_p()
        return self._ret(st, "PFACX_approxClose", check)

    def match_host_array(self, data):
        """match_host over a numpy array -> (pos, ids, mis) of the whole list: the count query first, then arrays of exactly that length."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        buf = data if data.size else np.zeros(1, dtype=np.uint8)
        _, n = self.match_host(buf.ctypes.data, data.size, None, None, None, 0)
        ids, pos, mis = (np.full(max(1, n), -7, dtype=np.int32) for _ in range(3))
        st, n2 = self.match_host(buf.ctypes.data, data.size, ids.ctypes.data, pos.ctypes.data, mis.ctypes.data, n)
        if st != 0 or n2 != n:
            raise PFACError(st, "PFACX_approxMatchFromHost", f"{n2} entries behind a count query that said {n}")
        return pos[:n].copy(), ids[:n].copy(), mis[:n].copy()


class EditSet:
    """One edit-distance object (``PFACX_edit_t``): patterns matched within k edits (substitutions, insertions, deletions) over the pieces it
    loaded into its handle.  Every match call returns ``(status, full length of the list)``; OUTPUT_TRUNCATED is returned, not raised.  The
    list holds (pattern id, start) with the end and the distance in a third and a fourth array, ordered by the owning candidate's position,
    not by start or end.  A context manager: it closes itself."""

    def __init__(self, handle: "PFAC", edit: C.c_void_p, num_patterns: int = 0, num_pieces: int = 0, bad: int = 0, status: int = 0):
        self._owner = handle
        self._lib = handle._lib
        self._c = edit
        self.num_patterns = num_patterns
        self.num_pieces = num_pieces                             # the sum of k + 1
        self.bad = bad
        self.status = status

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self._c:
            self.close(check=False)

    def _ret(self, st: int, where: str, check: bool) -> int:
        if check and st != 0:
            raise PFACError(st, where, error_string(st))
        return st

    def pieces(self, check: bool = True):
        """``PFACX_editGetPieces`` -> (piece_off, piece_id, piece_start, piece_len): piece_off uint64 with num_patterns + 2 entries in CSR form by
        pattern id, the others int32 with one entry per piece."""
        import numpy as np
        off = np.full(self.num_patterns + 2, 7, dtype=np.uint64)
        out = tuple(np.full(max(1, self.num_pieces), -7, dtype=np.int32) for _ in range(3))
        st = self._lib.PFACX_editGetPieces(self._c, off.ctypes.data, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, self.num_pieces)
        self._ret(st, "PFACX_editGetPieces", check)
        return (off,) + tuple(a[:self.num_pieces] for a in out)

    def match_device(self, d_input: int, size: int, d_ids, d_pos, d_end, d_dist, capacity: int, check: bool = True):
        """``PFACX_editMatchFromDevice``: capacity >= size entries in each device array; d_end and d_dist may be None."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_editMatchFromDevice(self._c, d_input, size, d_ids, d_pos, d_end, d_dist, capacity, C.byref(n))
        return self._ret(st, "PFACX_editMatchFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def match_host(self, h_input: int, size: int, h_ids, h_pos, h_end, h_dist, capacity: int, check: bool = True):
        """``PFACX_editMatchFromHost``: follows PFAC_setPlatform (the CPU platforms run on the CPU); any capacity, 0 with null arrays: the count."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_editMatchFromHost(self._c, h_input, size, h_ids, h_pos, h_end, h_dist, capacity, C.byref(n))
        return self._ret(st, "PFACX_editMatchFromHost", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def pairs_device(self, d_input: int, size: int, d_pair_ids, d_pair_pos, num_pairs: int, d_ids, d_pos, d_end, d_dist, capacity: int,
                     check: bool = True):
        """``PFACX_editPairsFromDevice``: the same list from an ordered LONGEST pair list of the handle over the same input (the output of
        matchFromDeviceReduce).  It runs no scan."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_editPairsFromDevice(self._c, d_input, size, d_pair_ids, d_pair_pos, num_pairs, d_ids, d_pos, d_end, d_dist, capacity,
                                                 C.byref(n))
        return self._ret(st, "PFACX_editPairsFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def close(self, check: bool = True) -> int:
        st = self._lib.PFACX_editClose(self._c)
        self._c = C.c_void_p()
        return self._ret(st, "PFACX_editClose", check)

    def match_host_array(self, data):
        """match_host over a numpy array -> (ids, start, end, dist) of the whole list: the count query first, then arrays of exactly that length."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        buf = data if data.size else np.zeros(1, dtype=np.uint8)
        _, n = self.match_host(buf.ctypes.data, data.size, None, None, None, None, 0)
        ids, pos, end, dist = (np.full(max(1, n), -7, dtype=np.int32) for _ in range(4))
        st, n2 = self.match_host(buf.ctypes.data, data.size, ids.ctypes.data, pos.ctypes.data, end.ctypes.data, dist.ctypes.data, n)
        if st != 0 or n2 != n:
            raise PFACError(st, "PFACX_editMatchFromHost", f"{n2} entries behind a count query that said {n}")
        return ids[:n].copy(), pos[:n].copy(), end[:n].copy(), dist[:n].copy()


class GapSigSet:
    """One gapped-signature object (``PFACX_gapsig_t``): signatures with bounded gaps between parts over the anchors it loaded into its handle.
    Every match call returns ``(status, full length of the list)``; OUTPUT_TRUNCATED is returned, not raised.  The list holds (signature id,
    start) and the smallest end in a third array, ordered by the owning anchor occurrence, not by start.  A context manager: it closes itself."""

    def __init__(self, handle: "PFAC", sig: C.c_void_p, num_sigs: int = 0, bad: int = 0, status: int = 0):
        self._owner = handle
        self._lib = handle._lib
        self._c = sig
        self.num_sigs = num_sigs
        self.bad = bad
        self.status = status

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self._c:
            self.close(check=False)

    def _ret(self, st: int, where: str, check: bool) -> int:
        if check and st != 0:
            raise PFACError(st, where, error_string(st))
        return st

    def anchors(self, check: bool = True):
        """``PFACX_gapsigGetAnchors`` -> (anchor_id, anchor_part, anchor_off, anchor_len), int32 arrays of num_sigs + 1 entries by signature id."""
        import numpy as np
        n = self.num_sigs + 1
        out = tuple(np.full(n, -7, dtype=np.int32) for _ in range(4))
        st = self._lib.PFACX_gapsigGetAnchors(self._c, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data, n)
        self._ret(st, "PFACX_gapsigGetAnchors", check)
        return out

    def match_device(self, d_input: int, size: int, d_ids, d_pos, d_end, capacity: int, check: bool = True):
        """``PFACX_gapsigMatchFromDevice``: capacity >= size entries in each device array; d_end may be None."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_gapsigMatchFromDevice(self._c, d_input, size, d_ids, d_pos, d_end, capacity, C.byref(n))
        return self._ret(st, "PFACX_gapsigMatchFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def match_host(self, h_input: int, size: int, h_ids, h_pos, h_end, capacity: int, check: bool = True):
        """``PFACX_gapsigMatchFromHost``: follows PFAC_setPlatform (the CPU platforms run on the CPU); any capacity, 0 with null arrays: the count."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_gapsigMatchFromHost(self._c, h_input, size, h_ids, h_pos, h_end, capacity, C.byref(n))
        return self._ret(st, "PFACX_gapsigMatchFromHost", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def pairs_device(self, d_input: int, size: int, d_pair_ids, d_pair_pos, num_pairs: int, d_ids, d_pos, d_end, capacity: int, check: bool = True):
        """``PFACX_gapsigPairsFromDevice``: the same list from an ordered LONGEST pair list of the handle over the same input (the output of
        matchFromDeviceReduce).  It runs no scan."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_gapsigPairsFromDevice(self._c, d_input, size, d_pair_ids, d_pair_pos, num_pairs, d_ids, d_pos, d_end, capacity, C.byref(n))
        return self._ret(st, "PFACX_gapsigPairsFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def close(self, check: bool = True) -> int:
        st = self._lib.PFACX_gapsigClose(self._c)
        self._c = C.c_void_p()
        return self._ret(st, "PFACX_gapsigClose", check)

    def match_host_array(self, data):
        """match_host over a numpy array -> (pos, ids, end) of the whole list: the count query first, then arrays of exactly that length."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        buf = data if data.size else np.zeros(1, dtype=np.uint8)
        _, n = self.match_host(buf.ctypes.data, data.size, None, None, None, 0)
        ids, pos, end = (np.full(max(1, n), -7, dtype=np.int32) for _ in range(3))
        st, n2 = self.match_host(buf.ctypes.data, data.size, ids.ctypes.data, pos.ctypes.data, end.ctypes.data, n)
        if st != 0 or n2 != n:
            raise PFACError(st, "PFACX_gapsigMatchFromHost", f"{n2} entries behind a count query that said {n}")
        return pos[:n].copy(), ids[:n].copy(), end[:n].copy()


class ClSigSet:
    """One class-signature object (``PFACX_clsig_t``): signatures of byte classes with bounded repeats over the anchors it loaded into its handle.
    Every match call returns ``(status, full length of the list)``; OUTPUT_TRUNCATED is returned, not raised.  The list holds (signature id,
    start) and the largest end (PFACX_CLSIG_SHORTEST_END: the smallest) in a third array, ordered by the owning anchor occurrence, not by start.  A context manager: it closes itself."""

    def __init__(self, handle: "PFAC", sig: C.c_void_p, num_sigs: int = 0, bad: int = 0, status: int = 0):
        self._owner = handle
        self._lib = handle._lib
        self._c = sig
        self.num_sigs = num_sigs
        self.bad = bad
        self.status = status

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self._c:
            self.close(check=False)

    def _ret(self, st: int, where: str, check: bool) -> int:
        if check and st != 0:
            raise PFACError(st, where, error_string(st))
        return st

    def anchors(self, check: bool = True):
        """``PFACX_clsigGetAnchors`` -> (anchor_id, anchor_part after fusion, anchor_off, anchor_len), int32 arrays of num_sigs + 1 entries by signature id."""
        import numpy as np
        n = self.num_sigs + 1
        out = tuple(np.full(n, -7, dtype=np.int32) for _ in range(4))
        st = self._lib.PFACX_clsigGetAnchors(self._c, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data, n)
        self._ret(st, "PFACX_clsigGetAnchors", check)
        return out

    def match_device(self, d_input: int, size: int, d_ids, d_pos, d_end, capacity: int, check: bool = True):
        """``PFACX_clsigMatchFromDevice``: capacity >= size entries in each device array; d_end may be None."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_clsigMatchFromDevice(self._c, d_input, size, d_ids, d_pos, d_end, capacity, C.byref(n))
        return self._ret(st, "PFACX_clsigMatchFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def match_host(self, h_input: int, size: int, h_ids, h_pos, h_end, capacity: int, check: bool = True):
        """``PFACX_clsigMatchFromHost``: follows PFAC_setPlatform (the CPU platforms run on the CPU); any capacity, 0 with null arrays: the count."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_clsigMatchFromHost(self._c, h_input, size, h_ids, h_pos, h_end, capacity, C.byref(n))
        return self._ret(st, "PFACX_clsigMatchFromHost", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def pairs_device(self, d_input: int, size: int, d_pair_ids, d_pair_pos, num_pairs: int, d_ids, d_pos, d_end, capacity: int, check: bool = True):
        """``PFACX_clsigPairsFromDevice``: the same list from an ordered LONGEST pair list of the handle over the same input (the output of
        matchFromDeviceReduce).  It runs no scan."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_clsigPairsFromDevice(self._c, d_input, size, d_pair_ids, d_pair_pos, num_pairs, d_ids, d_pos, d_end, capacity, C.byref(n))
        return self._ret(st, "PFACX_clsigPairsFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def match_batch_device(self, d_input: int, size: int, d_offsets, num_segments: int, d_ids, d_pos, d_end, capacity: int, d_seg_first=None,
                           check: bool = True):
        """``PFACX_clsigBatchMatchFromDevice``: match_device with every embedding, boundary test and owner inside one segment of the
        num_segments + 1 device offsets (size_t; clamped and raised, never trusted); d_seg_first: num_segments + 1 entries of size_t or None."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_clsigBatchMatchFromDevice(self._c, d_input, size, d_offsets, num_segments, d_ids, d_pos, d_end, capacity, d_seg_first,
                                                       C.byref(n))
        return self._ret(st, "PFACX_clsigBatchMatchFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def match_batch_host(self, h_input: int, size: int, h_offsets, num_segments: int, h_ids, h_pos, h_end, capacity: int, h_seg_first=None,
                         check: bool = True):
        """``PFACX_clsigBatchMatchFromHost``: the host form over validated host offsets; follows PFAC_setPlatform."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_clsigBatchMatchFromHost(self._c, h_input, size, h_offsets, num_segments, h_ids, h_pos, h_end, capacity, h_seg_first,
                                                     C.byref(n))
        return self._ret(st, "PFACX_clsigBatchMatchFromHost", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def batch_pairs_device(self, d_input: int, size: int, d_offsets, num_segments: int, d_pair_ids, d_pair_pos, num_pairs: int, d_ids, d_pos, d_end,
                           capacity: int, d_seg_first=None, check: bool = True):
        """``PFACX_clsigBatchPairsFromDevice``: the batch list from a longest pair list of the handle over the same input; a pair's segment comes
        from its position.  It runs no scan."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_clsigBatchPairsFromDevice(self._c, d_input, size, d_offsets, num_segments, d_pair_ids, d_pair_pos, num_pairs, d_ids,
                                                       d_pos, d_end, capacity, d_seg_first, C.byref(n))
        return self._ret(st, "PFACX_clsigBatchPairsFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def close(self, check: bool = True) -> int:
        st = self._lib.PFACX_clsigClose(self._c)
        self._c = C.c_void_p()
        return self._ret(st, "PFACX_clsigClose", check)

    def match_host_array(self, data):
        """match_host over a numpy array -> (pos, ids, end) of the whole list: the count query first, then arrays of exactly that length."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        buf = data if data.size else np.zeros(1, dtype=np.uint8)
        _, n = self.match_host(buf.ctypes.data, data.size, None, None, None, 0)
        ids, pos, end = (np.full(max(1, n), -7, dtype=np.int32) for _ in range(3))
        st, n2 = self.match_host(buf.ctypes.data, data.size, ids.ctypes.data, pos.ctypes.data, end.ctypes.data, n)
        if st != 0 or n2 != n:
            raise PFACError(st, "PFACX_clsigMatchFromHost", f"{n2} entries behind a count query that said {n}")
        return pos[:n].copy(), ids[:n].copy(), end[:n].copy()

    def match_batch_host_array(self, data, offsets):
        """match_batch_host over numpy arrays -> (pos, ids, end, seg_first) of the whole list: the count query first, then arrays of exactly
        that length."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        buf = data if data.size else np.zeros(1, dtype=np.uint8)
        segs = offsets.size - 1
        _, n = self.match_batch_host(buf.ctypes.data, data.size, offsets.ctypes.data, segs, None, None, None, 0)
        ids, pos, end = (np.full(max(1, n), -7, dtype=np.int32) for _ in range(3))
        first = np.full(segs + 1, 2 ** 64 - 7, dtype=np.uint64)
        st, n2 = self.match_batch_host(buf.ctypes.data, data.size, offsets.ctypes.data, segs, ids.ctypes.data, pos.ctypes.data, end.ctypes.data, n,
                                       first.ctypes.data)
        if st != 0 or n2 != n:
            raise PFACError(st, "PFACX_clsigBatchMatchFromHost", f"{n2} entries behind a count query that said {n}")
        return pos[:n].copy(), ids[:n].copy(), end[:n].copy(), first


def rule_member_dtype():
    """``PFACX_rule_member_t`` as a numpy structured dtype: pattern (int32), flags, offset, depth (uint32); 16 bytes, no padding."""
    import numpy as np
    return np.dtype(RULE_MEMBER_FIELDS)


def rule_seq_member_dtype():
    """``PFACX_rule_seq_member_t`` as a numpy structured dtype: pattern (int32), flags, offset, depth, distance, within (uint32); 24 bytes, no
    padding."""
    import numpy as np
    return np.dtype(RULE_SEQ_MEMBER_FIELDS)


class Rules:
    """One rule set (``PFACX_rules_t``) of a handle: a batch of segments in, the (segment, rule) pairs of the rules whose patterns all occur
    in one segment out.  Every match call returns ``(status, full length of the fired list)``; OUTPUT_TRUNCATED is returned, not raised."""

    def __init__(self, handle: PFAC, rules: C.c_void_p, num_rules: int, status: int = 0):
        self._owner = handle
        self._lib = handle._lib
        self._r = rules
        self.num_rules = num_rules
        self.status = status

    def _ret(self, st: int, where: str, check: bool) -> int:
        if check and st != 0:
            raise PFACError(st, where, error_string(st))
        return st

    def match_device(self, d_input: int, size: int, d_offsets, num_segments: int, d_fired_seg, d_fired_rule, capacity: int, d_seg_first,
                     check: bool = True):
        """``PFACX_rulesMatchFromDevice``: `d_offsets` (num_segments + 1 ``size_t``, device) may be None with one segment, `d_seg_first`
        (num_segments + 1 ``size_t``, device) may be None, the two arrays may be None with capacity 0."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_rulesMatchFromDevice(self._r, d_input, size, d_offsets, num_segments, d_fired_seg, d_fired_rule, capacity, d_seg_first,
                                                  C.byref(n))
        return self._ret(st, "PFACX_rulesMatchFromDevice", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def match_host(self, h_input: int, size: int, h_offsets, num_segments: int, h_fired_seg, h_fired_rule, capacity: int, h_seg_first,
                   check: bool = True):
        """``PFACX_rulesMatchFromHost``: follows PFAC_setPlatform (the CPU platforms run on the CPU)."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_rulesMatchFromHost(self._r, h_input, size, h_offsets, num_segments, h_fired_seg, h_fired_rule, capacity, h_seg_first,
                                                C.byref(n))
        return self._ret(st, "PFACX_rulesMatchFromHost", check and st != STATUS.OUTPUT_TRUNCATED), n.value

    def close(self, check: bool = True) -> int:
        st = self._lib.PFACX_rulesClose(self._r)
        self._r = C.c_void_p()
        return self._ret(st, "PFACX_rulesClose", check)

    def match_host_array(self, data, offsets=None):
        """match_host over numpy arrays -> (seg, rule, segFirst) of the whole fired list; offsets=None: the buffer is one segment."""
        import numpy as np
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uintp)
        segments = 1 if off is None else off.size - 1
        first = np.full(segments + 1, 0xDEAD, dtype=np.uintp)
        buf = data if data.size else np.zeros(1, dtype=np.uint8)
        optr = None if off is None else off.ctypes.data
        _, n = self.match_host(buf.ctypes.data, data.size, optr, segments, None, None, 0, first.ctypes.data)       # the count query
        seg = np.full(max(1, n), -7, dtype=np.int32)
        rule = np.full(max(1, n), -7, dtype=np.int32)
        st, n2 = self.match_host(buf.ctypes.data, data.size, optr, segments, seg.ctypes.data, rule.ctypes.data, n, first.ctypes.data)
        assert st == 0 and n2 == n
        return seg[:n].copy(), rule[:n].copy(), first


class FlowRules:
    """One flow-rule set (``PFACX_flowRules_t``) of a handle: the pairs of a flows call in (``ids``, ``pieceFirst``, the call's flow ids and its
    number of pairs -- or ``ids``, ``first`` and the flows of a flush), the (piece, rule) pairs the call completes out.  Every pairs call returns
    ``(status, full length of the list)``; OUTPUT_TRUNCATED is returned, not raised, and leaves every flow as it was."""

    def __init__(self, handle: PFAC, fr: C.c_void_p, num_rules: int, num_flows: int, status: int = 0):
        self._owner = handle
        self._lib = handle._lib
        self._f = fr
        self.num_rules = num_rules
        self.num_flows = num_flows
        self.status = status

    def _ret(self, st: int, where: str, check: bool) -> int:
        if check and st not in (0, STATUS.OUTPUT_TRUNCATED):
            raise PFACError(st, where, error_string(st))
        return st

    def pairs_device(self, d_pair_ids, num_pairs: int, d_piece_first, h_flow_ids, num_pieces: int, d_fired_piece, d_fired_rule, capacity: int,
                     d_piece_fired_first, check: bool = True):
        """``PFACX_flowRulesPairsFromDevice``: device arrays but for ``h_flow_ids``; ``d_piece_fired_first`` (numPieces + 1 ``size_t``) may be None,
        and so may the two fired arrays with capacity 0."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_flowRulesPairsFromDevice(self._f, d_pair_ids, num_pairs, d_piece_first, h_flow_ids, num_pieces, d_fired_piece,
                                                      d_fired_rule, capacity, d_piece_fired_first, C.byref(n))
        return self._ret(st, "PFACX_flowRulesPairsFromDevice", check), n.value

    def pairs_host(self, h_pair_ids, num_pairs: int, h_piece_first, h_flow_ids, num_pieces: int, h_fired_piece, h_fired_rule, capacity: int,
                   h_piece_fired_first, check: bool = True):
        """``PFACX_flowRulesPairsFromHost``: the same over host arrays, a loop on the host on every platform."""
        n = C.c_size_t(0)
        st = self._lib.PFACX_flowRulesPairsFromHost(self._f, h_pair_ids, num_pairs, h_piece_first, h_flow_ids, num_pieces, h_fired_piece,
                                                    h_fired_rule, capacity, h_piece_fired_first, C.byref(n))
        return self._ret(st, "PFACX_flowRulesPairsFromHost", check), n.value

    def reset(self, flow_ids=None, check: bool = True) -> int:
        """``PFACX_flowRulesReset``: the named flows, or (None) all flows."""
        import numpy as np
        if flow_ids is None:
            return self._ret(self._lib.PFACX_flowRulesReset(self._f, None, 0), "PFACX_flowRulesReset", check)
        f = np.ascontiguousarray(flow_ids, dtype=np.uint32)
        buf = f if f.size else np.zeros(1, dtype=np.uint32)
        return self._ret(self._lib.PFACX_flowRulesReset(self._f, buf.ctypes.data, f.size), "PFACX_flowRulesReset", check)

    def close(self, check: bool = True) -> int:
        st = self._lib.PFACX_flowRulesClose(self._f)
        self._f = C.c_void_p()
        return self._ret(st, "PFACX_flowRulesClose", check)

    def pairs_host_array(self, ids, piece_first, flow_ids, capacity=None, check: bool = True):
        """pairs_host over numpy arrays -> (status, piece[], rule[], pieceFiredFirst[numPieces + 1], full length).  capacity None: the count query
        first, then arrays of exactly that length; a number: arrays of exactly that many entries (status may be OUTPUT_TRUNCATED)."""
        import numpy as np
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        first = np.ascontiguousarray(piece_first, dtype=np.int32)
        fl = np.ascontiguousarray(flow_ids, dtype=np.uint32)
        pieces = fl.size
        idb = ids if ids.size else np.zeros(1, dtype=np.int32)
        flb = fl if fl.size else np.zeros(1, dtype=np.uint32)
        fired_first = np.zeros(pieces + 1, dtype=np.uintp)
        if capacity is None:
            st, capacity = self.pairs_host(idb.ctypes.data, ids.size, first.ctypes.data, flb.ctypes.data, pieces, None, None, 0, None, check=check)
            if st not in (0, STATUS.OUTPUT_TRUNCATED):
                return st, np.zeros(0, np.int32), np.zeros(0, np.int32), fired_first, 0
        piece = np.full(max(1, capacity), -7, dtype=np.int32)
        rule = np.full(max(1, capacity), -7, dtype=np.int32)
        st, n = self.pairs_host(idb.ctypes.data, ids.size, first.ctypes.data, flb.ctypes.data, pieces, piece.ctypes.data, rule.ctypes.data, capacity,
                                fired_first.ctypes.data, check=check)
        k = min(n, capacity)
        return st, piece[:k].copy(), rule[:k].copy(), fired_first, n
