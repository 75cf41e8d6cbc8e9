"""The cases of tests/test_linesctx_edges_host.py and tests/test_linesctx_edges_gpu.py: PFACX_matchLinesContext* where the device stage of
scan_lines.hip (pfac_lines_members, pfac_block_scan<max, max>, pfac_lines_widen, pfac_block_scan<sum>, pfac_lines_select<., ContextArgs>) takes
another path -- at the edges of a line block, of a block of the block scan and of one pass of the grid.  No test functions and none of the
library's line code: a builder returns calls (name, patterns, data, before, after, invert, H), H the sorted line numbers the plain call selects,
known from how the input was made, so that linesctx_ref.context_model(..., H=H) never runs a matcher over megabytes.  Every input is matched
with linesctx_ref.X: a line matches if it holds an 'x'.

    A  numLines on, one below and one above a multiple of a line block, one hit on either side of the edge, windows on, below and above a
       word and a line block
    B  groups across a line-block edge: apart, touching and merged exactly there
    C  position blocks on, one above and twice one pass of the grid (and one block of the block scan)
    D  two members more than a block of the block scan apart IN LINE BLOCKS: the nearest member arrives through the folded front of the scan

Test infrastructure only."""
import functools

import numpy as np

from tests.linesctx_ref import MAX, X

BLOCK = 2048                            # scan_lines.hip: kBlockShift = 11 -- the positions of a block, the lines of a line block
WORD = 32                               # scan_lines.hip: kBlockWords = 64 -- a block is 64 bitmap words of 32 bits, a word per lane
SCAN_BLOCK = 8192                       # scan_passes.h: kScanBlock = 1024 * kScanPer -- the values of a block of pfac_block_scan; from its second block on it folds its front
WAVES_PER_GROUP = 4                     # scan_lines.hip: kLinesThreads / 64 -- a wave per block, four blocks a workgroup
GROUPS_PER_CU = 8                       # scan_lines.hip: waveGridFor -- gridCap(c, 8) workgroups at most
GRID_PASS = WAVES_PER_GROUP * GROUPS_PER_CU * 256       # the blocks of one trip of `for (b ...; b += waves)` on 256 compute units: 8192

NL, FILL, HIT, OTHER = 10, ord("a"), ord("x"), ord("z")


def grid_pass(compute_units):
    return WAVES_PER_GROUP * GROUPS_PER_CU * int(compute_units)


def position_blocks(size, mis=0):
    """scan_lines.hip: linesArgs -- the positions q = p + mis of [0, mis + size]"""
    return (mis + size) // BLOCK + 1


def place(k):
    """(line block, word of the block, bit of the word) of line k in a bitmap by line number"""
    return k // BLOCK, k % BLOCK // WORD, k % WORD


def window_name(v):
    return "max" if v == MAX else str(v)


def others(num, hits):
    """H under INVERT: every line but `hits`"""
    return np.setdiff1d(np.arange(num, dtype=np.int64), np.asarray(hits, dtype=np.int64))


@functools.lru_cache(maxsize=None)
def short_lines(num, hits, terminated=True):
    """linesctx_ref.tiny_lines: `num` lines, empty at odd numbers and "z" at even ones, "x" at `hits` (a tuple); an unterminated last line that
    would be empty is "z" """
    lines = [b"x" if k in hits else (b"" if k & 1 else b"z") for k in range(num)]
    if not terminated and not lines[-1]:
        lines[-1] = b"z"
    return b"\n".join(lines) + (b"\n" if terminated else b"")


# ---------------------------------------------------------------------------------------------------------------- A: line-block edges

A_LINE_COUNTS = (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1)
A_WINDOW_VALUES = (0, 1, WORD - 1, WORD, WORD + 1, BLOCK - 1, BLOCK, MAX)
# (before, after): the square of A_WINDOW_VALUES thinned to one pair per value on either side, and no context at all.  Among them a window that
# ends exactly at numLines - 1: hit 2046 / after 1 / 2048 lines, hit 2047 / after 2048 / 4096 lines, hit 2048 / after 2047 / 4096 lines
A_WINDOWS = ((0, WORD + 1), (1, BLOCK), (WORD - 1, 0), (WORD, MAX), (WORD + 1, 1), (BLOCK - 1, WORD), (BLOCK, WORD - 1), (MAX, BLOCK - 1), (0, 0))
# by hand: where each hit lies.  2046 and 2047 are the last two bits of line block 0's last word, 2048 and 2049 the first two of line block 1
A_HIT_PLACES = {0: (0, 0, 0), 2046: (0, 63, 30), 2047: (0, 63, 31), 2048: (1, 0, 0), 2049: (1, 0, 1), 4094: (1, 63, 30), 4095: (1, 63, 31),
                4096: (2, 0, 0)}


def a_hits(num):
    """one hit a call: line 0, the two lines on either side of 2047 | 2048, the last line"""
    return sorted({k for k in (0, BLOCK - 2, BLOCK - 1, BLOCK, BLOCK + 1, num - 1) if k < num})


def a_shapes():
    return [(num, hit, terminated) for num in A_LINE_COUNTS for hit in a_hits(num) for terminated in (True, False)]


def line_block_edges():
    """FAMILY A.  `num` lines and one hit: (b << kBlockShift) >= numLines and lineBitsOf say "no line here" for the line block behind the last
    at 2048 and 4096 lines, "a full last word" for the one in front; the hit's window leaves its word and its line block in both directions;
    under INVERT every line but the hit is a member"""
    out = []
    for num, hit, terminated in a_shapes():
        data = short_lines(num, (hit,), terminated)
        for before, after in A_WINDOWS:
            for invert in (False, True):
                name = "A-%d-hit%d-b%s-a%s%s%s" % (num, hit, window_name(before), window_name(after), "-inverted" if invert else "",
                                                    "" if terminated else "-unterminated")
                out.append((name, X, data, before, after, invert, others(num, [hit]) if invert else np.asarray([hit], dtype=np.int64)))
    return out


# ---------------------------------------------------------------------------------------------------------------- B: groups across a line-block edge

B_LINES = 2 * BLOCK + 16
# hits on every fourth line: between neighbours, after + before < 3 leaves a gap, = 3 makes the windows touch, > 3 makes them overlap
B_WINDOWS = ((0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2), (2, 1), (1, 2), (3, 0), (0, 3), (2, 2))
B_PHASES = (0, 1, 2, 3)                 # the first hit is 2040 + phase: the edge 2047 | 2048 falls on every place of the period


def b_hits(phase):
    return [lo + phase + 4 * i for lo in (BLOCK - 8, 2 * BLOCK - 8) for i in range(5) if lo + phase + 4 * i <= lo + 16]


# by hand, `e` = 2048 or 4096, the first line of a line block: hits, before, after -> the group of each listed line, the listed lines.  Lines
# e - 1 and e are bit 31 of one line block's last word and bit 0 of the next one's first
B_EDGES = {
    # neighbours on both sides of the edge, no context: one group by the definition of include/pfac_ext.h ("a maximal run of consecutive
    # selected line numbers") -- the group of line e is that of line e - 1, which pfac_lines_select<1> sees only through `carry`
    "neighbours": (lambda e: [e - 1, e], 0, 0, [0, 0], lambda e: [e - 1, e]),
    "a-group-ends-at-the-edge": (lambda e: [e - 1], 3, 0, [0] * 4, lambda e: [e - 4, e - 3, e - 2, e - 1]),
    "a-group-starts-at-the-edge": (lambda e: [e], 0, 3, [0] * 4, lambda e: [e, e + 1, e + 2, e + 3]),
    "the-gap-is-the-last-line-in-front": (lambda e: [e - 2, e], 0, 0, [0, 1], lambda e: [e - 2, e]),
    "the-gap-is-the-first-line-behind": (lambda e: [e - 1, e + 1], 0, 0, [0, 1], lambda e: [e - 1, e + 1]),
    "the-gap-is-the-two-lines-at-the-edge": (lambda e: [e - 3, e + 2], 1, 1, [0] * 3 + [1] * 3, lambda e: [e - 4, e - 3, e - 2, e + 1, e + 2, e + 3]),
    "windows-meet-at-the-edge": (lambda e: [e - 3, e + 2], 2, 2, [0] * 10, lambda e: list(range(e - 5, e + 5))),
}


@functools.lru_cache(maxsize=None)
def aligned_lines(num, hits, e):
    """`num` empty lines, "x" at `hits` (a tuple), and as many "z" lines at the front as it takes for line `e` to start at a multiple of
    32 bytes: with the pointer on a 16-byte boundary a word of the newline bitmap starts with line e, so pfac_lines_select<1> has
    first = e, r = 0 there -- the group of line e is groupBase[e / 2048] + groupRank[e / 32] + 0, and whether it goes on is `carry` alone"""
    pads = -sum(1 for h in hits if h < e) % WORD
    assert all(h >= pads for h in hits) and e >= pads
    lines = [b"x" if k in hits else (b"z" if k < pads else b"") for k in range(num)]
    return b"".join(line + b"\n" for line in lines)


def groups_across_edges():
    """FAMILY B.  groupBase[wi >> 6] + groupRank[wi] and `carry` = bits[wi - 1] >> 31 where wi is a line block's first word"""
    out = []
    for phase in B_PHASES:
        hits = b_hits(phase)
        data = short_lines(B_LINES, tuple(hits))
        for before, after in B_WINDOWS:
            out.append(("B-every-fourth-from-%d-b%d-a%d" % (hits[0], before, after), X, data, before, after, False, np.asarray(hits, dtype=np.int64)))
    for e in (BLOCK, 2 * BLOCK):
        for kind, (hits, before, after, _, _) in B_EDGES.items():
            out.append(("B-%d-%s" % (e, kind), X, aligned_lines(B_LINES, tuple(hits(e)), e), before, after, False, np.asarray(hits(e), dtype=np.int64)))
    return out


def b_by_hand(name):
    """(groups of the listed lines, the listed lines, the members) of a B_EDGES case, None for the others"""
    for e in (BLOCK, 2 * BLOCK):
        for kind, (hits, _, _, groups, listed) in B_EDGES.items():
            if name == "B-%d-%s" % (e, kind):
                return groups, listed(e), hits(e)
    return None


# ---------------------------------------------------------------------------------------------------------------- C: position blocks

C_SIZES = ((GRID_PASS - 1) * BLOCK, GRID_PASS * BLOCK, (2 * GRID_PASS + 1) * BLOCK)       # 16 MiB - 2048, 16 MiB, 32 MiB + 2048: B = 8192, 8193, 16386
C_MIS_SIZE = GRID_PASS * BLOCK - 8      # B = 8192 at a pointer on a 16-byte boundary, 8193 at 15 mod 16
C_WIDE = 1 << 20                        # more lines than any input of the family has
C_WINDOWS = ((0, 0, False), (0, 0, True), (3, 3, False), (C_WIDE, C_WIDE, False))         # (before, after, invert)


def c_sizes(grid):
    """C_SIZES, and for a device whose pass is not GRID_PASS blocks the sizes that stand to its pass as C_SIZES to GRID_PASS"""
    return sorted(set(C_SIZES) | {(grid - 1) * BLOCK, grid * BLOCK, (2 * grid + 1) * BLOCK})


class Text:
    """`size` bytes of lines of 20 to 200 'a' (seeded), the last line unterminated and up to 222 bytes: its virtual newline is position
    q = mis + size, alone in the last block.  `ends`: the position of each line's newline, size for the last line"""

    def __init__(self, size, mis=0, seed=7):
        rng = np.random.Generator(np.random.PCG64(seed))
        ends = np.cumsum(rng.integers(21, 202, size=size // 21 + 1)) - 1
        self.size, self.mis = int(size), int(mis)
        self.ends = np.append(ends[ends < size - 21], size).astype(np.int64)
        self.data = np.full(size, FILL, dtype=np.uint8)
        self.data[self.ends[:-1]] = NL
        self.num_lines = int(self.ends.size)
        self.blocks = position_blocks(size, mis)
        self.hits = []

    def block_of(self, line):
        """the position block line `line` ends in: where pfac_lines_select lists it"""
        return int(self.ends[line] + self.mis) // BLOCK

    def hit_inside(self, block):
        """an 'x' in the first line that lies inside position block `block` with all its bytes"""
        line = int(np.searchsorted(self.ends + self.mis, block * BLOCK, side="left")) + 1
        start = int(self.ends[line - 1]) + 1
        assert (start + self.mis) // BLOCK == block == self.block_of(line) and line < self.num_lines - 1
        self.data[start] = HIT
        self.hits.append(line)

    def hit_last_line(self):
        self.data[self.size - 1] = HIT
        self.hits.append(self.num_lines - 1)

    def H(self, invert=False):
        return others(self.num_lines, self.hits) if invert else np.asarray(sorted(self.hits), dtype=np.int64)


def c_text(size, mis=0, grid=GRID_PASS):
    """the input of family C: hits in the first block, in the last block of the first pass of `grid` blocks, in the first block of the second
    pass, in the last block that holds bytes -- as far as the input has them -- and in the last line, whose newline is the last block"""
    text = Text(size, mis)
    B = text.blocks
    for block in sorted({b for b in (0, grid - 1, grid, B - 2) if 0 <= b <= B - 2}):
        text.hit_inside(block)
    text.hit_last_line()
    return text


def position_block_calls(size, mis=0, grid=GRID_PASS, text=None):
    """FAMILY C.  The calls over one input"""
    text = text or c_text(size, mis, grid)
    return [("C-%d-mis%d-b%d-a%d%s" % (size, mis, before, after, "-inverted" if invert else ""), X, text.data, before, after, invert, text.H(invert))
            for before, after, invert in C_WINDOWS]


# ---------------------------------------------------------------------------------------------------------------- D: line numbers past the scan block

D_LINES = SCAN_BLOCK * BLOCK + 3 * BLOCK + 5
D_HITS = (3, D_LINES - 4)               # in line blocks 0 and 8195
# (0, MAX) and (MAX, 0): every line from line 3 on, every line up to D_LINES - 4 -- each line block takes them from a member more than 8192 line
# blocks away, through the folded front of column 0 and of the back-to-front column 1.  The third reaches from the far member down to line 6138,
# six lines past the nearer one's window; the last keeps the two groups apart
D_WINDOWS = ((0, MAX), (MAX, 0), (BLOCK * SCAN_BLOCK + 7, 2), (5, 5))
D_INVERTED_WINDOWS = ((0, MAX), (MAX, 0), (5, 5))


def far_members(invert=False):
    """FAMILY D.  The input: D_LINES empty lines but for "x" at D_HITS; `invert`: D_LINES lines "x" but for "z" at D_HITS, twice the bytes --
    H is D_HITS in both"""
    if invert:
        data = np.tile(np.asarray([HIT, NL], dtype=np.uint8), D_LINES)
        data[2 * np.asarray(D_HITS)] = OTHER
        return data
    data = np.full(D_LINES + len(D_HITS), NL, dtype=np.uint8)
    data[np.asarray(D_HITS) + np.arange(len(D_HITS))] = HIT              # line k starts behind k newlines and the hits in front of it
    return data


def far_member_calls(invert=False, data=None):
    data = far_members(invert) if data is None else data
    return [("D-b%s-a%s%s" % (window_name(before), window_name(after), "-inverted" if invert else ""), X, data, before, after, invert,
             np.asarray(D_HITS, dtype=np.int64)) for before, after in (D_INVERTED_WINDOWS if invert else D_WINDOWS)]


def by_name(cases):
    out = {c[0]: c for c in cases}
    assert len(out) == len(cases), "case names are unique"
    return out
