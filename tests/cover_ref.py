"""Two models of PFACX_coverSpans* that share no code with the library or with each other, and the lists both test files use.

  spans_by_map    a numpy bool array of `size` entries filled interval by interval, the runs taken from np.diff
  spans_by_sweep  the clamped intervals sorted by start and swept with a running maximum end, in Python integers

model() runs both and asserts that they agree; every comparison against the library is exact."""

import numpy as np

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def ends_of(starts, second, lengths):
    """the exclusive ends as Python integers: `second` itself, or start + length without any 32-bit wrap"""
    return [int(s) + int(x) if lengths else int(x) for s, x in zip(starts, second)]


def spans_by_map(starts, second, size, lengths=False):
    covered = np.zeros(size + 2, dtype=bool)                    # entry b + 1: byte b; a False on either side
    for s, e in zip(starts, ends_of(starts, second, lengths)):
        lo, hi = max(int(s), 0), min(e, size)
        if lo < hi:
            covered[lo + 1:hi + 1] = True
    step = np.diff(covered.astype(np.int8))
    first = np.nonzero(step == 1)[0]
    behind = np.nonzero(step == -1)[0]
    return first.astype(np.int64), (behind - first).astype(np.int64), int(covered.sum())


def spans_by_sweep(starts, second, size, lengths=False):
    kept = sorted((max(int(s), 0), min(e, size)) for s, e in zip(starts, ends_of(starts, second, lengths)) if max(int(s), 0) < min(e, size))
    out = []
    for lo, hi in kept:
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return (np.array([o[0] for o in out], dtype=np.int64), np.array([o[1] - o[0] for o in out], dtype=np.int64),
            sum(o[1] - o[0] for o in out))


def model(starts, second, size, lengths=False):
    """(span starts, span lengths, covered bytes) by both models, asserted equal"""
    a = spans_by_map(starts, second, size, lengths)
    b = spans_by_sweep(starts, second, size, lengths)
    assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist() and a[2] == b[2], "the two models disagree"
    assert len(a[0]) <= (size + 1) // 2 and all(n >= 1 for n in a[1].tolist())
    assert all(s0 + n0 < s1 for s0, n0, s1 in zip(a[0].tolist(), a[1].tolist(), a[0].tolist()[1:])), "spans touch or descend"
    return a


def model_sweep_only(starts, second, size, lengths=False):
    """the sweep alone, for a `size` no byte map should be made of"""
    return spans_by_sweep(starts, second, size, lengths)


def same(got, want, what):
    assert got[0].tolist() == want[0].tolist(), f"{what}: span starts"
    assert got[1].tolist() == want[1].tolist(), f"{what}: span lengths"
    assert int(got[2]) == int(want[2]), f"{what}: covered bytes"


def as_lengths(starts, ends):
    """a list of (start, end) as (start, length) wherever the length fits an int; None where one does not"""
    lens = [int(e) - int(s) for s, e in zip(starts, ends)]
    return lens if all(INT_MIN <= n <= INT_MAX for n in lens) else None


# hostile entries over size = 100: (name, starts, second array, lengths flag)
HOSTILE_SIZE = 100
HOSTILE = [
    ("negative start", [-5], [7], False),
    ("negative start and end", [-9], [-3], False),
    ("end beyond size", [90], [250], False),
    ("both outside", [-4], [400], False),
    ("e == s", [40], [40], False),
    ("e < s", [60], [20], False),
    ("s == size", [100], [130], False),
    ("s > size", [170], [180], False),
    ("e == 0", [-3], [0], False),
    ("INT_MIN start", [INT_MIN], [3], False),
    ("INT_MIN both", [INT_MIN], [INT_MIN], False),
    ("INT_MAX end", [10], [INT_MAX], False),
    ("INT_MIN to INT_MAX", [INT_MIN], [INT_MAX], False),
    ("INT_MAX start", [INT_MAX], [INT_MAX], False),
    ("descending INT_MAX to INT_MIN", [INT_MAX], [INT_MIN], False),
    ("length overflows 32 bits", [50], [INT_MAX], True),
    ("length overflows 32 bits at INT_MAX", [INT_MAX], [INT_MAX], True),
    ("negative length", [50], [-10], True),
    ("zero length", [50], [0], True),
    ("INT_MIN length", [70], [INT_MIN], True),
    ("negative start, length reaches in", [-5], [10], True),
    ("negative start, length does not", [-5], [5], True),
    ("INT_MIN start, INT_MAX length", [INT_MIN], [INT_MAX], True),
    ("mixed", [-5, 98, 30, 60, INT_MIN, 20, 100], [2, 1000, 30, 20, INT_MAX - 5, 25, 101], False),
    ("mixed lengths", [-5, 98, 30, 60, 20, 100, 7], [7, INT_MAX, 0, -40, 5, 1, 1], True),
]

# duplicates, nesting, touching and overlapping pairs over size = 64: (name, starts, ends)
SHAPES_SIZE = 64
SHAPES = [
    ("duplicates", [5, 5, 5], [9, 9, 9]),
    ("duplicate starts", [5, 5, 5], [9, 7, 12]),
    ("nested", [10, 12, 11], [30, 14, 29]),
    ("nested, inner first", [12, 10], [14, 30]),
    ("touching", [3, 8], [8, 11]),
    ("touching, given backwards", [8, 3], [11, 8]),
    ("a gap of one", [3, 9], [8, 11]),
    ("overlap", [3, 6], [8, 11]),
    ("a chain that touches", [0, 4, 8, 12, 16], [4, 8, 12, 16, 20]),
    ("the whole range twice", [0, 0], [64, 64]),
    ("first and last byte", [0, 63], [1, 64]),
    ("all but the ends", [1], [63]),
]


def alternating(size):
    """[2 i, 2 i + 1) for every i that fits: (size + 1) // 2 spans of one byte"""
    starts = list(range(0, size, 2))
    return starts, [s + 1 for s in starts]


def random_list(seed):
    """a seeded list over a seeded size: mostly short intervals, some long, some hostile -> (starts, ends, size)"""
    rng = np.random.RandomState(seed)
    size = int(rng.choice([1, 2, 31, 32, 33, 64, 100, 257, 1000, 4097, 70000]))
    count = int(rng.randint(1, 60))
    starts, ends = [], []
    for _ in range(count):
        kind = rng.randint(0, 10)
        s = int(rng.randint(-3, size + 3))
        if kind < 6:
            e = s + int(rng.randint(-2, 12))
        elif kind < 8:
            e = s + int(rng.randint(0, size + 1))
        elif kind == 8:
            e = s                                       # empty
        else:
            s, e = int(rng.randint(-size, 1)), int(rng.randint(size - 2, 2 * size + 2))
        starts.append(s)
        ends.append(e)
    return starts, ends, size


RANDOM_SEEDS = list(range(200))


# ---------------------------------------------------------------- the cross-checks against the library's own calls

# a plain set with patterns that are prefixes of one another, and a text full of them
PREFIX_PATTERNS = [b"ab", b"abc", b"abcd", b"b", b"bcd", b"dd"]


def prefix_text(seed, size):
    return np.frombuffer(b"abcd ", dtype=np.uint8)[np.random.RandomState(seed).randint(0, 5, size=size)].copy()


# three token rules no two of whose matches overlap, so that re.sub finds exactly what the library lists
CLSIG_RULES = [b"(?<![0-9A-Z])AKIA[0-9A-Z]{16}(?![0-9A-Z])", b"(?<![0-9])[0-9]{3}-[0-9]{2}-[0-9]{4}(?![0-9])",
               b"xox[baprs]-[0-9a-z]{10,20}(?![0-9a-z])"]


def token_text(seed, size):
    """filler without digits or capitals, and seeded tokens of the three rules: most between blanks, some run into their neighbours"""
    rng = np.random.RandomState(seed)
    text = bytearray(np.frombuffer(b"efghijk .,\n", dtype=np.uint8)[rng.randint(0, 11, size=size)].tobytes())
    upper, digits, lower = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789", b"0123456789", b"abcdefghijklmnopqrstuvwxyz0123456789"

    def pick(alphabet, n):
        return bytes(alphabet[i] for i in rng.randint(0, len(alphabet), size=n))

    at = 3
    while at + 40 < size:
        kind = rng.randint(0, 3)
        if kind == 0:
            tok = b"AKIA" + pick(upper, 16)
        elif kind == 1:
            tok = pick(digits, 3) + b"-" + pick(digits, 2) + b"-" + pick(digits, 4)
        else:
            tok = b"xox" + pick(b"baprs", 1) + b"-" + pick(lower, int(rng.randint(8, 24)))
        glue = rng.randint(0, 6)
        if glue == 0 and kind != 2:
            tok = tok + tok                                     # two tokens that touch: the boundary classes decide (never two of the third rule:
                                                                # the first would run into the second, and re.sub skips what overlaps)
        elif glue == 1:
            tok = pick(digits, 1) + tok
        text[at:at + len(tok)] = tok
        at += len(tok) + int(rng.randint(1, 60))
    return bytes(text[:size])


# ---------------------------------------------------------------- word and thread edges, worked out by hand

# Over size = 200: the words of the bitmap end at 32, 64, ..., a thread's 16 bytes of it at 128.  (intervals as (start, end), spans as (start, length))
EDGE_SIZE = 200
EDGE_TABLE = [
    ([(0, 1)], [(0, 1)]),
    ([(0, 200)], [(0, 200)]),
    ([(1, 199)], [(1, 198)]),
    ([(199, 200)], [(199, 1)]),
    ([(0, 1), (199, 200)], [(0, 1), (199, 1)]),
    ([(15, 16)], [(15, 1)]),
    ([(15, 17)], [(15, 2)]),
    ([(16, 17), (15, 16)], [(15, 2)]),
    ([(15, 16), (17, 31)], [(15, 1), (17, 14)]),
    ([(31, 32)], [(31, 1)]),
    ([(32, 33)], [(32, 1)]),
    ([(31, 33)], [(31, 2)]),
    ([(31, 32), (32, 33)], [(31, 2)]),
    ([(31, 32), (33, 63)], [(31, 1), (33, 30)]),
    ([(0, 32)], [(0, 32)]),
    ([(0, 31)], [(0, 31)]),
    ([(1, 32)], [(1, 31)]),
    ([(0, 33)], [(0, 33)]),
    ([(32, 64)], [(32, 32)]),
    ([(0, 32), (32, 64)], [(0, 64)]),
    ([(0, 32), (33, 64)], [(0, 32), (33, 31)]),
    ([(0, 31), (32, 64)], [(0, 31), (32, 32)]),
    ([(0, 64)], [(0, 64)]),
    ([(1, 63)], [(1, 62)]),
    ([(1, 65)], [(1, 64)]),
    ([(63, 65)], [(63, 2)]),
    ([(63, 64), (64, 65)], [(63, 2)]),
    ([(63, 64), (65, 127)], [(63, 1), (65, 62)]),
    ([(64, 128)], [(64, 64)]),
    ([(0, 128)], [(0, 128)]),
    ([(0, 127)], [(0, 127)]),
    ([(127, 128)], [(127, 1)]),
    ([(128, 200)], [(128, 72)]),
    ([(127, 200)], [(127, 73)]),
    ([(0, 128), (128, 199)], [(0, 199)]),
    ([(0, 127), (128, 200)], [(0, 127), (128, 72)]),
    ([(17, 127), (33, 65), (16, 17)], [(16, 111)]),
    ([(0, 1), (15, 16), (31, 32), (63, 64), (127, 128), (199, 200)], [(0, 1), (15, 1), (31, 1), (63, 1), (127, 1), (199, 1)]),
    ([(1, 15), (16, 17), (32, 33), (64, 65), (128, 199)], [(1, 14), (16, 1), (32, 1), (64, 1), (128, 71)]),
    ([(1, 15), (15, 16), (16, 17), (17, 31), (31, 32), (32, 33), (33, 63), (63, 64), (64, 65), (65, 127), (127, 128), (128, 199)], [(1, 198)]),
    ([(128, 199), (65, 127), (33, 63), (17, 31), (1, 15)], [(1, 14), (17, 14), (33, 30), (65, 62), (128, 71)]),
    ([(32, 128), (0, 16)], [(0, 16), (32, 96)]),
    ([(33, 127), (0, 17), (199, 200), (198, 199)], [(0, 17), (33, 94), (198, 2)]),
]
