"""Two models of PFACX_orderHits* that share no code with the library or with each other, and the lists both test files use.

(a) numpy: np.lexsort (a stable sort, last key first) over int64 keys, or np.argsort(kind="stable") without the ties flag;
(b) pure Python: sorted(range(n), key=...) -- Python's sort is stable, the key a tuple of Python ints.

Both return the permutation: perm[k] = the incoming index of the entry that ends up at k.  A list was ordered iff that is the identity (for a
stable sort the identity is the answer exactly when no entry has to go in front of its predecessor)."""

import numpy as np

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def perm_numpy(starts, ids=None, ties=False):
    s = np.asarray(starts, dtype=np.int64)
    if ties:
        return np.lexsort((np.asarray(ids, dtype=np.int64), s)).astype(np.int32)
    return np.argsort(s, kind="stable").astype(np.int32)


def perm_python(starts, ids=None, ties=False):
    s = [int(v) for v in starts]
    if ties:
        i = [int(v) for v in ids]
        return sorted(range(len(s)), key=lambda k: (s[k], i[k]))
    return sorted(range(len(s)), key=lambda k: s[k])


def model(starts, ids=None, ends=None, aux=None, ties=False, python_too=True):
    """-> (the given columns permuted, in the order starts, ids, ends, aux ..., perm, was_ordered); both models must agree"""
    perm = perm_numpy(starts, ids, ties)
    if python_too:
        assert perm.tolist() == perm_python(starts, ids, ties), "the two models disagree"
    cols = [np.asarray(c, dtype=np.int32)[perm] for c in (starts, ids, ends, aux) if c is not None]
    was = int(np.array_equal(perm, np.arange(perm.size)))
    return (*cols, perm, was)


def same(got, want, what=""):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got[:-1], want[:-1])):
        assert np.array_equal(np.asarray(g), np.asarray(w)), (what, "column" if k < len(got) - 2 else "perm", k)
    assert int(got[-1]) == int(want[-1]), (what, "was_ordered")


# every combination of the optional columns: (ids, ends, aux) given or not
COLUMN_COMBINATIONS = [(i, e, a) for i in (False, True) for e in (False, True) for a in (False, True)]


def pick_columns(starts, ids, ends, aux, combo):
    return starts, (ids if combo[0] else None), (ends if combo[1] else None), (aux if combo[2] else None)


def random_list(seed, n=None):
    """a seeded list with many equal starts and equal (start, id): (starts, ids, ends, aux), aux = arange"""
    rng = np.random.RandomState(seed)
    n = int(rng.randint(2, 400)) if n is None else n
    kind = seed % 4
    if kind == 0:
        starts = rng.randint(0, max(2, n // 4), size=n)
    elif kind == 1:
        starts = rng.randint(-50, 50, size=n)
    elif kind == 2:
        starts = rng.choice([INT_MIN, INT_MIN + 1, -1, 0, 1, INT_MAX - 1, INT_MAX], size=n)
    else:
        starts = rng.randint(INT_MIN, INT_MAX, size=n, dtype=np.int64)
    ids = rng.choice([INT_MIN, -3, 0, 1, 2, 3, 70000, INT_MAX], size=n) if seed % 3 == 0 else rng.randint(1, 6, size=n)
    ends = starts.astype(np.int64) + rng.randint(1, 30, size=n)
    ends = np.clip(ends, INT_MIN, INT_MAX)
    return starts.astype(np.int32), ids.astype(np.int32), ends.astype(np.int32), np.arange(n, dtype=np.int32)


RANDOM_SEEDS = list(range(60))

# (name, starts, ids): by hand
HAND = [
    ("two swapped", [5, 3], [1, 2]),
    ("ties keep incoming order", [4, 4, 4, 1, 1], [9, 8, 7, 6, 5]),
    ("extremes", [INT_MAX, INT_MIN, 0, -1, 1, INT_MIN, INT_MAX], [INT_MIN, INT_MAX, 0, -1, 1, INT_MIN, INT_MAX]),
    ("negative starts", [-1, -2 ** 30, -2, -1, -2], [3, 2, 1, 0, -1]),
    ("sign bit only", [5, 5 + INT_MIN, 5, 5 + INT_MIN], [1, 1, 1, 1]),
    ("ids descending inside each start", [7, 7, 7, 2, 2, 2], [3, 2, 1, 3, 2, 1]),
    ("equal (start, id) runs", [7, 7, 7, 7, 2, 2], [2, 1, 2, 1, 5, 5]),
    ("all starts equal", [9] * 6, [6, 5, 4, 3, 2, 1]),
    ("strictly descending", list(range(40, 0, -1)), list(range(1, 41))),
    ("already ordered", [1, 1, 2, 3, 3, 3], [1, 1, 1, 2, 4, 4]),
    ("ordered by start, not by id", [1, 1, 2, 3, 3, 3], [2, 1, 1, 2, 4, 3]),
]


# ---------------------------------------------------------------- real lists that are NOT in start order

# class signatures (over tests/cover_ref.py: token_text): the first rule starts up to 20 bytes in front of its anchor, the last one has its
# anchor inside that stretch -- the anchor order of the list is not the start order
CLSIG_RULES = [b"[e-k ]{4,20}AKIA[0-9A-Z]{4}", b"(?<![0-9])[0-9]{3}-[0-9]{2}-[0-9]{4}(?![0-9])", b"xox[baprs]-[0-9a-z]{10,20}(?![0-9a-z])",
               b" e[e-k]{0,3}"]

# edit distance: the long pattern is found through its second piece where its first one holds the edit, and the two short ones occur inside it
EDIT_PATTERNS, EDIT_BUDGETS = [b"gattacacctgaagtc", b"tacacctg", b"cctgaagt"], [1, 0, 0]


def edit_text(seed, size):
    rng = np.random.RandomState(seed)
    text = bytearray(np.frombuffer(b"acgt", dtype=np.uint8)[rng.randint(0, 4, size=size)].tobytes())
    at = 5
    while at + 40 < size:
        tok = bytearray(EDIT_PATTERNS[0])
        kind = rng.randint(0, 3)
        if kind == 0:
            tok[int(rng.randint(0, 8))] = ord("n")
        elif kind == 1:
            del tok[int(rng.randint(8, 16))]
        text[at:at + len(tok)] = tok
        at += len(tok) + int(rng.randint(1, 50))
    return bytes(text[:size])


# masked signatures: the first one starts three wildcards in front of its anchor
SIG_TEXT = b"?? ?? ?? 74 74 61\n61 ?? 67 74\n63 63 ?? ?? 61\n"
