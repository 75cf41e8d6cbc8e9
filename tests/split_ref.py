"""Reference for PFACX_split* (include/pfac_ext.h) that does not call the library: the delimiter mask from a 256-entry lookup, the cut rules word
for word as the header states them, in numpy.  And the table of small cases that the host test, the GPU test and tools/split_host_san.cpp's twin
all run under the four flag combinations."""

import numpy as np

BEFORE, RUNS = 1, 2                       # PFACX_SPLIT_BEFORE, PFACX_SPLIT_RUNS
ALL_FLAGS = (0, BEFORE, RUNS, BEFORE | RUNS)
NEWLINE = b"\n"                           # the class of a null h_class


def class_lookup(cls):
    """256 booleans: byte b is in the class.  cls: bytes (or any iterable of byte values); None: {'\\n'}."""
    table = np.zeros(256, dtype=bool)
    members = NEWLINE if cls is None else bytes(cls)
    if len(members):
        table[np.frombuffer(members, dtype=np.uint8)] = True
    return table


def cuts(data, cls=None, flags=0):
    """The cuts of the header's definition, ascending, as uint64."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = data.size
    is_delim = class_lookup(cls)[data]                      # a position p with in[p] in D is a delimiter
    p = np.nonzero(is_delim)[0].astype(np.int64)
    if flags & RUNS:                                        # only one delimiter of each maximal run of delimiters cuts
        if flags & BEFORE:                                  # the first one: in[p - 1] is not in D
            keep = np.ones(p.size, dtype=bool)
            inside = p > 0
            keep[inside] = ~is_delim[p[inside] - 1]
        else:                                               # the last one: in[p + 1] is not in D
            keep = np.ones(p.size, dtype=bool)
            inside = p + 1 < n
            keep[inside] = ~is_delim[p[inside] + 1]
        p = p[keep]
    if flags & BEFORE:
        c = p[p > 0]                                        # every delimiter p with p > 0 gives the cut p
    else:
        c = p[p + 1 < n] + 1                                # every delimiter p with p + 1 < n gives the cut p + 1
    return c.astype(np.uint64)


def split(data, cls=None, flags=0):
    """-> (offsets: 0, the cuts, n as uint64 -- empty for an empty input --, number of segments, longest segment)."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = data.size
    if n == 0:
        return np.zeros(0, dtype=np.uint64), 0, 0
    c = cuts(data, cls, flags)
    offsets = np.concatenate([np.zeros(1, dtype=np.uint64), c, np.full(1, n, dtype=np.uint64)])
    lengths = np.diff(offsets.astype(np.int64))
    assert np.all(lengths > 0), "no segment is ever empty"
    assert np.all(c > 0) and np.all(c < n), "cuts lie strictly inside (0, n)"
    return offsets, int(c.size) + 1, int(lengths.max())


EMPTY_CLASS = b""
FULL_CLASS = bytes(range(256))

# (name, text, class; None: the default class)
TABLE = [
    ("empty", b"", None),
    ("one newline", b"\n", None),
    ("one byte", b"a", None),
    ("terminated", b"a\n", None),
    ("newline first", b"\na", None),
    ("only newlines", b"\n\n\n", None),
    ("blank line", b"a\n\nb", None),
    ("crlf", b"a\r\nb\r\n", b"\r\n"),
    ("empty class", b"no cut\nanywhere\n", EMPTY_CLASS),
    ("full class", b"every byte", FULL_CLASS),
    ("csv", b"id,name,,value\n7,x,,\n", b",\n"),
]

# what the definition gives for some of them, written out by hand: (name, flags) -> offsets
BY_HAND = {
    ("one newline", 0): [0, 1],
    ("terminated", 0): [0, 2],
    ("terminated", BEFORE): [0, 1, 2],
    ("newline first", 0): [0, 1, 2],
    ("newline first", BEFORE): [0, 2],
    ("only newlines", 0): [0, 1, 2, 3],
    ("only newlines", BEFORE): [0, 1, 2, 3],
    ("only newlines", RUNS): [0, 3],
    ("only newlines", BEFORE | RUNS): [0, 3],
    ("blank line", 0): [0, 2, 3, 4],
    ("blank line", BEFORE): [0, 1, 2, 4],
    ("blank line", RUNS): [0, 3, 4],
    ("blank line", BEFORE | RUNS): [0, 1, 4],
    ("crlf", 0): [0, 2, 3, 5, 6],
    ("crlf", RUNS): [0, 3, 6],
    ("crlf", BEFORE | RUNS): [0, 1, 4, 6],
    ("empty class", 0): [0, 16],
    ("full class", 0): list(range(11)),
    ("full class", RUNS): [0, 10],
}


def table_cases():
    """(id, data as uint8, class, flags, expected offsets, segments, longest) for every text under every flag combination."""
    for name, text, cls in TABLE:
        data = np.frombuffer(text, dtype=np.uint8)
        for flags in ALL_FLAGS:
            offsets, segments, longest = split(data, cls, flags)
            if (name, flags) in BY_HAND:
                assert offsets.tolist() == BY_HAND[(name, flags)], (name, flags, offsets.tolist())
            yield "%s-%d" % (name.replace(" ", "_"), flags), data, cls, flags, offsets, segments, longest


def random_case(rng, size, members):
    """`size` bytes that hold delimiters singly and in runs, and a class of `members` byte values."""
    cls = bytes(rng.choice(256, size=members, replace=False).astype(np.uint8).tolist())
    data = rng.integers(0, 256, size=size, dtype=np.uint8)
    if size and members <= 3:                                # a few delimiters of a small class, some of them in runs
        at = rng.integers(0, size, size=max(1, size // 40))
        data[at] = rng.choice(np.frombuffer(cls, dtype=np.uint8), size=at.size)
        for start in rng.integers(0, size, size=max(1, size // 400)):
            data[start:start + int(rng.integers(2, 6))] = cls[0]
    return data, cls


def make_log(lines=200, seed=5):
    """a small log and a 20-pattern set over its words -> (data, pattern bytes, rules as (rule_off, rule_patterns))"""
    rng = np.random.Generator(np.random.PCG64(seed))
    words = [b"ERROR", b"WARN", b"INFO", b"payment-service", b"auth-service", b"timeout", b"retry", b"refused", b"user=", b"GET ",
             b"POST ", b"/admin", b"/login", b"500", b"404", b"200", b"disk", b"full", b"ERR", b"pay"]
    filler = [b"the", b"request", b"took", b"ms", b"id", b"42", b"from", b"10.0.0.7"]
    out = []
    for _ in range(lines):
        parts = []
        for _ in range(int(rng.integers(0, 9))):
            pool = words if rng.random() < 0.4 else filler
            parts.append(pool[int(rng.integers(0, len(pool)))])
        out.append(b" ".join(parts))
    data = np.frombuffer(b"\n".join(out) + b"\n", dtype=np.uint8)
    rule_off = [0, 2, 4, 5, 8]
    rule_patterns = [1, 4, 2, 6, 12, 10, 13, 14]          # ERROR + payment-service, WARN + timeout, /admin, GET + /login + 500
    return data, b"".join(w + b"\n" for w in words), (rule_off, rule_patterns)
