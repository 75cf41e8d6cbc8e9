"""Reference for PFACX_capture* (include/pfac_ext.h) that does not call the library: the six rules of the header, byte by byte and deliberately
naive, and a table of small cases written out by hand that pins the reference itself."""

import numpy as np

AT_POS = 1


def members(cls, default):
    """a class given as bytes (or None: the default) -> a set of byte values"""
    return set(default if cls is None else bytes(cls))


def capture(data, ids, positions, lens, skip=None, stop=None, window=0, flags=0):
    """-> (valStart, valLen) as int32.  `lens`: the pattern lengths by id, [0] unused (F = len(lens) - 1); `ids` and `lens` may be None with AT_POS;
    `skip`: bytes or None (empty), `stop`: bytes or None ({'\\n'})."""
    data = bytes(np.ascontiguousarray(data, dtype=np.uint8).tobytes())
    n = len(data)
    D = members(stop, b"\n")
    S = members(skip, b"") - D                                             # a byte in both classes is a stop byte only
    start, length = [], []
    for k, p in enumerate(int(x) for x in positions):
        if p < 0 or p >= n:                                                # rule 1
            start.append(-1)
            length.append(0)
            continue
        if flags & AT_POS:
            b = p
        else:
            i = int(ids[k])
            if i < 1 or i > len(lens) - 1:
                start.append(-1)
                length.append(0)
                continue
            b = p + int(lens[i])                                           # rule 2
        b = min(b, n)
        w = n if window == 0 else min(n, b + window)                       # rule 3
        s = b
        while s < w and data[s] in S:                                      # rule 4
            s += 1
        e = s
        while e < w and data[e] not in D:                                  # rule 5
            e += 1
        start.append(s)                                                    # rule 6
        length.append(e - s)
    return np.asarray(start, dtype=np.int32), np.asarray(length, dtype=np.int32)


def values_text(data, val_start, val_len):
    """the values as PFACX_gatherLinesFromDevice writes them: one per line, an entry with valStart == -1 an empty line"""
    data = bytes(np.ascontiguousarray(data, dtype=np.uint8).tobytes())
    out = bytearray()
    for s, ln in zip((int(x) for x in val_start), (int(x) for x in val_len)):
        s = max(s, 0)
        out += data[s:s + max(ln, 0)] + b"\n"
    return bytes(out)


def pattern_file(patterns):
    """the patterns, one per line, and their lengths by id"""
    return b"".join(p + b"\n" for p in patterns), [0] + [len(p) for p in patterns]


#        H o s t : _ a . b \r \n u  s  e  r  =  b  o  b  \n x  =  _  _  \n _  k  =  v
#        0 1 2 3 4 5 6 7 8 9  10 11 12 13 14 15 16 17 18 19 20 21 22 23 24 25 26 27 28      n = 29
TEXT = b"Host: a.b\r\nuser=bob\nx=  \n k=v"
KEYS = [b"Host:", b"user=", b"x=", b"k="]                                  # ids 1 .. 4
KEY_PAIRS = [(1, 0), (2, 11), (3, 20), (4, 26)]
#        a b c = 1 ; a b = 2 ;
#        0 1 2 3 4 5 6 7 8 9 10     n = 11
TWICE = b"abc=1;ab=2;"
EVERY_BYTE = bytes(range(256))

# (text, patterns, skip, stop, window, flags, pairs (id, pos)) -> (valStart, valLen) pairs, by hand
BY_HAND = [
    # blanks skipped, CRLF and LF stops, an empty value behind blanks, a value that the input's end closes
    (TEXT, KEYS, b" \t", b"\r\n", 0, 0, KEY_PAIRS, [(6, 3), (16, 3), (24, 0), (28, 1)]),
    # nothing skipped, the default stop: up to the '\n' of the line, the '\r' and the blanks are part of the value
    (TEXT, KEYS, None, None, 0, 0, KEY_PAIRS, [(5, 5), (16, 3), (22, 2), (28, 1)]),
    # the position as it is: a whole line, a position on the stop byte, the last byte, n and -1
    (TEXT, None, None, None, 0, AT_POS, [(0, 0), (0, 10), (0, 11), (0, 28), (0, 29), (0, -1)], [(0, 10), (10, 0), (11, 8), (28, 1), (-1, 0), (-1, 0)]),
    # a window of 2: it ends the value, and it is spent on blanks
    (TEXT, KEYS, b" ", b"\r\n", 2, 0, [(1, 0), (3, 20)], [(6, 1), (24, 0)]),
    # w one in front of the stop byte, and on it
    (TEXT, KEYS, b" ", b"\r\n", 4, 0, [(1, 0)], [(6, 3)]),
    (TEXT, KEYS, b" ", b"\r\n", 5, 0, [(1, 0)], [(6, 3)]),
    # a window larger than the input changes nothing
    (TEXT, KEYS, b" \t", b"\r\n", 1000, 0, KEY_PAIRS, [(6, 3), (16, 3), (24, 0), (28, 1)]),
    # a byte in both classes is a stop byte only; in the skip class alone it is skipped
    (TEXT, None, b" \n", b"\n", 0, AT_POS, [(0, 22)], [(24, 0)]),
    (TEXT, None, b" \n", b"=", 0, AT_POS, [(0, 22)], [(26, 1)]),
    # ids the set does not have give nothing
    (TEXT, KEYS, b" ", b"\r\n", 0, 0, [(0, 0), (5, 0), (-1, 0), (1, 0)], [(-1, 0), (-1, 0), (-1, 0), (6, 3)]),
    # a match that ends with the input, and a length that reaches beyond it
    (b"ab", [b"ab"], None, None, 0, 0, [(1, 0)], [(2, 0)]),
    (b"ab", [b"abcde"], None, None, 0, 0, [(1, 0)], [(2, 0)]),
    # every byte a skip byte and no stop byte: the window, or the input, is spent
    (TEXT, None, EVERY_BYTE, b"", 0, AT_POS, [(0, 3)], [(29, 0)]),
    (TEXT, None, EVERY_BYTE, b"", 4, AT_POS, [(0, 3)], [(7, 0)]),
    # no skip byte and no stop byte: the rest of the input
    (TEXT, None, None, b"", 0, AT_POS, [(0, 3)], [(3, 26)]),
    # two pairs at one position with different ids, as PFACX_matchAll* lists them
    (TWICE, [b"abc=", b"ab"], b"=", b";", 0, 0, [(1, 0), (2, 0), (2, 6)], [(4, 1), (2, 3), (9, 1)]),
    # a long pattern at a lower position ends behind a short one at a higher position
    (b"abcdefgh\n", [b"abcdef", b"c"], None, None, 0, 0, [(1, 0), (2, 2)], [(6, 2), (3, 5)]),
]


def table_cases():
    """(data as uint8, pattern file or None, lens or None, skip, stop, window, flags, ids, pos as int32, valStart, valLen), each asserted against
    the reference"""
    for text, patterns, skip, stop, window, flags, pairs, expected in BY_HAND:
        data = np.frombuffer(text, dtype=np.uint8)
        file, lens = pattern_file(patterns) if patterns is not None else (None, None)
        ids = np.asarray([i for i, _ in pairs], dtype=np.int32)
        pos = np.asarray([p for _, p in pairs], dtype=np.int32)
        start, length = capture(data, ids, pos, lens, skip, stop, window, flags)
        assert list(zip(start.tolist(), length.tolist())) == expected, (text, skip, stop, window, flags, start.tolist(), length.tolist())
        yield data, file, lens, skip, stop, window, flags, ids, pos, start, length
