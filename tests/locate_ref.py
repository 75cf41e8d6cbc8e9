"""Reference for PFACX_locate* (include/pfac_ext.h) that does not call the library: the offsets of tests/split_ref.py and a searchsorted over
them -- the header's "equivalently" -- and a table of small cases written out by hand that pins the reference itself."""

import numpy as np

from tests import split_ref

BEFORE, RUNS, ALL_FLAGS = split_ref.BEFORE, split_ref.RUNS, split_ref.ALL_FLAGS


def locate(data, positions, cls=None, flags=0):
    """-> (records, columns as int32, number of records): record = (the number of offsets <= p) - 1, column = p - offsets[record]; -1 both for a
    position outside [0, n)."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    pos = np.asarray(positions, dtype=np.int64)
    offsets, segments, _ = split_ref.split(data, cls, flags)
    record = np.full(pos.size, -1, dtype=np.int32)
    column = np.full(pos.size, -1, dtype=np.int32)
    inside = (pos >= 0) & (pos < data.size)
    if data.size and inside.any():
        off = offsets.astype(np.int64)
        r = np.searchsorted(off, pos[inside], side="right") - 1
        record[inside] = r
        column[inside] = pos[inside] - off[r]
    return record, column, segments


TEXT = b"ab\ncd\n\nxyz"                    # a b \n c d \n \n x y z: newlines at 2, 5, 6
EVERY = list(range(len(TEXT)))
CRLF = b"a\r\nbc\r\n\r\nd"                 # a \r \n b c \r \n \r \n d

# (text, class; None: the default, flags, positions) -> (records, columns), by hand
BY_HAND = [
    (TEXT, None, 0, EVERY, [0, 0, 0, 1, 1, 1, 2, 3, 3, 3], [0, 1, 2, 0, 1, 2, 0, 0, 1, 2]),                     # cuts 3, 6, 7: the '\n' ends its line
    (TEXT, None, BEFORE, EVERY, [0, 0, 1, 1, 1, 2, 3, 3, 3, 3], [0, 1, 0, 1, 2, 0, 0, 1, 2, 3]),                # cuts 2, 5, 6: the '\n' opens a record
    (TEXT, None, RUNS, EVERY, [0, 0, 0, 1, 1, 1, 1, 2, 2, 2], [0, 1, 2, 0, 1, 2, 3, 0, 1, 2]),                  # cuts 3, 7
    (TEXT, None, BEFORE | RUNS, EVERY, [0, 0, 1, 1, 1, 2, 2, 2, 2, 2], [0, 1, 0, 1, 2, 0, 1, 2, 3, 4]),         # cuts 2, 5
    (TEXT, None, 0, [-3, -1, 0, 0, 2, 3, 3, 9, 10, 11], [-1, -1, 0, 0, 0, 1, 1, 3, -1, -1], [-1, -1, 0, 0, 2, 0, 0, 2, -1, -1]),
    (TEXT, b"", 0, [0, 4, 9], [0, 0, 0], [0, 4, 9]),                                                            # the empty class: one record
    (CRLF, b"\r\n", RUNS, list(range(10)), [0, 0, 0, 1, 1, 1, 1, 1, 1, 2], [0, 1, 2, 0, 1, 2, 3, 4, 5, 0]),     # cuts 3, 9
    (CRLF, b"\r\n", 0, [0, 2, 3, 8, 9], [0, 1, 2, 5, 6], [0, 0, 0, 0, 0]),                                      # cuts 2, 3, 6, 7, 8, 9
    (b"x", None, 0, [0], [0], [0]),
    (b"\n", None, 0, [0], [0], [0]),
]


def table_cases():
    """(data as uint8, class, flags, positions as int32, records, columns, number of records), each asserted against the reference"""
    for text, cls, flags, positions, records, columns in BY_HAND:
        data = np.frombuffer(text, dtype=np.uint8)
        record, column, segments = locate(data, positions, cls, flags)
        assert record.tolist() == records and column.tolist() == columns, (text, cls, flags, record.tolist(), column.tolist())
        yield data, cls, flags, np.asarray(positions, dtype=np.int32), record, column, segments
