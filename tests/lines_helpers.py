"""Helpers shared by tests/test_lines_host.py and tests/test_lines_gpu.py: pattern files, the host call over poisoned arrays.  Test
infrastructure only."""
import os

import numpy as np

from pfac_amd import api


def pattern_file(workdir, name, pats):
    path = os.path.join(workdir, "lines_" + name + ".pat")
    with open(path, "wb") as f:
        f.write(b"".join(bytes(p) + b"\n" for p in pats))
    return path


def host_lines(h, data, invert, with_index=True):
    """matchLinesFromHost over poisoned arrays of capacity == size -> ((numLines, start, len, index), the input bytes after the call)"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    n = buf.size
    cap = max(n, 1)
    start, length, index = (np.full(cap, -7, dtype=np.int32) for _ in range(3))
    st, nl, ns = h.matchLinesFromHost(buf.ctypes.data if n else start.ctypes.data, n, api.PFACX_LINES_INVERT if invert else 0, start.ctypes.data,
                                      length.ctypes.data, index.ctypes.data if with_index else None, n)
    assert st == 0 and ns <= nl <= n
    if not with_index:
        assert np.all(index == -7)
    return (nl, start[:ns].copy(), length[:ns].copy(), index[:ns].copy()), buf.tobytes()
