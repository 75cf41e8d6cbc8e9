"""Helpers shared by tests/test_spans_host.py and tests/test_spans_gpu.py: pattern files, the host call over poisoned arrays with guard words
behind capacity, the seeded random cases.  Test infrastructure only."""
import os

import numpy as np

GUARD = 64


def pattern_file(workdir, name, pats):
    path = os.path.join(workdir, "spans_" + name + ".pat")
    with open(path, "wb") as f:
        f.write(b"".join(bytes(p) + b"\n" for p in pats))
    return path


def host_spans(h, data):
    """matchSpansFromHost over poisoned arrays of capacity == size (+ GUARD) -> ((start, len), covered bytes, the input bytes after the call)"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    n = buf.size
    start, length = (np.full(n + GUARD, -7, dtype=np.int32) for _ in range(2))
    st, ns, cb = h.matchSpansFromHost(buf.ctypes.data if n else start.ctypes.data, n, start.ctypes.data, length.ctypes.data, n)
    assert st == 0 and ns <= (n + 1) // 2
    assert np.all(start[n:] == -7) and np.all(length[n:] == -7), "wrote behind capacity"
    return (start[:ns].copy(), length[:ns].copy()), cb, buf.tobytes()


def random_case(seed):
    """(patterns, data): an alphabet of 2 - 3 letters, 1 - 40 patterns of 1 - 40 bytes, an input of 1 - 20 000 bytes"""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    letters = np.frombuffer(b"abc", dtype=np.uint8)[:int(rng.integers(2, 4))]
    longest = int(rng.choice([3, 8, 40]))
    pats = sorted({rng.choice(letters, size=int(rng.integers(1, longest + 1))).tobytes() for _ in range(int(rng.integers(1, 41)))})
    n = int(rng.choice([1, 2, 17, 300, 5000, 20000])) if seed % 3 == 0 else int(rng.integers(1, 20001))
    return pats, rng.choice(letters, size=n).astype(np.uint8)


RANDOM_SEEDS = list(range(30))
