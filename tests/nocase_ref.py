"""Caseless pattern sets (PFACX_READ_NOCASE) for tests/test_nocase_host.py and test_nocase_gpu.py: the ASCII fold and the sets.

The definition (include/pfac_ext.h): a set read with the flag is the set read without it from the folded pattern bytes, and every match
call returns what the same call returns on that folded set over the folded input.  So the expected result is always computed from
folded bytes -- by the oracle, or by brute force -- and never by the library under test.  `bytes.lower()` folds ASCII only, like the
library: it is the fold the brute force uses.
"""
import numpy as np

from pfac_amd import workloads as wl

# bytes around the fold range and Latin-1 capitals: none of them may be folded
FOLD_EDGES = bytes([0x40, 0x5B, 0x60, 0x7B]) + bytes(range(0xC0, 0xDF))


def fold(b: bytes) -> bytes:
    return bytes(b).lower()


def fold_array(a):
    a = np.asarray(a, dtype=np.uint8)
    return np.where((a >= 0x41) & (a <= 0x5A), a + 32, a).astype(np.uint8)


def flip_case(p: bytes, rng) -> bytes:
    """each ASCII letter of p upper- or lower-cased at random"""
    out = bytearray(p)
    for i, c in enumerate(out):
        if 0x41 <= c <= 0x5A or 0x61 <= c <= 0x7A:
            out[i] = (c & ~0x20) if rng.integers(0, 2) else (c | 0x20)
    return bytes(out)


def flip_array(a, rng, fraction=0.5):
    """an input stream with a random part of its letters case-flipped (the bytes that are no letters stay)"""
    a = np.array(a, dtype=np.uint8, copy=True)
    letter = ((a >= 0x41) & (a <= 0x5A)) | ((a >= 0x61) & (a <= 0x7A))
    flip = letter & (rng.random(a.size) < fraction)
    a[flip] ^= 0x20
    return a


def pattern_bytes(pats, crlf=False) -> bytes:
    """the pattern-file bytes of a list (duplicate lines allowed)"""
    end = b"\r\n" if crlf else b"\n"
    return b"".join(bytes(p) + end for p in pats)


def write_patterns(path, pats):
    with open(path, "wb") as f:
        f.write(pattern_bytes(pats))
    return path


def mixed_sets(seed=21):
    """{name: (pattern list with random case, input stream with random case)}: an example, a C2-like random set and a C3-like Snort set"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    ex = [flip_case(p, rng) for p in wl.example_patterns()]
    out["example"] = (ex, np.frombuffer(b"abEDedaBg\nABEDEDABG abedg", dtype=np.uint8).copy())
    c2 = [flip_case(p, rng) for p in wl.random_patterns(400)]
    d2 = wl.random_bytes(48 << 10, seed=9).copy()
    for p in c2[:120]:
        at = int(rng.integers(0, d2.size - 40))
        q = flip_case(p, rng)
        d2[at:at + len(q)] = np.frombuffer(q, dtype=np.uint8)
    out["c2"] = (c2, d2)
    c3raw = wl.snort_patterns(1500)
    c3 = [flip_case(p, rng) for p in c3raw]
    d3 = flip_array(wl.http_stream(64 << 10, wl.http_message_pool(c3raw, pool_size=256, embed_fraction=0.3)), rng)
    out["c3"] = (c3, d3)
    return out


def edge_set():
    """patterns and an input over every byte value, with the bytes around the fold range next to letters"""
    rng = np.random.Generator(np.random.PCG64(3))
    pats = [b"@A", b"[z", b"`a", b"{Z", b"a@", b"Z[", b"\xc0A", b"\xc9\xdeb", b"\xe0a", bytes(range(0x3E, 0x5E)), bytes(range(0x5E, 0x7E)),
            b"\x00Q\xff", b"ABC", b"abd", b"aBe", b"\xdeX", b"\xfeX"]
    alphabet = np.frombuffer(FOLD_EDGES + b"AaBbCcDdEeQqXxZz" + bytes([0x00, 0xFF, 0xE0, 0xFE]), dtype=np.uint8)
    data = rng.choice(alphabet, size=20000)
    data[:256] = np.arange(256, dtype=np.uint8)
    data[256:512] = np.arange(256, dtype=np.uint8)[::-1]
    for p in pats:
        for _ in range(20):
            at = int(rng.integers(512, data.size - 64))
            q = flip_case(p, rng)
            data[at:at + len(q)] = np.frombuffer(q, dtype=np.uint8)
    return pats, np.ascontiguousarray(data, dtype=np.uint8)


DUPLICATES = [b"GET", b"get", b"Get /a", b"gEt /A"]
