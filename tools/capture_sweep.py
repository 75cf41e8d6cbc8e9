"""tools/capture_sweep.py -- what a capture call (PFACX_capturePairsFromDevice) costs (GPU box only) over --size MiB of log-like text made from a
seed on the device: lower-case letters in lines of 128 bytes, a key `k=` and a blank at every `period` bytes, its value of about `value` bytes behind
it, a '\\n' behind the value.  Shapes:

    rare-16                  a key per MiB, values of 16 bytes: one tile in 64 holds a pair
    sparse-16, sparse-200    a key per 4 KiB -- four in every tile --, values of 16 and of 200 bytes
    dense-16, dense-200      a key per 64 bytes; values of 16 bytes, and of about 200 (a '\\n' every 400 bytes: a value runs over the keys behind it)
    hostile                  the sparse-200 text with every position of its first --prefix MiB in the list

each with window 0 and 256, S = {' '}, D = {'\\n'}, the list (id 1, the key's position) built on the device, not scanned for.  Per shape and window
one JSON line: the time of the pairs form alone, pairs/s, and the share of the pairs that took the slow path (PFACX_captureRun's *h_slowPairs, asked
of the module entry over the same list).  For comparison on the same buffers, once per shape: (a) what a caller has today where it can say the same
thing -- S empty, no window: PFACX_splitFromDevice + torch.searchsorted + the look at the record's last byte -- next to the call with S empty and no
window, results compared; (b) PFACX_locatePairsFromDevice over the same list, the yardstick of a tiled pass over a pair list.  The calls are
synchronous; each is timed alone with HIP events around it behind --warmup settle calls, the median of --steps.  Each shape runs in a child process
of its own under a time limit; the first that fails ends the sweep.  With --out the lines go to that file (profiles/capture_sweep.txt).

    python tools/capture_sweep.py [--size 1024] [--prefix 64] [--steps 11] [--warmup 2] [--out profiles/capture_sweep.txt]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"rare-16": (1 << 20, 16), "sparse-16": (4096, 16), "sparse-200": (4096, 200), "dense-16": (64, 16), "dense-200": (64, 200), "hostile": (4096, 200)}


class CaptureRun(C.Structure):              # include/pfac_module.h: PFACX_captureRun_t
    _fields_ = [("d_input", C.c_void_p), ("size", C.c_size_t), ("skip", C.c_uint * 8), ("stop", C.c_uint * 8), ("window", C.c_size_t),
                ("flags", C.c_uint), ("d_ids", C.c_void_p), ("d_pos", C.c_void_p), ("numPairs", C.c_size_t), ("d_patternLen", C.c_void_p),
                ("numLens", C.c_size_t), ("d_valStart", C.c_void_p), ("d_valLen", C.c_void_p)]


def one(shape, size_mib, prefix_mib, steps, warmup):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pfac_amd import api, hiprt

    n = size_mib << 20
    period, value = SHAPES[shape]
    dev = "cuda:0"
    gen = torch.Generator(device=dev)
    gen.manual_seed(20)
    d_in = torch.randint(97, 123, (n,), dtype=torch.uint8, device=dev, generator=gen)
    at = torch.arange(n, dtype=torch.int64, device=dev)
    off = at % period
    if period >= value + 4:                                      # the value's '\n', lines of 128 bytes behind it
        d_in[(off == 3 + value) | ((off > 3 + value) & (off % 128 == 127))] = 10
    else:
        d_in[at % (2 * value) == 2 * value - 1] = 10             # values of `value` bytes on average
    for k, byte in enumerate(b"k= "):
        d_in[off == k] = byte
    del off
    keys = at[::period].to(torch.int32)
    if shape == "hostile":
        prefix = min(prefix_mib << 20, n)
        keys = torch.cat([torch.arange(prefix, dtype=torch.int32, device=dev), keys[keys >= prefix]])
    del at
    d_pos = keys.contiguous()
    pairs = int(d_pos.numel())
    d_ids = torch.ones(pairs, dtype=torch.int32, device=dev)
    d_start = torch.empty(pairs, dtype=torch.int32, device=dev)
    d_len = torch.empty(pairs, dtype=torch.int32, device=dev)
    d_rec = torch.empty(pairs, dtype=torch.int32, device=dev)
    h = api.PFAC.create()
    h.readPatternFromMemory(b"k=\n")
    module = C.CDLL(api.library_paths()[1])
    module.PFACX_captureRun.argtypes = [C.c_void_p, C.POINTER(CaptureRun), C.POINTER(C.c_size_t)]
    d_lens = torch.tensor([0, 2], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def capture_call(skip, window):
        h.capturePairsFromDevice(d_in.data_ptr(), n, skip, None, window, 0, d_ids.data_ptr(), d_pos.data_ptr(), pairs, d_start.data_ptr(), d_len.data_ptr())

    def slow_pairs(skip, window):
        run = CaptureRun(d_in.data_ptr(), n, api.word_class(skip), api.word_class(b"\n"), window, 0, d_ids.data_ptr(), d_pos.data_ptr(), pairs,
                         d_lens.data_ptr(), 2, d_start.data_ptr(), d_len.data_ptr())
        slow = C.c_size_t(0)
        st = module.PFACX_captureRun(h._h, C.byref(run), C.byref(slow))
        assert st == 0, st
        return slow.value

    def median_ms(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(steps):
            a, b = hiprt.Event(), hiprt.Event()
            a.record(0)
            fn()
            b.record(0)
            torch.cuda.synchronize()
            t.append(a.elapsed_ms(b))
        return float(np.median(t)), [round(x, 4) for x in t]

    # the comparisons, once per shape
    _, segments, _ = h.splitFromDevice(d_in.data_ptr(), n, None, 0, None, 0, check=False)
    d_off = torch.empty(segments + 1, dtype=torch.int64, device=dev)
    d_b = (d_pos.to(torch.int64) + 2).clamp(max=n)                # the list as torch.searchsorted wants it: not part of the timed path
    got = {}

    def diy_call():
        h.splitFromDevice(d_in.data_ptr(), n, None, 0, d_off.data_ptr(), segments + 1)
        last = d_off[torch.searchsorted(d_off, d_b.clamp(max=n - 1), right=True)] - 1
        got["end"] = torch.where(d_in[last] == 10, last, torch.full_like(last, n))

    def locate_call():
        h.locatePairsFromDevice(d_in.data_ptr(), n, None, 0, d_pos.data_ptr(), pairs, d_rec.data_ptr(), None, want_records=False)

    noskip_ms, _ = median_ms(lambda: capture_call(None, 0))
    ends = d_start.to(torch.int64) + d_len
    diy_ms, _ = median_ms(diy_call)
    same = bool(torch.equal(torch.where(d_b < n, got["end"], torch.full_like(d_b, n)), ends))
    locate_ms, _ = median_ms(locate_call)
    del d_off, got, ends
    rc = 0 if same else 1
    for window in (0, 256):
        ms, raw = median_ms(lambda: capture_call(b" ", window))
        slow = slow_pairs(b" ", window)
        print(json.dumps({
            "shape": shape, "bytes": n, "pairs": pairs, "window": window, "capture_ms": round(ms, 4), "pairs_per_s": round(pairs / ms * 1e3),
            "slow_pairs": slow, "slow_share": round(slow / pairs, 6), "mean_value": round(float(d_len.to(torch.float64).mean()), 1),
            "capture_noskip_nowindow_ms": round(noskip_ms, 4), "split_searchsorted_ms": round(diy_ms, 4), "diy_equal": same,
            "split_searchsorted_over_capture": round(diy_ms / noskip_ms, 2), "locate_ms": round(locate_ms, 4),
            "capture_over_locate": round(ms / locate_ms, 3), "calls_ms": raw}), flush=True)
    h.destroy()
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--size", type=int, default=1024, help="MiB of text")
    ap.add_argument("--prefix", type=int, default=64, help="MiB of the every-position prefix of the hostile shape")
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per shape")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.size, a.prefix, a.steps, a.warmup)
    lines = []
    rc = 0
    for shape in a.shapes.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", shape, "--size", str(a.size), "--prefix", str(a.prefix),
                                "--steps", str(a.steps), "--warmup", str(a.warmup)], cwd=ROOT, timeout=a.timeout, stdout=subprocess.PIPE)
        except subprocess.TimeoutExpired:
            lines.append(json.dumps({"shape": shape, "error": "time limit"}))
            rc = 124
            break
        out = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
        lines.extend(out)
        for ln in out:
            print(ln, flush=True)
        if p.returncode != 0:
            lines.append(json.dumps({"shape": shape, "error": "exit %d" % p.returncode}))
            rc = p.returncode if p.returncode > 0 else 1
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/capture_sweep.py: PFACX_capturePairsFromDevice (S = {' '}, D = {'\\n'}) over %d MiB of seeded log-like text, a key per MiB (rare), per 4 KiB (sparse) or\n"
                    "# per 64 bytes (dense), values of about 16 and 200 bytes, and with every position of the first %d MiB in the list (hostile); window 0 and\n"
                    "# 256.  slow_share: the pairs that left the bitmaps of their tile.  Next to it, S empty and no window on both sides: PFACX_splitFromDevice\n"
                    "# + torch.searchsorted + the look at the record's last byte; and PFACX_locatePairsFromDevice over the same list.  One process per shape,\n"
                    "# median of %d event-timed calls after %d warm-ups, one round.\n" % (a.size, a.prefix, a.steps, a.warmup))
            for ln in lines:
                f.write(ln + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
