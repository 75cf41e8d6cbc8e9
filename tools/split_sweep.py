"""tools/split_sweep.py -- what a split call (PFACX_splitFromDevice) costs (GPU box only), default class, flags 0, over the text workload (C3's
stream): the whole call and its count query (capacity 0: no write pass) next to two yardsticks measured in the same process over the same
bytes -- PFACX_linesBitmapProbe, the existing one-read newline pass, and the do-it-yourself path: torch.nonzero(x == 10) plus the additions
that make offsets of it.  The calls are synchronous; each is timed alone with HIP events around it; the median of --steps calls after
warm-up, the better of two interleaved rounds.
Every size runs in a child process of its own under a time limit; the first that fails ends the sweep.  One JSON line per size on stdout;
with --out the lines go to that file (profiles/split_sweep.txt).

    python tools/split_sweep.py [--sizes 64k,1,16,256,1024] [--steps 20] [--out profiles/split_sweep.txt]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def size_of(item):
    return int(item[:-1]) << 10 if item.endswith("k") else int(item) << 20


def one(item, steps):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pfac_amd import api, hiprt
    from pfac_amd import workloads as wl

    n = size_of(item)
    data = wl.make_config("c3").input_slice(n, 0)
    h = api.PFAC.create()                                      # no pattern set: the call needs none
    d_in = torch.from_numpy(np.ascontiguousarray(data)).to("cuda:0")
    st, segments, longest = h.splitFromDevice(d_in.data_ptr(), n, None, 0, None, 0, check=False)
    d_off = torch.empty(segments + 1, dtype=torch.int64, device="cuda:0")
    got = {"segments": segments, "longest": longest}

    def split_call():
        got["split"] = h.splitFromDevice(d_in.data_ptr(), n, None, 0, d_off.data_ptr(), segments + 1)[1]

    def query_call():
        got["query"] = h.splitFromDevice(d_in.data_ptr(), n, None, 0, None, 0, check=False)[1]

    def diy_call():
        ends = torch.nonzero(d_in == 10).flatten() + 1
        if int(ends.numel()) and int(ends[-1]) == n:
            ends = ends[:-1]
        got["diy_offsets"] = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda:0"), ends, torch.full((1,), n, dtype=torch.int64, device="cuda:0")])

    def median_ms(fn):
        for _ in range(3):
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
        return float(np.median(t))

    mod = C.CDLL(api.library_paths()[1])
    mod.PFACX_linesBitmapProbe.restype = C.c_double
    mod.PFACX_linesBitmapProbe.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    runs = {k: [] for k in ("split", "query", "diy", "probe")}
    for _ in range(2):                                          # interleaved rounds: a drift of the clocks hits every call alike
        runs["split"].append(median_ms(split_call))
        runs["probe"].append(mod.PFACX_linesBitmapProbe(h._h, d_in.data_ptr(), n, steps) if n < (1 << 31) else -1.0)
        runs["query"].append(median_ms(query_call))
        runs["diy"].append(median_ms(diy_call))
    same = bool(torch.equal(got["diy_offsets"], d_off))
    h.destroy()
    best = {k: min(v) for k, v in runs.items()}
    gbs = lambda nbytes, ms: round(nbytes / ms / 1e6, 2) if ms > 0 else None  # noqa: E731
    print(json.dumps({
        "size": item, "bytes": n, "segments": got["split"], "longest": longest, "diy_equal": same,
        "split_ms": round(best["split"], 4), "query_ms": round(best["query"], 4), "newline_pass_ms": round(best["probe"], 4), "diy_ms": round(best["diy"], 4),
        "split_over_newline_pass": round(best["split"] / best["probe"], 3) if best["probe"] > 0 else None,
        "diy_over_split": round(best["diy"] / best["split"], 3),
        "split_input_GBps": gbs(n, best["split"]), "split_traffic_GBps": gbs(2 * n + 8 * (got["split"] + 1), best["split"]),
        "newline_pass_input_GBps": gbs(n, best["probe"]),
        "runs_ms": {k: [round(x, 4) for x in v] for k, v in runs.items()}}), flush=True)
    return 0 if same and got["query"] == got["split"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64k,1,16,256,1024", help="MiB, or KiB with a k")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per size")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.steps)
    lines = []
    rc = 0
    for item in a.sizes.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", item, "--steps", str(a.steps)], cwd=ROOT,
                               timeout=a.timeout, stdout=subprocess.PIPE)
        except subprocess.TimeoutExpired:
            lines.append(json.dumps({"size": item, "error": "time limit"}))
            rc = 124
            break
        out = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
        lines.extend(out)
        for ln in out:
            print(ln, flush=True)
        if p.returncode != 0:
            lines.append(json.dumps({"size": item, "error": "exit %d" % p.returncode}))
            rc = p.returncode if p.returncode > 0 else 1
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/split_sweep.py: PFACX_splitFromDevice (default class, flags 0) over C3's stream: the whole call, its count query (no write pass), the\n"
                    "# newline pass of the lines calls alone (PFACX_linesBitmapProbe: one read) and the do-it-yourself path (torch.nonzero(x == 10) + the additions\n"
                    "# that make offsets of it), same bytes, same process.  Median of %d event-timed calls after warm-up, the better of two interleaved rounds.\n"
                    "# split_traffic = two reads of the input plus 8 bytes per offset.\n" % a.steps)
            for ln in lines:
                f.write(ln + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
