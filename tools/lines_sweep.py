"""tools/lines_sweep.py -- what a lines call (PFACX_matchLinesFromDevice) costs (GPU box only): against the compacted call
(PFAC_matchFromDeviceReduce) over the same bytes, the floor it cannot go below; against the do-it-yourself path (newline offsets from
torch.nonzero on the device, PFACX_matchBatchFromDeviceReduce, a d_segFirst difference); the newline pass alone in bytes per second; and
the gather (PFACX_gatherLinesFromDevice) of the matching lines and of the lines that do not match (INVERT), as bytes read plus bytes
written per second.  C3's set over its stream.  All calls are synchronous; each is timed alone with HIP events around it; the median of
--steps calls after warm-up, the better of two interleaved rounds.
Every size runs in a child process of its own under a time limit; the first that fails ends the sweep.  One JSON line per size on
stdout; with --out the lines go to that file (profiles/lines_sweep.txt).

    python tools/lines_sweep.py [--sizes 64k,1,16,256,1024] [--steps 20] [--out profiles/lines_sweep.txt]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

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
    cfg = wl.make_config("c3")
    data = cfg.input_slice(n, 0)
    pf = wl.write_pattern_file(os.path.join(tempfile.mkdtemp(), "c3.pat"), list(cfg.patterns))
    h = api.PFAC.create()
    h.setPerfMode(cfg.perf_mode)
    h.readPatternFromFile(pf)
    d_in = torch.from_numpy(np.ascontiguousarray(data)).to("cuda:0")
    d_a = torch.empty(n, dtype=torch.int32, device="cuda:0")
    d_b = torch.empty(n, dtype=torch.int32, device="cuda:0")
    d_seg = torch.empty(n + 2, dtype=torch.int32, device="cuda:0")
    d_out = torch.empty(n + 1, dtype=torch.uint8, device="cuda:0")
    got = {}

    def reduce_call():
        got["pairs"] = h.matchFromDeviceReduce(d_in.data_ptr(), n, d_a.data_ptr(), d_b.data_ptr())[1]

    def lines_call(flags=0):
        _, got["lines"], got["selected" if not flags else "selected_invert"] = h.matchLinesFromDevice(
            d_in.data_ptr(), n, flags, d_a.data_ptr(), d_b.data_ptr(), None, n)

    def diy_call():
        ends = torch.nonzero(d_in == 10).flatten() + 1
        offs = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda:0"), ends, torch.full((1,), n, dtype=torch.int64, device="cuda:0")])
        segs = int(offs.numel()) - 1
        h.matchBatchFromDeviceReduce(d_in.data_ptr(), n, offs.data_ptr(), segs, d_a.data_ptr(), d_b.data_ptr(), d_seg.data_ptr())
        first = d_seg[:segs + 1]
        got["diy_selected"] = int(torch.count_nonzero(first[1:] - first[:-1]))

    def gather_call(key):
        got["gather_bytes_" + key] = h.gatherLinesFromDevice(d_in.data_ptr(), n, d_a.data_ptr(), d_b.data_ptr(), got[key], d_out.data_ptr(), n + 1)[1]

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

    # interleaved rounds: a drift of the clocks hits every call alike
    runs = {k: [] for k in ("reduce", "lines", "lines_invert", "diy", "gather", "gather_invert")}
    for _ in range(2):
        runs["reduce"].append(median_ms(reduce_call))
        runs["lines"].append(median_ms(lines_call))
        runs["gather"].append(median_ms(lambda: gather_call("selected")))           # the list the call in front of it left
        runs["lines_invert"].append(median_ms(lambda: lines_call(api.PFACX_LINES_INVERT)))
        runs["gather_invert"].append(median_ms(lambda: gather_call("selected_invert")))
        runs["diy"].append(median_ms(diy_call))
    best = {k: min(v) for k, v in runs.items()}
    mod = C.CDLL(api.library_paths()[1])
    mod.PFACX_linesBitmapProbe.restype = C.c_double
    mod.PFACX_linesBitmapProbe.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    probe = min(mod.PFACX_linesBitmapProbe(h._h, d_in.data_ptr(), n, steps) for _ in range(2))
    h.destroy()
    gbs = lambda nbytes, ms: round(nbytes / ms / 1e6, 2) if ms > 0 else None  # noqa: E731
    print(json.dumps({
        "size": item, "bytes": n, "lines": got["lines"], "pairs": got["pairs"], "selected": got["selected"], "selected_invert": got["selected_invert"],
        "diy_selected": got["diy_selected"],
        "reduce_ms": round(best["reduce"], 4), "lines_ms": round(best["lines"], 4), "lines_invert_ms": round(best["lines_invert"], 4),
        "diy_ms": round(best["diy"], 4), "lines_over_reduce": round(best["lines"] / best["reduce"], 4), "diy_over_lines": round(best["diy"] / best["lines"], 4),
        "newline_pass_ms": round(probe, 4), "newline_pass_input_GBps": gbs(n, probe), "newline_pass_traffic_GBps": gbs(n + n * 5 // 16, probe),
        "gather_ms": round(best["gather"], 4), "gather_bytes": got["gather_bytes_selected"], "gather_rw_GBps": gbs(2 * got["gather_bytes_selected"], best["gather"]),
        "gather_invert_ms": round(best["gather_invert"], 4), "gather_invert_bytes": got["gather_bytes_selected_invert"],
        "gather_invert_rw_GBps": gbs(2 * got["gather_bytes_selected_invert"], best["gather_invert"]),
        "runs_ms": {k: [round(x, 4) for x in v] for k, v in runs.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64k,1,16,256,1024", help="MiB, or KiB with a k")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per size")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a.one, a.steps)
        return 0
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
            f.write("# tools/lines_sweep.py: PFACX_matchLinesFromDevice against PFAC_matchFromDeviceReduce (the same build: this change does not touch that path) and\n"
                    "# against the do-it-yourself path (torch.nonzero + PFACX_matchBatchFromDeviceReduce + a d_segFirst difference), C3 set and stream, same bytes, same\n"
                    "# handle; the newline pass alone; the gather of the matching lines and of the others (INVERT).  Median of %d event-timed calls after warm-up, the\n"
                    "# better of two interleaved rounds.  newline_pass_traffic = the input plus the 5/16 byte per input byte the pass writes; gather_rw = 2 x the text.\n" % a.steps)
            for ln in lines:
                f.write(ln + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
