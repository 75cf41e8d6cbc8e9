"""tools/countbatch_sweep.py -- what a batch count call (PFACX_countBatchFromDevice) costs against (a) PFACX_matchBatchFromDeviceReduce over the
same bytes and offsets -- the scan the call contains -- and (b) the do-it-yourself path: PFACX_matchAllBatchFromDevice, then torch.unique over
segment * (F + 1) + id keys with counts (GPU box only).  C3's set (30 000 Snort-style patterns, hashed) over its HTTP stream; buffers of 16 MiB and
256 MiB cut into segments of 64 B, 1.5 KiB and 64 KiB.  Every call is synchronous and timed alone with HIP events around it; the median of --steps
calls after 2 warm-ups is reported with the fastest and the slowest.  With --parent-lib DIR (libpfac.so and libpfac_gfx950.so built from the parent
commit) (a) and the call inside (b) run in the parent's build, as the baseline.  Every (shape, mode) runs in a child process of its own under a time
limit; the first that fails ends the sweep.  One JSON line per shape on stdout; with --out the lines go to that file (profiles/countbatch_sweep.txt).
The torch path of (b) allocates its index and row-pointer tensors in every timed call, as a caller's would; its calls lie up to 30 % apart,
so one round does not settle a ratio near 1.  `count` is the all-occurrence list, `longest` the call with PFACX_COUNT_LONGEST (no chain walk, the table never read).

    python tools/countbatch_sweep.py [--shapes 16777216:1536,...] [--steps 11] [--parent-lib DIR] [--modes count,reduce,...] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = "16777216:64,16777216:1536,16777216:65536,268435456:64,268435456:1536,268435456:65536"


def one(mode, n, seg, steps):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pfac_amd import api, hiprt
    from pfac_amd import workloads as wl

    cfg = wl.make_config("c3")
    pf = wl.write_pattern_file(os.path.join(tempfile.mkdtemp(), "c3.pat"), cfg.patterns)
    h = api.PFAC.create()
    h.setPerfMode(cfg.perf_mode)
    h.readPatternFromFile(pf)
    info = h.info()
    F = int(info.numOfPatterns)
    segs = n // seg
    n = segs * seg
    data = cfg.input_slice(max(n, 4096), 0)[:n]
    d_in = torch.from_numpy(np.ascontiguousarray(data)).to("cuda:0")
    d_off = torch.from_numpy((np.arange(segs + 1, dtype=np.int64) * seg)).to("cuda:0")
    result = {}

    if mode in ("count", "longest"):
        flags = api.PFACX_COUNT_LONGEST if mode == "longest" else 0
        d_first = torch.empty(segs + 1, dtype=torch.int64, device="cuda:0")
        _, entries, _ = h.countBatchFromDevice(d_in.data_ptr(), n, d_off.data_ptr(), segs, flags, None, None, 0, d_first.data_ptr(), check=False)
        d_ids = torch.empty(max(1, entries), dtype=torch.int32, device="cuda:0")
        d_counts = torch.empty(max(1, entries), dtype=torch.int32, device="cuda:0")

        def call():
            _, result["entries"], result["occurrences"] = h.countBatchFromDevice(d_in.data_ptr(), n, d_off.data_ptr(), segs, flags, d_ids.data_ptr(),
                                                                                 d_counts.data_ptr(), entries, d_first.data_ptr())
    elif mode == "reduce":
        d_ids = torch.empty(n, dtype=torch.int32, device="cuda:0")
        d_pos = torch.empty(n, dtype=torch.int32, device="cuda:0")
        d_first = torch.empty(segs + 1, dtype=torch.int32, device="cuda:0")

        def call():
            result["pairs"] = h.matchBatchFromDeviceReduce(d_in.data_ptr(), n, d_off.data_ptr(), segs, d_ids.data_ptr(), d_pos.data_ptr(), d_first.data_ptr())[1]
    else:
        cap = n * max(1, int(info.maxMatchesPerPosition))
        d_ids = torch.empty(cap, dtype=torch.int32, device="cuda:0")
        d_pos = torch.empty(cap, dtype=torch.int32, device="cuda:0")
        d_first = torch.empty(segs + 1, dtype=torch.int64, device="cuda:0")

        def call():
            p = h.matchAllBatchFromDevice(d_in.data_ptr(), n, d_off.data_ptr(), segs, d_ids.data_ptr(), d_pos.data_ptr(), cap, d_first.data_ptr())[1]
            seg_of = torch.searchsorted(d_first[1:], torch.arange(p, device="cuda:0"), right=True)
            keys, counts = torch.unique(seg_of * (F + 1) + d_ids[:p].long(), return_counts=True)
            row = torch.zeros(segs + 1, dtype=torch.int64, device="cuda:0")
            row[1:] = torch.cumsum(torch.bincount(keys // (F + 1), minlength=segs), 0)          # the row pointer the call returns
            result["occurrences"] = p
            result["entries"] = int(keys.numel())

    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(steps):
        a, b = hiprt.Event(), hiprt.Event()
        t0 = time.perf_counter()
        a.record(0)
        call()
        b.record(0)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6)
        ev.append(a.elapsed_ms(b) * 1e3)
    h.destroy()
    ev = np.array(ev)
    print(json.dumps({"mode": mode, "bytes": n, "segment": seg, "segments": segs, **result,
                      "event_us": round(float(np.median(ev)), 2), "event_us_min": round(float(ev.min()), 2), "event_us_max": round(float(ev.max()), 2),
                      "wall_us": round(float(np.median(wall)), 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="bytes:segment, comma separated")
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--parent-lib", default="", help="directory with the parent commit's libpfac.so and libpfac_gfx950.so")
    ap.add_argument("--modes", default="count,longest,reduce,diy", help="comma separated")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        mode, n, seg = a.one.split(":")
        one(mode, int(n), int(seg), a.steps)
        return 0
    lines = []
    rc = 0
    for shape in a.shapes.split(","):
        row = {"shape": shape}
        for mode in a.modes.split(","):
            env = dict(os.environ)
            if a.parent_lib and mode in ("reduce", "diy"):
                env["PFAC_HOST_LIB"] = os.path.join(os.path.abspath(a.parent_lib), "libpfac.so")
                env["PFAC_AB_OLD_LIBS"] = "1"
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", f"{mode}:{shape}", "--steps", str(a.steps)],
                                   cwd=ROOT, env=env, timeout=a.timeout, stdout=subprocess.PIPE)
            except subprocess.TimeoutExpired:
                row["error"] = f"{mode}: time limit"
                rc = 124
                break
            out = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not out:
                row["error"] = f"{mode}: exit {p.returncode}"
                rc = p.returncode if p.returncode > 0 else 1
                break
            r = json.loads(out[-1])
            row[mode + "_us"] = r["event_us"]
            row[mode + "_us_range"] = [r["event_us_min"], r["event_us_max"]]
            row[mode + "_wall_us"] = r["wall_us"]
            row["segments"] = r["segments"]
            for k in ("entries", "occurrences", "pairs"):
                if k in r:
                    row[mode + "_" + k] = r[k]
        for mode in ("count", "longest"):
            if mode + "_us" in row and "reduce_us" in row:
                row[mode + "_over_reduce"] = round(row[mode + "_us"] / row["reduce_us"], 3)
                row[mode + "_extra_us"] = round(row[mode + "_us"] - row["reduce_us"], 2)
        if "count_us" in row and "diy_us" in row:
            row["diy_over_count"] = round(row["diy_us"] / row["count_us"], 2)
        ln = json.dumps(row)
        lines.append(ln)
        print(ln, flush=True)
        if rc:
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/countbatch_sweep.py: PFACX_countBatchFromDevice per batch (count; longest: with PFACX_COUNT_LONGEST) against (a)\n"
                    "# PFACX_matchBatchFromDeviceReduce over the same bytes and offsets (reduce: the scan the call contains) and (b) PFACX_matchAllBatchFromDevice\n"
                    "# plus torch.unique over segment * (F + 1) + id keys with counts (diy); C3 set and stream; microseconds, median of %d event-timed calls\n"
                    "# after 2 warm-ups, *_us_range = fastest and slowest of them, *_wall_us = the host's clock; reduce and diy %s\n"
                    % (a.steps, "in the parent commit's build" if a.parent_lib else "in this build"))
            for ln in lines:
                f.write(ln + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
