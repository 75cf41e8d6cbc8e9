"""tools/flows_sweep.py -- what a flows call (PFACX_flowsMatchFromDevice) costs against (a) PFACX_matchBatchFromDeviceReduce over the
same buffer and offsets -- the call that does the same scan and loses the seams -- and (b) one PFACX_streamMatchFromDevice per piece
over the same pieces -- the call it replaces (GPU box only).  C3's set (30 000 Snort-style patterns, hashed) over its HTTP stream;
batches of 16 MiB and 256 MiB cut into pieces of 64 B, 1.5 KiB and 64 KiB, one flow per piece, plus 1 000 pieces of 1500 B; in steady
state: every flow has a full carry.  Every call is synchronous and timed alone with HIP events around it; the median of --steps calls
after 2 warm-ups is reported with the fastest and the slowest.  (b) is timed over at most --stream-pieces pieces of the batch and scaled
to the batch (every piece costs the same call).  With --parent-lib DIR (libpfac.so and libpfac_gfx950.so built from the parent commit)
(a) and (b) run in the parent's build, as the baseline.  Every (shape, mode) runs in a child process of its own under a time limit; the
first that fails ends the sweep.  One JSON line per shape on stdout; with --out the lines go to that file (profiles/flows_sweep.txt).

    python tools/flows_sweep.py [--shapes 16777216:64,16777216:1536,...] [--steps 11] [--parent-lib DIR] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = "1500000:1500,16777216:64,16777216:1536,16777216:65536,268435456:64,268435456:1536,268435456:65536"


def one(mode, n, piece, steps, stream_pieces):
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
    M = int(h.info().maxPatternLen)
    pieces = n // piece
    n = pieces * piece
    data = cfg.input_slice(max(n, 4096), 0)[:n]
    d_in = torch.from_numpy(np.ascontiguousarray(data)).to("cuda:0")
    offsets = (np.arange(pieces + 1, dtype=np.uintp) * piece)
    cap = n + pieces * (M - 1) + M
    d_ids = torch.empty(cap, dtype=torch.int32, device="cuda:0")
    d_pos = torch.empty(cap, dtype=torch.int32, device="cuda:0")
    d_first = torch.empty(pieces + 1, dtype=torch.int32, device="cuda:0")
    pairs = {}
    scale = 1.0

    if mode == "flows":
        fl = h.flowsOpen(pieces)
        flows = np.arange(pieces, dtype=np.uint32)
        offs = np.zeros(pieces, np.uint64)

        def call():
            pairs["n"] = fl.match_device(d_in.data_ptr(), n, offsets.ctypes.data, flows.ctypes.data, pieces, d_ids.data_ptr(), d_pos.data_ptr(), cap,
                                         d_first.data_ptr(), offs.ctypes.data)[1]
    elif mode == "batch":
        d_off = torch.from_numpy(offsets.astype(np.int64)).to("cuda:0")

        def call():
            pairs["n"] = h.matchBatchFromDeviceReduce(d_in.data_ptr(), n, d_off.data_ptr(), pieces, d_ids.data_ptr(), d_pos.data_ptr(), d_first.data_ptr())[1]
    else:
        fed = min(pieces, stream_pieces)
        scale = pieces / fed
        streams = [h.streamOpen() for _ in range(fed)]

        def call():
            total = 0
            for k in range(fed):
                total += streams[k].match_device(d_in.data_ptr() + k * piece, piece, d_ids.data_ptr(), d_pos.data_ptr(), cap)[1]
            pairs["n"] = total

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
        wall.append((time.perf_counter() - t0) * 1e6 * scale)
        ev.append(a.elapsed_ms(b) * 1e3 * scale)
    h.destroy()
    ev = np.array(ev)
    print(json.dumps({"mode": mode, "bytes": n, "piece": piece, "pieces": pieces, "maxPatternLen": M, "pairs": pairs["n"], "scaled_by": round(scale, 3),
                      "event_us": round(float(np.median(ev)), 2), "event_us_min": round(float(ev.min()), 2), "event_us_max": round(float(ev.max()), 2),
                      "wall_us": round(float(np.median(wall)), 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="bytes:piece, comma separated")
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--stream-pieces", type=int, default=2000, help="pieces the per-piece stream calls are timed over (scaled to the batch)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--parent-lib", default="", help="directory with the parent commit's libpfac.so and libpfac_gfx950.so")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        mode, n, piece = a.one.split(":")
        one(mode, int(n), int(piece), a.steps, a.stream_pieces)
        return 0
    lines = []
    rc = 0
    for shape in a.shapes.split(","):
        row = {"shape": shape}
        for mode in ("flows", "batch", "stream"):
            env = dict(os.environ)
            if a.parent_lib and mode != "flows":
                env["PFAC_HOST_LIB"] = os.path.join(os.path.abspath(a.parent_lib), "libpfac.so")
                env["PFAC_AB_OLD_LIBS"] = "1"
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", f"{mode}:{shape}", "--steps", str(a.steps),
                                    "--stream-pieces", str(a.stream_pieces)], cwd=ROOT, env=env, timeout=a.timeout, stdout=subprocess.PIPE)
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
            row[mode + "_pairs"] = r["pairs"]
            row["pieces"] = r["pieces"]
            row["maxPatternLen"] = r["maxPatternLen"]
            if mode == "stream":
                row["stream_scaled_by"] = r["scaled_by"]
        if "flows_us" in row and "batch_us" in row:
            row["flows_over_batch"] = round(row["flows_us"] / row["batch_us"], 3)
        if "flows_us" in row and "stream_us" in row:
            row["stream_over_flows"] = round(row["stream_us"] / row["flows_us"], 1)
        ln = json.dumps(row)
        lines.append(ln)
        print(ln, flush=True)
        if rc:
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/flows_sweep.py: PFACX_flowsMatchFromDevice per batch against (a) PFACX_matchBatchFromDeviceReduce over the same buffer and\n"
                    "# offsets (batch) and (b) one PFACX_streamMatchFromDevice per piece (stream; timed over a part of the pieces and scaled); C3 set and\n"
                    "# stream, one flow per piece, full carries; microseconds, median of %d event-timed calls after 2 warm-ups, *_us_range = fastest\n"
                    "# and slowest of them, *_wall_us = the host's clock; batch and stream %s\n" % (a.steps, "in the parent commit's build" if a.parent_lib else "in this build"))
            for ln in lines:
                f.write(ln + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
