"""tools/stream_sweep.py -- what a stream call (PFACX_streamMatchFromDevice) costs per piece against the plain compacted call
(PFAC_matchFromDeviceReduce) over the same bytes, and against the do-it-yourself alternative it replaces (GPU box only).
C3's set (30 000 Snort-style patterns, hashed) over its HTTP stream; pieces of 1500 B (one packet per call), 64 KiB, 1 MiB, 16 MiB,
256 MiB and 1 GiB.  Every call is synchronous; each is timed alone with HIP events around it (and by the host's clock), the median
of --steps calls after 2 warm-ups is reported.
  stream   one stream fed the piece again and again (every call: seam launch + the piece in place + the carry)
  plain    PFAC_matchFromDeviceReduce over the piece -- of this build and, with --parent-lib DIR (libpfac.so and libpfac_gfx950.so
           built from the parent commit), of the parent: the baseline the extra per call is measured against
  diy      what a caller does without streams: the last maxPatternLen - 1 bytes of the previous piece and the piece copied into
           one buffer, the plain call over it, the positions downloaded and the pairs of the glued bytes dropped on the host
Every (size, mode) runs in a child process of its own under a time limit; the first that fails ends the sweep.  One JSON line per
size on stdout; with --out the lines go to that file (profiles/stream_sweep.txt).

    python tools/stream_sweep.py [--sizes 1500,65536,1048576,16777216,268435456,1073741824] [--steps 11] [--parent-lib DIR] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(mode, n, steps):
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
    data = cfg.input_slice(max(n, 4096), 0)[:n]
    d_in = torch.from_numpy(np.ascontiguousarray(data)).to("cuda:0")
    cap = n + M
    d_ids = torch.empty(cap, dtype=torch.int32, device="cuda:0")
    d_pos = torch.empty(cap, dtype=torch.int32, device="cuda:0")
    pairs = {}

    if mode == "stream":
        s = h.streamOpen()

        def call():
            pairs["n"] = s.match_device(d_in.data_ptr(), n, d_ids.data_ptr(), d_pos.data_ptr(), cap)[1]
    elif mode == "plain":
        def call():
            pairs["n"] = h.matchFromDeviceReduce(d_in.data_ptr(), n, d_ids.data_ptr(), d_pos.data_ptr())[1]
    else:
        keep = min(M - 1, n)
        d_glue = torch.empty(n + M - 1, dtype=torch.uint8, device="cuda:0")
        d_tail = d_in[n - keep:].clone()

        def call():
            d_glue[:keep] = d_tail
            d_glue[keep:keep + n] = d_in
            k = h.matchFromDeviceReduce(d_glue.data_ptr(), keep + n, d_ids.data_ptr(), d_pos.data_ptr())[1]
            pos = d_pos[:k].cpu().numpy()
            ids = d_ids[:k].cpu().numpy()
            final = pos + M <= keep + n                       # what is not final comes back out of the next call
            pairs["n"] = int(np.count_nonzero(final))
            pairs["ids"] = ids[final]
            d_tail.copy_(d_glue[keep + n - keep:keep + n])

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
    print(json.dumps({"mode": mode, "bytes": n, "maxPatternLen": M, "pairs": pairs["n"], "event_us": round(float(np.median(ev)), 2),
                      "event_us_min": round(float(ev.min()), 2), "event_us_max": round(float(ev.max()), 2),
                      "wall_us": round(float(np.median(wall)), 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1500,65536,1048576,16777216,268435456,1073741824")
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--parent-lib", default="", help="directory with the parent commit's libpfac.so and libpfac_gfx950.so")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        mode, n = a.one.split(":")
        one(mode, int(n), a.steps)
        return 0
    lines = []
    rc = 0
    modes = [("stream", None), ("plain", None), ("diy", None)] + ([("plain", a.parent_lib)] if a.parent_lib else [])
    for size in a.sizes.split(","):
        row = {"bytes": int(size)}
        for mode, lib in modes:
            env = dict(os.environ)
            if lib:
                env["PFAC_HOST_LIB"] = os.path.join(os.path.abspath(lib), "libpfac.so")
                env["PFAC_AB_OLD_LIBS"] = "1"
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", f"{mode}:{size}", "--steps", str(a.steps)], cwd=ROOT, env=env,
                                   timeout=a.timeout, stdout=subprocess.PIPE)
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
            key = "parent_plain" if lib else mode
            row[key + "_us"] = r["event_us"]
            row[key + "_us_range"] = [r["event_us_min"], r["event_us_max"]]
            row[key + "_wall_us"] = r["wall_us"]
            row[key + "_pairs"] = r["pairs"]
            row["maxPatternLen"] = r["maxPatternLen"]
        base = "parent_plain_us" if "parent_plain_us" in row else "plain_us"
        if "stream_us" in row and base in row:
            row["stream_minus_" + base[:-3] + "_us"] = round(row["stream_us"] - row[base], 2)
        ln = json.dumps(row)
        lines.append(ln)
        print(ln, flush=True)
        if rc:
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/stream_sweep.py: PFACX_streamMatchFromDevice per piece against PFAC_matchFromDeviceReduce over the same bytes (this build:\n"
                    "# plain; the parent commit's build: parent_plain) and against the do-it-yourself glue (diy); C3 set and stream; microseconds,\n"
                    "# median of %d event-timed calls after 2 warm-ups, *_us_range = fastest and slowest of them, *_wall_us = the host's clock\n" % a.steps)
            for ln in lines:
                f.write(ln + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
