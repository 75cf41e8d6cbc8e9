"""tools/batch_sweep.py -- what a batch call (PFACX_matchBatchFromDevice) costs against the plain call over the same bytes and against
a loop of one call per segment (GPU box only).  C3's set (30 000 Snort-style patterns, hashed) over its HTTP stream, 16 MiB and 256 MiB,
segments of 64 B, 1.5 KiB and 64 KiB.  Every (size) step runs in a child process of its own under a time limit; the first step that
fails ends the sweep.  One JSON line per measurement on stdout.

    python tools/batch_sweep.py [--sizes-mib 16,256] [--timeout 600]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEGMENTS = (64, 1536, 64 << 10)
LOOP_SEGMENTS = 1000


def one(size_mib, steps):
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
    n = size_mib << 20
    d_in = torch.from_numpy(cfg.input_slice(n, 0).copy()).to("cuda:0")
    d_out = torch.empty(n, dtype=torch.int32, device="cuda:0")

    def ms_per(fn, reps):
        fn()
        torch.cuda.synchronize()
        a, b = hiprt.Event(), hiprt.Event()
        a.record(0)
        for _ in range(reps):
            fn()
        b.record(0)
        torch.cuda.synchronize()
        return a.elapsed_ms(b) / reps

    plain = ms_per(lambda: h.matchFromDevice(d_in.data_ptr(), n, d_out.data_ptr()), steps)
    plain_out = d_out.cpu().numpy()
    print(json.dumps({"size_mib": size_mib, "what": "plain", "ms": round(plain, 4), "gbps": round(n / plain / 1e6, 1)}), flush=True)
    for seg in SEGMENTS:
        offs = np.arange(0, n + 1, seg, dtype=np.int64)
        if offs[-1] != n:
            offs = np.append(offs, n)
        d_off = torch.from_numpy(offs).to("cuda:0")
        nseg = offs.size - 1
        batch = ms_per(lambda: h.matchBatchFromDevice(d_in.data_ptr(), n, d_off.data_ptr(), nseg, d_out.data_ptr()), steps)
        got = d_out.cpu().numpy()
        changed = int(np.count_nonzero(got != plain_out))          # positions the segment ends changed
        print(json.dumps({"size_mib": size_mib, "what": "batch", "segment_bytes": seg, "segments": nseg, "ms": round(batch, 4),
                          "gbps": round(n / batch / 1e6, 1), "vs_plain": round(plain / batch, 3), "positions_changed_by_ends": changed}), flush=True)
        loop_n = min(LOOP_SEGMENTS, nseg)
        loop_bytes = int(offs[loop_n])

        def per_segment_loop():
            for k in range(loop_n):
                s = int(offs[k])
                h.matchFromDevice(d_in.data_ptr() + s, int(offs[k + 1]) - s, d_out.data_ptr() + 4 * s)
        loop = ms_per(per_segment_loop, 3)
        loop_rate = loop_bytes / loop / 1e6
        print(json.dumps({"size_mib": size_mib, "what": "per_segment_loop", "segment_bytes": seg, "segments": loop_n, "ms": round(loop, 4),
                          "gbps": round(loop_rate, 2), "batch_vs_loop": round(n / batch / 1e6 / loop_rate, 1)}), flush=True)
    h.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes-mib", default="16,256")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per size step")
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a.one, a.steps)
        return 0
    for mib in [int(x) for x in a.sizes_mib.split(",")]:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(mib), "--steps", str(a.steps)], cwd=ROOT, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(json.dumps({"size_mib": mib, "error": "time limit"}), flush=True)
            return 124
        if p.returncode != 0:
            print(json.dumps({"size_mib": mib, "error": "exit %d" % p.returncode}), flush=True)
            return p.returncode if p.returncode > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
