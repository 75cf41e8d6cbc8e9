"""tools/locate_sweep.py -- what a locate call (PFACX_locatePairsFromDevice) costs (GPU box only), default class, flags 0, over the text workload
(C3's stream) and the pairs of the C3 set over it, in two modes:

    sparse   the C3 pairs as the compacted call returns them: a few pairs per MiB
    dense    the same list with every position of a prefix of the stream (--prefix MiB) in place of that prefix's pairs: every tile of the prefix
             holds 16 384 pairs

next to what a caller can do without the call, measured in the same process over the same bytes and list: PFACX_splitFromDevice followed by
torch.searchsorted over its offsets (and the subtraction that makes columns), and PFACX_splitFromDevice alone.  The calls are synchronous; each is
timed alone with HIP events around it; the median of --steps calls after --warmup calls.  Each mode runs in a child process of its own under a
time limit; the first that fails ends the sweep.  One JSON line per mode on stdout; with --out the lines go to that file
(profiles/locate_sweep.txt).

    python tools/locate_sweep.py [--size 1024] [--prefix 16] [--steps 11] [--warmup 2] [--out profiles/locate_sweep.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(mode, size_mib, prefix_mib, steps, warmup):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pfac_amd import api, hiprt
    from pfac_amd import workloads as wl

    n = size_mib << 20
    cfg = wl.make_config("c3")
    data = np.ascontiguousarray(cfg.input_slice(n, 0))
    h = api.PFAC.create()
    h.setPerfMode(cfg.perf_mode)
    h.readPatternFromFile(wl.write_pattern_file(os.path.join(tempfile.mkdtemp(), "c3.pat"), list(cfg.patterns)))
    d_in = torch.from_numpy(data).to("cuda:0")
    d_ids = torch.empty(n, dtype=torch.int32, device="cuda:0")
    d_all = torch.empty(n, dtype=torch.int32, device="cuda:0")
    _, found = h.matchFromDeviceReduce(d_in.data_ptr(), n, d_ids.data_ptr(), d_all.data_ptr())
    torch.cuda.synchronize()
    d_pos = d_all[:found].clone()
    del d_ids, d_all
    if mode == "dense":
        prefix = min(prefix_mib << 20, n)
        d_pos = torch.cat([torch.arange(prefix, dtype=torch.int32, device="cuda:0"), d_pos[d_pos >= prefix]]).contiguous()
    pairs = int(d_pos.numel())
    d_pos64 = d_pos.to(torch.int64)                              # the list as torch.searchsorted wants it: not part of the timed path
    d_rec = torch.empty(pairs, dtype=torch.int32, device="cuda:0")
    d_col = torch.empty(pairs, dtype=torch.int32, device="cuda:0")
    _, segments, _ = h.splitFromDevice(d_in.data_ptr(), n, None, 0, None, 0, check=False)
    d_off = torch.empty(segments + 1, dtype=torch.int64, device="cuda:0")
    got = {}

    def locate_call():
        got["records"] = h.locatePairsFromDevice(d_in.data_ptr(), n, None, 0, d_pos.data_ptr(), pairs, d_rec.data_ptr(), d_col.data_ptr())[1]

    def split_call():
        got["segments"] = h.splitFromDevice(d_in.data_ptr(), n, None, 0, d_off.data_ptr(), segments + 1)[1]

    def diy_call():
        split_call()
        rec = torch.searchsorted(d_off, d_pos64, right=True) - 1
        got["diy"] = (rec, d_pos64 - d_off[rec])

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

    ms = {}
    raw = {}
    for name, fn in (("locate", locate_call), ("split", split_call), ("diy", diy_call)):
        ms[name], raw[name] = median_ms(fn)
    same = bool(torch.equal(got["diy"][0].to(torch.int32), d_rec) and torch.equal(got["diy"][1].to(torch.int32), d_col))
    h.destroy()
    print(json.dumps({
        "mode": mode, "bytes": n, "pairs": pairs, "records": got["records"], "diy_equal": same,
        "locate_ms": round(ms["locate"], 4), "split_ms": round(ms["split"], 4), "split_searchsorted_ms": round(ms["diy"], 4),
        "locate_over_split": round(ms["locate"] / ms["split"], 3), "split_searchsorted_over_locate": round(ms["diy"] / ms["locate"], 3),
        "locate_input_GBps": round(n / ms["locate"] / 1e6, 2), "calls_ms": raw}), flush=True)
    return 0 if same and got["records"] == got["segments"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="sparse,dense")
    ap.add_argument("--size", type=int, default=1024, help="MiB of the stream")
    ap.add_argument("--prefix", type=int, default=16, help="MiB of the every-position prefix of the dense mode")
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per mode")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.size, a.prefix, a.steps, a.warmup)
    lines = []
    rc = 0
    for mode in a.modes.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", mode, "--size", str(a.size), "--prefix", str(a.prefix),
                                "--steps", str(a.steps), "--warmup", str(a.warmup)], cwd=ROOT, timeout=a.timeout, stdout=subprocess.PIPE)
        except subprocess.TimeoutExpired:
            lines.append(json.dumps({"mode": mode, "error": "time limit"}))
            rc = 124
            break
        out = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
        lines.extend(out)
        for ln in out:
            print(ln, flush=True)
        if p.returncode != 0:
            lines.append(json.dumps({"mode": mode, "error": "exit %d" % p.returncode}))
            rc = p.returncode if p.returncode > 0 else 1
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/locate_sweep.py: PFACX_locatePairsFromDevice (default class, flags 0, records and columns) over %d MiB of C3's stream and the\n"
                    "# pairs of the C3 set (sparse), and with every position of the first %d MiB in the list (dense), next to PFACX_splitFromDevice +\n"
                    "# torch.searchsorted + the column subtraction over the same bytes and list, and PFACX_splitFromDevice alone.  One process per mode,\n"
                    "# median of %d event-timed calls after %d warm-ups, one round.\n" % (a.size, a.prefix, a.steps, a.warmup))
            for ln in lines:
                f.write(ln + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
