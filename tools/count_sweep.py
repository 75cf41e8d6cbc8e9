"""tools/count_sweep.py -- what the count calls cost (GPU box only).  (a) PFACX_countFromDevice, all occurrences and PFACX_COUNT_LONGEST, against
the ordered compacted call (PFAC_matchFromDeviceReduce) over the same bytes: C3's set over its stream; (b) the passes behind the scan alone --
PFACX_countPairsFromDevice over the id list the compacted call left, asynchronous, event-timed: with PFACX_COUNT_LONGEST the memset, pfac_count_hist
and pfac_count_store (reported as pairs per second), without it pfac_count_chain on top (the difference is its figure); (c) the same on the
all-matching input (pattern "a" over a run of "a": pairs == size, ONE id), on the nested input (a, aa, ..., a x 8 over runs of a) and on a
synthetic id list spread evenly over the 100 000 ids of the S100 set (no scan: the histogram's tagged cache alone); (d) the do-it-yourself path:
PFACX_matchAllFromDevice with capacity = size x maxMatchesPerPosition, then torch.bincount.  All calls are timed alone with HIP events around them;
the median of --steps calls after warm-up, the better of two interleaved rounds.
Every item runs in a child process of its own under a time limit; the first that fails ends the sweep.  One JSON line per item on stdout; with
--out the lines go to that file (profiles/count_sweep.txt).

    python tools/count_sweep.py [--sizes 64k,16,256,1024] [--others covered:256,nested:32,spread:64] [--steps 20] [--out profiles/count_sweep.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def size_of(item):
    item = item.split(":")[-1]
    return int(item[:-1]) << 10 if item.endswith("k") else int(item) << 20


def one(item, steps):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pfac_amd import api, hiprt
    from pfac_amd import workloads as wl

    n = size_of(item)
    kind = item.split(":")[0] if ":" in item else "c3"
    tmp = tempfile.mkdtemp()
    h = api.PFAC.create()
    if kind == "c3":
        cfg = wl.make_config("c3")
        data = np.ascontiguousarray(cfg.input_slice(n, 0))
        pats = list(cfg.patterns)
        h.setPerfMode(cfg.perf_mode)
    elif kind == "covered":                 # pairs == size, one id
        data = np.full(n, ord("a"), dtype=np.uint8)
        pats = [b"a"]
    elif kind == "nested":                  # runs of 0 .. 40 a, one or two b between them: chains of depth 8
        rng = np.random.Generator(np.random.PCG64(8))
        data = np.full(n, ord("a"), dtype=np.uint8)
        data[np.cumsum(rng.integers(1, 43, n // 20))[:n // 20] % n] = ord("b")
        pats = [b"a" * k for k in range(1, 9)]
    else:                                   # "spread": n / 4 pairs over the ids of a 100 000-pattern set, no scan
        data = np.zeros(1, dtype=np.uint8)
        pats = wl.snort_patterns(100000)
        h.setPerfMode(api.PFAC_SPACE_DRIVEN)
    h.readPatternFromFile(wl.write_pattern_file(os.path.join(tmp, kind + ".pat"), pats))
    f = int(h.info().numOfPatterns)
    most = int(h.info().maxMatchesPerPosition)
    d_counts = torch.zeros(f + 1, dtype=torch.int64, device="cuda:0")
    got = {}
    runs = {}

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

    if kind == "spread":
        pairs = n // 4
        d_a = torch.randint(1, f + 1, (pairs,), dtype=torch.int32, device="cuda:0")
        got["pairs"] = pairs
        calls = {"pairs_longest": lambda: h.countPairsFromDevice(d_a.data_ptr(), pairs, api.PFACX_COUNT_LONGEST, d_counts.data_ptr(), f + 1),
                 "pairs_all": lambda: h.countPairsFromDevice(d_a.data_ptr(), pairs, 0, d_counts.data_ptr(), f + 1)}
    else:
        d_in = torch.from_numpy(data).to("cuda:0")
        d_a = torch.empty(n, dtype=torch.int32, device="cuda:0")
        d_b = torch.empty(n, dtype=torch.int32, device="cuda:0")

        def reduce_call():
            got["pairs"] = h.matchFromDeviceReduce(d_in.data_ptr(), n, d_a.data_ptr(), d_b.data_ptr())[1]

        def count_call():
            got["occurrences"] = h.countFromDevice(d_in.data_ptr(), n, 0, d_counts.data_ptr(), f + 1)[1]

        def longest_call():
            got["longest"] = h.countFromDevice(d_in.data_ptr(), n, api.PFACX_COUNT_LONGEST, d_counts.data_ptr(), f + 1)[1]

        calls = {"reduce": reduce_call, "count": count_call, "count_longest": longest_call,
                 # the id list the compacted call left in d_a
                 "pairs_longest": lambda: h.countPairsFromDevice(d_a.data_ptr(), got["pairs"], api.PFACX_COUNT_LONGEST, d_counts.data_ptr(), f + 1),
                 "pairs_all": lambda: h.countPairsFromDevice(d_a.data_ptr(), got["pairs"], 0, d_counts.data_ptr(), f + 1)}
        if n * most <= (1 << 30):           # the do-it-yourself path holds 8 bytes per entry of its capacity
            cap = n * most
            d_i = torch.empty(cap, dtype=torch.int32, device="cuda:0")
            d_p = torch.empty(cap, dtype=torch.int32, device="cuda:0")

            def diy_call():
                listed = h.matchAllFromDevice(d_in.data_ptr(), n, d_i.data_ptr(), d_p.data_ptr(), cap)[1]
                got["diy_total"] = int(torch.bincount(d_i[:listed], minlength=f + 1).sum())

            calls["diy"] = diy_call
    # interleaved rounds: a drift of the clocks hits every call alike
    for _ in range(2):
        for k, fn in calls.items():
            if k == "pairs_longest" and "reduce" in calls:
                reduce_call()               # (the count calls in between do not touch d_a; the list is the compacted call's again all the same)
            runs.setdefault(k, []).append(median_ms(fn))
    scratch = int(h.info().deviceScratchBytes)
    h.destroy()
    best = {k: min(v) for k, v in runs.items()}
    rec = {"input": kind, "size": item.split(":")[-1], "bytes": n, "patterns": f, "max_chain": most, "pairs": got["pairs"]}
    for k, v in best.items():
        rec[k + "_ms"] = round(v, 4)
    if "count" in best:
        rec.update({"occurrences": got["occurrences"], "count_over_reduce": round(best["count"] / best["reduce"], 4),
                    "count_minus_reduce_ms": round(best["count"] - best["reduce"], 4)})
    rec["hist_store_Mpairs_per_s"] = round(got["pairs"] / best["pairs_longest"] / 1e3, 1) if got["pairs"] else None
    rec["chain_ms"] = round(best["pairs_all"] - best["pairs_longest"], 4)
    if "diy" in best:
        rec.update({"diy_total": got["diy_total"], "diy_over_count": round(best["diy"] / best["count"], 4)})
    rec["device_scratch_bytes"] = scratch
    rec["runs_ms"] = {k: [round(x, 4) for x in v] for k, v in runs.items()}
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64k,16,256,1024", help="MiB, or KiB with a k: C3's set over its stream")
    ap.add_argument("--others", default="covered:256,nested:32,spread:64", help="kind:size of the other inputs")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per item")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a.one, a.steps)
        return 0
    items = [s for s in a.sizes.split(",") if s] + [s for s in a.others.split(",") if s]
    lines = []
    rc = 0
    for item in items:
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
            f.write("# tools/count_sweep.py: PFACX_countFromDevice (count: all occurrences; count_longest: PFACX_COUNT_LONGEST) against PFAC_matchFromDeviceReduce (the same\n"
                    "# build: this change does not touch that path, so its timing stands in for the parent commit's); PFACX_countPairsFromDevice over the compacted call's id\n"
                    "# list (pairs_longest: memset + pfac_count_hist + pfac_count_store, also as pairs per second; pairs_all: + pfac_count_chain, chain_ms the difference);\n"
                    "# diy: PFACX_matchAllFromDevice + torch.bincount.  input c3: C3's set over its stream; covered: pattern a over a run of a (pairs == size, one id);\n"
                    "# nested: a .. a x 8 over runs of a; spread: size / 4 ids drawn evenly from the 100 000 ids of the S100 set (no scan).\n"
                    "# Median of %d event-timed calls after warm-up, the better of two interleaved rounds.\n" % a.steps)
            for ln in lines:
                f.write(ln + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
