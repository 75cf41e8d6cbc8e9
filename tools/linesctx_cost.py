#!/usr/bin/env python3
"""What the context stage of PFACX_matchLinesContextFromDevice costs: the plain PFACX_matchLinesFromDevice, the context call
with before = after = 0 and with before = after = 3 on one handle over one input -- synthetic HTTP traffic (pfac_amd.workloads.http_stream:
lines of a few dozen bytes) under a Snort-like set of a few thousand patterns.  The three calls alternate round by round; every call is
synchronous (its counts come to the host), so the host clock around it is the call's time.  Prints the median and the spread of each and
the two differences as one JSON line.

    python tools/linesctx_cost.py [--mib 256] [--patterns 3000] [--rounds 15] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--patterns", type=int, default=3000)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import tempfile

    import torch

    from pfac_amd import api
    from pfac_amd import workloads as wl

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    n = args.mib << 20
    pats = wl.snort_patterns(args.patterns)
    data = wl.http_stream(n, wl.http_message_pool(pats))
    with tempfile.TemporaryDirectory() as tmp:
        pf = wl.write_pattern_file(os.path.join(tmp, "cost.pat"), pats)
        h = api.PFAC.create()
        h.readPatternFromFile(pf)
    d_in = torch.from_numpy(data).to("cuda:0")
    d_start, d_len, d_index, d_tag = (torch.empty(n, dtype=torch.int32, device="cuda:0") for _ in range(4))
    I, S, L, X, T = d_in.data_ptr(), d_start.data_ptr(), d_len.data_ptr(), d_index.data_ptr(), d_tag.data_ptr()
    calls = {
        "plain": lambda: h.matchLinesFromDevice(I, n, 0, S, L, X, n)[1:],
        "context_0": lambda: h.matchLinesContextFromDevice(I, n, 0, 0, 0, S, L, X, T, n)[1:],
        "context_3": lambda: h.matchLinesContextFromDevice(I, n, 0, 3, 3, S, L, X, T, n)[1:],
    }
    times = {k: [] for k in calls}
    counts = {}
    for r in range(args.warmup + args.rounds):
        for name, call in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            counts[name] = call()
            t1 = time.perf_counter()
            if r >= args.warmup:
                times[name].append((t1 - t0) * 1e3)
    h.destroy()
    assert counts["context_0"][:2] == counts["plain"] and counts["context_0"][1] == counts["context_0"][2], counts
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {
        "mib": args.mib, "patterns": len(pats), "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
        "lines": counts["plain"][0], "matching_lines": counts["plain"][1], "selected_context_3": counts["context_3"][1],
        "groups_context_3": counts["context_3"][3],
        "ms_median": {k: round(v, 4) for k, v in med.items()},
        "ms_min": {k: round(min(v), 4) for k, v in times.items()},
        "ms_max": {k: round(max(v), 4) for k, v in times.items()},
        "ms_context_0_minus_plain": round(med["context_0"] - med["plain"], 4),
        "ms_context_3_minus_plain": round(med["context_3"] - med["plain"], 4),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
