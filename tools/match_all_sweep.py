"""tools/match_all_sweep.py -- what an all-match call (PFACX_matchAllFromDevice) costs against the compacted call
(PFAC_matchFromDeviceReduce) over the same bytes (GPU box only).  Both calls are synchronous; each is timed alone with HIP events
around it, the median of --steps calls after warm-up is reported.
  c3       C3's set (30 000 Snort-style patterns, hashed) over its HTTP stream: 256 MiB and 1 GiB
  c2       C2's set (1 000 random patterns, dense), which has no nested prefixes: the fast path, no expansion launch
  nested   C3's set plus every prefix of length 3..12 of 2 000 of its patterns, over the C3 stream (256 MiB)
  hostile  the Snort-length set of tests/test_hostile.py (lengths 1..243, 1- and 2-byte patterns; rebuilt here the same way) over
           64 MiB of its text
Every case runs in a child process of its own under a time limit; the first that fails ends the sweep.  One JSON line per case on
stdout; with --out the lines and a summary go to that file (profiles/match_all_sweep.txt).

    python tools/match_all_sweep.py [--cases c3:256,c3:1024,c2:256,nested:256,hostile:64] [--steps 20] [--out profiles/match_all_sweep.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hostile_set_and_stream(n):
    """the Snort-length set and its text as tests/test_hostile.py builds them (same seed, same steps)"""
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(2431))
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789 /.-_=&%:", dtype=np.uint8)
    pats = {b"q", b"Z", b"zq", b"0x", b"%%"}
    while len(pats) < 3000:
        u = rng.random()
        ln = int(rng.integers(1, 3)) if u < 0.01 else int(rng.integers(3, 40)) if u < 0.8 else int(rng.integers(40, 244))
        pats.add(alpha[rng.integers(0, alpha.size, ln)].tobytes())
    pats = sorted(pats, key=lambda p: (rng.random(), p))
    data = alpha[rng.integers(0, alpha.size, n)].copy()
    for k in range(400):
        p = np.frombuffer(pats[int(rng.integers(0, len(pats)))], dtype=np.uint8)
        at = int(rng.integers(0, n - 300)) if k % 4 else (int(rng.integers(1, n >> 13)) << 13) - int(rng.integers(1, 200))
        data[at:at + p.size] = p
    return pats, 0, data


def workload(case, n):
    from pfac_amd import workloads as wl
    if case == "hostile":
        return hostile_set_and_stream(n)
    cfg = wl.make_config("c2" if case == "c2" else "c3")
    pats = list(cfg.patterns)
    if case == "nested":
        seen = set(pats)
        for p in cfg.patterns[:2000]:
            for k in range(3, 13):
                if k < len(p) and p[:k] not in seen:
                    seen.add(p[:k])
                    pats.append(p[:k])
    return pats, cfg.perf_mode, cfg.input_slice(n, 0)


def one(case, size_mib, steps):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pfac_amd import api, hiprt
    from pfac_amd import workloads as wl

    n = size_mib << 20
    pats, perf, data = workload(case, n)
    pf = wl.write_pattern_file(os.path.join(tempfile.mkdtemp(), case + ".pat"), pats)
    h = api.PFAC.create()
    h.setPerfMode(perf)
    h.readPatternFromFile(pf)
    chains = h.info().maxMatchesPerPosition
    d_in = torch.from_numpy(np.ascontiguousarray(data)).to("cuda:0")
    cap = n * chains
    d_ids = torch.empty(cap, dtype=torch.int32, device="cuda:0")
    d_pos = torch.empty(cap, dtype=torch.int32, device="cuda:0")
    counts = {}

    def reduce_call():
        counts["longest"] = h.matchFromDeviceReduce(d_in.data_ptr(), n, d_ids.data_ptr(), d_pos.data_ptr())[1]

    def all_call():
        counts["all"] = h.matchAllFromDevice(d_in.data_ptr(), n, d_ids.data_ptr(), d_pos.data_ptr(), cap)[1]

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

    # interleaved rounds: a drift of the clocks hits both calls alike
    r1 = median_ms(reduce_call)
    a1 = median_ms(all_call)
    r2 = median_ms(reduce_call)
    a2 = median_ms(all_call)
    red, alls = min(r1, r2), min(a1, a2)
    h.destroy()
    print(json.dumps({"case": case, "size_mib": size_mib, "maxMatchesPerPosition": chains, "longest_pairs": counts["longest"],
                      "all_pairs": counts["all"], "reduce_ms": round(red, 4), "all_ms": round(alls, 4),
                      "expansion_ms": round(alls - red, 4), "ratio": round(alls / red, 4),
                      "runs_ms": {"reduce": [round(r1, 4), round(r2, 4)], "all": [round(a1, 4), round(a2, 4)]}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c3:256,c3:1024,c2:256,nested:256,hostile:64")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per case")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        case, mib = a.one.split(":")
        one(case, int(mib), a.steps)
        return 0
    lines = []
    rc = 0
    for item in a.cases.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", item, "--steps", str(a.steps)], cwd=ROOT,
                               timeout=a.timeout, stdout=subprocess.PIPE)
        except subprocess.TimeoutExpired:
            lines.append(json.dumps({"case": item, "error": "time limit"}))
            rc = 124
            break
        out = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
        lines.extend(out)
        for ln in out:
            print(ln, flush=True)
        if p.returncode != 0:
            lines.append(json.dumps({"case": item, "error": "exit %d" % p.returncode}))
            rc = p.returncode if p.returncode > 0 else 1
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/match_all_sweep.py: PFACX_matchAllFromDevice against PFAC_matchFromDeviceReduce, same bytes, same handle;\n"
                    "# median of %d event-timed calls after warm-up, the better of two interleaved rounds; expansion_ms = all_ms - reduce_ms\n" % a.steps)
            for ln in lines:
                f.write(ln + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
