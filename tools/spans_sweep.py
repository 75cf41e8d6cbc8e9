"""tools/spans_sweep.py -- what the spans calls cost (GPU box only).  (a) PFACX_matchSpansFromDevice against the compacted call
(PFAC_matchFromDeviceReduce) over the same bytes, the floor it cannot go below: C3's set over its stream; (b) the same on an all-covered input
(pattern "a" over a run of "a": pairs == size), the worst case of the pair-space passes; (c) PFACX_redactSpansFromDevice out of place and in
place, as bytes read plus bytes written per second (out of place: 2 x size minus the covered bytes, which are not read; in place: what the
threads that cover something read and write is not known to the host -- reported as size per second), at C3's density and on the "abab..."
input (pattern "a": every second byte a span); (d) a do-it-yourself path in torch: the compacted call, a gather of the pattern lengths, cummax,
compare, nonzero, and a masked fill through a difference array and cumsum.  All calls are timed alone with HIP events around them; the median
of --steps calls after warm-up, the better of two interleaved rounds.
Every size runs in a child process of its own under a time limit; the first that fails ends the sweep.  One JSON line per size on stdout; with
--out the lines go to that file (profiles/spans_sweep.txt).

    python tools/spans_sweep.py [--sizes 64k,16,256,1024] [--covered 256] [--steps 20] [--out profiles/spans_sweep.txt]
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
    else:                                   # "covered": pairs == size; "abab": every second byte a span
        data = np.full(n, ord("a"), dtype=np.uint8)
        if kind == "abab":
            data[1::2] = ord("b")
        pats = [b"a"]
    h.readPatternFromFile(wl.write_pattern_file(os.path.join(tmp, kind + ".pat"), pats))
    lens = torch.tensor([0] + [len(p) for p in pats], dtype=torch.int64, device="cuda:0")
    d_in = torch.from_numpy(data).to("cuda:0")
    d_a = torch.empty(n, dtype=torch.int32, device="cuda:0")
    d_b = torch.empty(n, dtype=torch.int32, device="cuda:0")
    d_s = torch.empty(n, dtype=torch.int32, device="cuda:0")
    d_l = torch.empty(n, dtype=torch.int32, device="cuda:0")
    d_out = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    d_work = d_in.clone()
    got = {}

    def reduce_call():
        got["pairs"] = h.matchFromDeviceReduce(d_in.data_ptr(), n, d_a.data_ptr(), d_b.data_ptr())[1]

    def spans_call():
        _, got["spans"], got["covered"] = h.matchSpansFromDevice(d_in.data_ptr(), n, d_s.data_ptr(), d_l.data_ptr(), n)

    def redact_call():
        h.redactSpansFromDevice(d_in.data_ptr(), n, d_s.data_ptr(), d_l.data_ptr(), got["spans"], 0x2A, d_out.data_ptr())

    def redact_in_place_call():             # (after the first call the covered bytes hold the fill already: the work is the same)
        h.redactSpansFromDevice(d_work.data_ptr(), n, d_s.data_ptr(), d_l.data_ptr(), got["spans"], 0x2A, d_work.data_ptr())

    def diy_call():
        cnt = h.matchFromDeviceReduce(d_in.data_ptr(), n, d_a.data_ptr(), d_b.data_ptr())[1]
        if cnt == 0:
            got["diy_spans"] = 0
            d_out.copy_(d_in)
            return
        pos = d_b[:cnt].to(torch.int64)
        end = pos + lens[d_a[:cnt].to(torch.int64)]
        top = torch.cummax(end, 0).values
        head = torch.ones(cnt, dtype=torch.bool, device="cuda:0")
        head[1:] = pos[1:] > top[:-1]
        first = torch.nonzero(head).flatten()
        got["diy_spans"] = int(first.numel())
        last = torch.cat([first[1:] - 1, torch.full((1,), cnt - 1, dtype=torch.int64, device="cuda:0")])
        mark = torch.zeros(n + 1, dtype=torch.int32, device="cuda:0")
        mark[pos[first]] = 1
        mark.index_add_(0, top[last], torch.full((first.numel(),), -1, dtype=torch.int32, device="cuda:0"))
        torch.where(torch.cumsum(mark[:n], 0) > 0, torch.full((), 0x2A, dtype=torch.uint8, device="cuda:0"), d_in, out=d_out)

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
    runs = {k: [] for k in ("reduce", "spans", "redact", "redact_in_place", "diy")}
    diy = n <= (256 << 20)                  # the torch path holds a dozen 8-byte temporaries per pair and 4 bytes per input byte
    for _ in range(2):
        runs["reduce"].append(median_ms(reduce_call))
        runs["spans"].append(median_ms(spans_call))
        runs["redact"].append(median_ms(redact_call))           # the list the call in front of it left
        runs["redact_in_place"].append(median_ms(redact_in_place_call))
        if diy:
            runs["diy"].append(median_ms(diy_call))
    scratch = int(h.info().deviceScratchBytes)
    h.destroy()
    best = {k: min(v) for k, v in runs.items() if v}
    gbs = lambda nbytes, ms: round(nbytes / ms / 1e6, 2) if ms > 0 else None  # noqa: E731
    rec = {
        "input": kind, "size": item.split(":")[-1], "bytes": n, "pairs": got["pairs"], "spans": got["spans"], "covered": got["covered"],
        "reduce_ms": round(best["reduce"], 4), "spans_ms": round(best["spans"], 4), "spans_extra_ms": round(best["spans"] - best["reduce"], 4),
        "spans_over_reduce": round(best["spans"] / best["reduce"], 4),
        "redact_ms": round(best["redact"], 4), "redact_rw_GBps": gbs(2 * n - got["covered"], best["redact"]),
        "redact_in_place_ms": round(best["redact_in_place"], 4), "redact_in_place_size_GBps": gbs(n, best["redact_in_place"]),
        "device_scratch_bytes": scratch}
    if diy:
        rec.update({"diy_spans": got["diy_spans"], "diy_ms": round(best["diy"], 4),
                    "diy_over_spans_plus_redact": round(best["diy"] / (best["spans"] + best["redact"]), 4)})
    rec["runs_ms"] = {k: [round(x, 4) for x in v] for k, v in runs.items() if v}
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64k,16,256,1024", help="MiB, or KiB with a k: C3's set over its stream")
    ap.add_argument("--covered", default="256", help="sizes of the all-covered input and of the abab input")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per size")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a.one, a.steps)
        return 0
    items = [s for s in a.sizes.split(",") if s] + ["%s:%s" % (k, s) for s in a.covered.split(",") if s for k in ("covered", "abab")]
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
            f.write("# tools/spans_sweep.py: PFACX_matchSpansFromDevice against PFAC_matchFromDeviceReduce (the same build: this change does not touch that path, so\n"
                    "# its timing stands in for the parent commit's), PFACX_redactSpansFromDevice out of place (redact_rw = 2 x size - covered bytes per second) and in\n"
                    "# place (size per second), and a do-it-yourself path in torch (compacted call, length gather, cummax, compare, nonzero, difference array + cumsum +\n"
                    "# where).  input c3: C3's set over its stream; covered: pattern a over a run of a (pairs == size); abab: pattern a over abab... (size / 2 spans).\n"
                    "# Median of %d event-timed calls after warm-up, the better of two interleaved rounds.\n" % a.steps)
            for ln in lines:
                f.write(ln + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
