"""tools/disjoint_sweep.py -- what the disjoint and the replace calls cost (GPU box only).  (a) PFACX_matchDisjointFromDevice against the compacted
call (PFAC_matchFromDeviceReduce) over the same bytes, the floor it cannot go below: C3's set over its stream, the all-covered input (pattern "a"
over a run of "a": pairs == size) and "abab..." under ab / ba (pairs == size, two chains that never merge); (b) PFACX_replaceFromDevice as bytes
read plus bytes written per second (size - covered bytes read, outBytes written), every pattern replaced by a tag of 5 bytes (C3) or "a" -> "b",
next to the out-of-place redaction and the gather of one line per span over the same buffers; (c) a do-it-yourself path: the compacted call, the
pairs copied to the host, the sequential selection in numpy / Python and a Python join of the pieces.  All library calls are timed alone with HIP
events around them; the median of --steps calls after warm-up, the better of two interleaved rounds; the do-it-yourself path by the wall clock.
Every size runs in a child process of its own under a time limit; the first that fails ends the sweep.  One JSON line per size on stdout; with
--out the lines go to that file (profiles/disjoint_sweep.txt).

    python tools/disjoint_sweep.py [--sizes 64k,16,256,1024] [--dense 256] [--steps 10] [--out profiles/disjoint_sweep.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

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
        repls = [b""] + [b"<TAG>"] * len(pats)
    else:                                   # "covered": a over a...; "abab": ab / ba over abab...
        data = np.full(n, ord("a"), dtype=np.uint8)
        pats = [b"a"]
        repls = [b"", b"b"]
        if kind == "abab":
            data[1::2] = ord("b")
            pats = [b"ab", b"ba"]
            repls = [b"", b"AB", b"BA"]
    h.readPatternFromFile(wl.write_pattern_file(os.path.join(tmp, kind + ".pat"), pats))
    lens = np.array([0] + [len(p) for p in pats], dtype=np.int64)
    off = np.concatenate(([0], np.cumsum([len(r) for r in repls]))).astype(np.int32)
    blob = np.frombuffer(b"".join(repls), dtype=np.uint8).copy()
    d_off, d_blob = torch.from_numpy(off).to("cuda:0"), torch.from_numpy(blob).to("cuda:0")
    d_in = torch.from_numpy(data).to("cuda:0")
    d_a, d_b, d_i, d_p, d_s, d_l = (torch.empty(n, dtype=torch.int32, device="cuda:0") for _ in range(6))
    d_red = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    got = {}

    def reduce_call():
        got["pairs"] = h.matchFromDeviceReduce(d_in.data_ptr(), n, d_a.data_ptr(), d_b.data_ptr())[1]

    def disjoint_call():
        _, got["tokens"], got["covered"] = h.matchDisjointFromDevice(d_in.data_ptr(), n, d_i.data_ptr(), d_p.data_ptr(), n)

    disjoint_call()
    got["out_bytes"] = h.replaceFromDevice(d_in.data_ptr(), n, d_i.data_ptr(), d_p.data_ptr(), got["tokens"], d_off.data_ptr(), off.size, d_blob.data_ptr(),
                                           blob.size, None, 0, check=False)[1]
    d_out = torch.empty(max(got["out_bytes"], 1), dtype=torch.uint8, device="cuda:0")
    _, got["spans"], _ = h.matchSpansFromDevice(d_in.data_ptr(), n, d_s.data_ptr(), d_l.data_ptr(), n)
    d_gather = torch.empty(n + got["spans"] + 1, dtype=torch.uint8, device="cuda:0")

    def replace_call():
        h.replaceFromDevice(d_in.data_ptr(), n, d_i.data_ptr(), d_p.data_ptr(), got["tokens"], d_off.data_ptr(), off.size, d_blob.data_ptr(), blob.size,
                            d_out.data_ptr(), got["out_bytes"])

    def redact_call():
        h.redactSpansFromDevice(d_in.data_ptr(), n, d_s.data_ptr(), d_l.data_ptr(), got["spans"], 0x2A, d_red.data_ptr())

    def gather_call():                      # the spans as "lines": the covered bytes and a newline behind each
        got["gather_bytes"] = h.gatherLinesFromDevice(d_in.data_ptr(), n, d_s.data_ptr(), d_l.data_ptr(), got["spans"], d_gather.data_ptr(), d_gather.numel())[1]

    def diy_call():
        cnt = h.matchFromDeviceReduce(d_in.data_ptr(), n, d_a.data_ptr(), d_b.data_ptr())[1]
        ids, pos = d_a[:cnt].cpu().numpy(), d_b[:cnt].cpu().numpy()
        end = pos.astype(np.int64) + lens[ids]
        pieces, at, k = [], 0, 0
        raw = data.tobytes()
        while k < cnt:                      # the loop of the definition over the pairs
            pieces.append(raw[at:pos[k]])
            pieces.append(repls[ids[k]])
            at = int(end[k])
            k = int(np.searchsorted(pos, at, side="left"))
        pieces.append(raw[at:])
        got["diy_bytes"] = len(b"".join(pieces))

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
    runs = {k: [] for k in ("reduce", "disjoint", "replace", "redact", "gather", "diy")}
    diy = kind == "c3" and n <= (256 << 20)     # a Python loop per token: minutes on the dense inputs
    for _ in range(2):
        runs["reduce"].append(median_ms(reduce_call))
        runs["disjoint"].append(median_ms(disjoint_call))
        runs["replace"].append(median_ms(replace_call))
        runs["redact"].append(median_ms(redact_call))
        if got["spans"]:
            runs["gather"].append(median_ms(gather_call))
        if diy:
            t0 = time.perf_counter()
            diy_call()
            runs["diy"].append((time.perf_counter() - t0) * 1e3)
    scratch = int(h.info().deviceScratchBytes)
    h.destroy()
    best = {k: min(v) for k, v in runs.items() if v}
    gbs = lambda nbytes, ms: round(nbytes / ms / 1e6, 2) if ms > 0 else None  # noqa: E731
    blocks = (got["pairs"] + api.PFACX_DISJOINT_BLOCK - 1) // api.PFACX_DISJOINT_BLOCK
    rec = {
        "input": kind, "size": item.split(":")[-1], "bytes": n, "pairs": got["pairs"], "tokens": got["tokens"], "covered": got["covered"],
        "doubling_rounds": max(blocks - 1, 0).bit_length(),
        "reduce_ms": round(best["reduce"], 4), "disjoint_ms": round(best["disjoint"], 4), "disjoint_extra_ms": round(best["disjoint"] - best["reduce"], 4),
        "disjoint_over_reduce": round(best["disjoint"] / best["reduce"], 4),
        "out_bytes": got["out_bytes"], "replace_ms": round(best["replace"], 4), "replace_rw_GBps": gbs(n - got["covered"] + got["out_bytes"], best["replace"]),
        "redact_ms": round(best["redact"], 4), "redact_rw_GBps": gbs(2 * n - got["covered"], best["redact"]),
        "device_scratch_bytes": scratch}
    if "gather" in best:
        rec.update({"gather_ms": round(best["gather"], 4), "gather_rw_GBps": gbs(2 * got["gather_bytes"] - got["spans"], best["gather"])})
    if diy:
        assert got["diy_bytes"] == got["out_bytes"], "the do-it-yourself path builds another text"
        rec.update({"diy_ms": round(best["diy"], 4), "diy_over_disjoint_plus_replace": round(best["diy"] / (best["disjoint"] + best["replace"]), 4)})
    rec["runs_ms"] = {k: [round(x, 4) for x in v] for k, v in runs.items() if v}
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64k,16,256,1024", help="MiB, or KiB with a k: C3's set over its stream")
    ap.add_argument("--dense", default="256", help="sizes of the all-covered input and of the abab input")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per size")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a.one, a.steps)
        return 0
    items = [s for s in a.sizes.split(",") if s] + ["%s:%s" % (k, s) for s in a.dense.split(",") if s for k in ("covered", "abab")]
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
            f.write("# tools/disjoint_sweep.py: PFACX_matchDisjointFromDevice against PFAC_matchFromDeviceReduce (the same build: this change does not touch that path,\n"
                    "# so its timing stands in for the parent commit's), PFACX_replaceFromDevice (replace_rw = size - covered + outBytes per second) next to the\n"
                    "# out-of-place redaction and the gather of the spans over the same buffers, and a do-it-yourself path (compacted call, pairs to the host, the\n"
                    "# sequential selection and a Python join; wall clock).  input c3: C3's set over its stream, every pattern -> <TAG>; covered: a -> b over a run of a\n"
                    "# (pairs == size); abab: ab / ba over abab... (pairs == size, two chains).  Median of %d event-timed calls after warm-up, the better of two\n"
                    "# interleaved rounds.\n" % a.steps)
            for ln in lines:
                f.write(ln + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
