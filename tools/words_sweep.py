"""tools/words_sweep.py -- what the words calls cost (GPU box only).  PFACX_matchWordsFromDevice, the word list (words) and PFACX_WORDS_ALL
(words_all), default class, against PFACX_matchAllFromDevice (all) and PFAC_matchFromDeviceReduce (reduce) over the same bytes -- they run the same
scan: C3's set over its stream.  The boundary passes alone: PFACX_wordsPairsFromDevice over the list the reduce call left (pairs, pairs_all; also
as pairs per second).  The do-it-yourself path (diy): PFACX_matchAllFromDevice with capacity = size x maxMatchesPerPosition, then the boundary test
in torch -- two gathers of the input per entry, a mask, two masked selects.  All calls are timed alone with HIP events around them; the median of
--steps calls after warm-up, the better of two interleaved rounds.  The expectation the record checks: the extra of words_all over all follows the
pairs, not the bytes (extra_ns_per_pair next to extra_ns_per_byte over the sizes).
Every size runs in a child process of its own under a time limit; the first that fails ends the sweep.  One JSON line per size on stdout; with --out
the lines go to that file (profiles/words_sweep.txt).

    python tools/words_sweep.py [--sizes 64k,16,256,1024] [--steps 20] [--out profiles/words_sweep.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def size_of(item):
    return int(item[:-1]) << 10 if item.endswith("k") else int(item) << 20


def one(item, steps):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pfac_amd import api, hiprt
    from pfac_amd import workloads as wl

    n = size_of(item)
    tmp = tempfile.mkdtemp()
    h = api.PFAC.create()
    cfg = wl.make_config("c3")
    data = np.ascontiguousarray(cfg.input_slice(n, 0))
    pats = list(cfg.patterns)
    h.setPerfMode(cfg.perf_mode)
    h.readPatternFromFile(wl.write_pattern_file(os.path.join(tmp, "c3.pat"), pats))
    most = int(h.info().maxMatchesPerPosition)
    cls = api.word_class()
    d_in = torch.from_numpy(data).to("cuda:0")
    d_a, d_b, d_i, d_p = (torch.empty(n, dtype=torch.int32, device="cuda:0") for _ in range(4))
    got, runs = {}, {}

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

    def reduce_call():
        got["pairs"] = h.matchFromDeviceReduce(d_in.data_ptr(), n, d_a.data_ptr(), d_b.data_ptr())[1]

    def all_call():
        got["all"] = h.matchAllFromDevice(d_in.data_ptr(), n, d_i.data_ptr(), d_p.data_ptr(), n, check=False)[1]

    def words_call():
        got["words"] = h.matchWordsFromDevice(d_in.data_ptr(), n, cls, 0, d_i.data_ptr(), d_p.data_ptr(), n)[1]

    def words_all_call():
        got["words_all"] = h.matchWordsFromDevice(d_in.data_ptr(), n, cls, api.PFACX_WORDS_ALL, d_i.data_ptr(), d_p.data_ptr(), n)[1]

    calls = {"reduce": reduce_call, "all": all_call, "words": words_call, "words_all": words_all_call,
             # the list the reduce call left in d_a / d_b
             "pairs": lambda: h.wordsPairsFromDevice(d_in.data_ptr(), n, cls, 0, d_a.data_ptr(), d_b.data_ptr(), got["pairs"], d_i.data_ptr(), d_p.data_ptr(), n),
             "pairs_all": lambda: h.wordsPairsFromDevice(d_in.data_ptr(), n, cls, api.PFACX_WORDS_ALL, d_a.data_ptr(), d_b.data_ptr(), got["pairs"],
                                                         d_i.data_ptr(), d_p.data_ptr(), n)}
    if n * most <= (1 << 30):               # the do-it-yourself path holds 8 bytes per entry of its capacity
        cap = n * most
        d_ci = torch.empty(cap, dtype=torch.int32, device="cuda:0")
        d_cp = torch.empty(cap, dtype=torch.int32, device="cuda:0")
        d_len = torch.tensor([0] + [len(p) for p in pats], dtype=torch.int64, device="cuda:0")
        inw = torch.zeros(256, dtype=torch.bool, device="cuda:0")
        inw[torch.tensor(list(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz_"), device="cuda:0")] = True

        def diy_call():
            listed = h.matchAllFromDevice(d_in.data_ptr(), n, d_ci.data_ptr(), d_cp.data_ptr(), cap)[1]
            ids, pos = d_ci[:listed].long(), d_cp[:listed].long()
            end = pos + d_len[ids]
            ok = ((pos == 0) | ~inw[d_in[(pos - 1).clamp(min=0)].long()]) & ((end == n) | ~inw[d_in[end.clamp(max=n - 1)].long()])
            kept_ids, kept_pos = ids[ok], pos[ok]
            got["diy"] = int(kept_ids.numel())
            assert kept_pos.numel() == got["diy"]

        calls["diy"] = diy_call
    for _ in range(2):                      # interleaved rounds: a drift of the clocks hits every call alike
        for k, fn in calls.items():
            if k == "pairs":
                reduce_call()
            runs.setdefault(k, []).append(median_ms(fn))
    scratch = int(h.info().deviceScratchBytes)
    h.destroy()
    best = {k: min(v) for k, v in runs.items()}
    pairs = got["pairs"]
    rec = {"input": "c3", "size": item, "bytes": n, "patterns": len(pats), "max_chain": most, "pairs": pairs, "all_listed": got["all"],
           "words_listed": got["words"], "words_all_listed": got["words_all"]}
    for k, v in best.items():
        rec[k + "_ms"] = round(v, 4)
    extra = best["words_all"] - best["all"]
    rec.update({"words_over_reduce": round(best["words"] / best["reduce"], 4), "words_all_over_all": round(best["words_all"] / best["all"], 4),
                "extra_over_all_ms": round(extra, 4), "extra_ns_per_pair": round(extra * 1e6 / pairs, 3) if pairs else None,
                "extra_ns_per_byte": round(extra * 1e6 / n, 4),
                "passes_Mpairs_per_s": round(pairs / best["pairs_all"] / 1e3, 1) if pairs else None})
    if "diy" in best:
        assert got["diy"] == got["words_all"], (got["diy"], got["words_all"])
        rec["diy_over_words_all"] = round(best["diy"] / best["words_all"], 4)
    rec["device_scratch_bytes"] = scratch
    rec["runs_ms"] = {k: [round(x, 4) for x in v] for k, v in runs.items()}
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64k,16,256,1024", help="MiB, or KiB with a k: C3's set over its stream")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per size")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a.one, a.steps)
        return 0
    lines = []
    rc = 0
    for item in [s for s in a.sizes.split(",") if s]:
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
            f.write("# tools/words_sweep.py: PFACX_matchWordsFromDevice (words: the word list; words_all: PFACX_WORDS_ALL; default class) against PFACX_matchAllFromDevice (all)\n"
                    "# and PFAC_matchFromDeviceReduce (reduce) of the same build (this change does not touch those paths, so their timing stands in for the parent commit's);\n"
                    "# pairs / pairs_all: PFACX_wordsPairsFromDevice over the reduce call's list, the boundary passes alone; diy: PFACX_matchAllFromDevice + the boundary test in torch.\n"
                    "# C3's set over its stream.  Median of %d event-timed calls after warm-up, the better of two interleaved rounds.\n" % a.steps)
            for ln in lines:
                f.write(ln + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
