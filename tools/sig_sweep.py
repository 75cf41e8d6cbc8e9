"""tools/sig_sweep.py -- what the signature calls cost (GPU box only).  A seeded set of signatures (tests/sig_ref.py: random_signatures; 16 - 200
bytes, 0 - 20 % wildcard bytes, one in four of them a half byte) over C3's stream with occurrences and near misses embedded at seeded places.
PFACX_sigMatchFromDevice (sig) against PFAC_matchFromDeviceReduce (reduce) on the same handle over the same bytes -- the same scan over the anchors;
its code is untouched by the signature calls, so its timing stands in for the parent commit's.  The passes alone: PFACX_sigPairsFromDevice over the
list the reduce call left (pairs).  The do-it-yourself path (diy): the reduce call, its pairs copied to the host, then per signature a numpy masked
compare at the starts its anchor's pairs give, over a host copy of the input (wall clock, the copy of the input not counted).
The device calls are timed alone with HIP events around them; the median of --steps calls after warm-up, the better of two interleaved rounds.  The
expectation the record checks: the extra of sig over reduce follows the pairs, not the bytes; the last line fits extra = fixed + per_pair * pairs over
the sizes and says whether that held.
Every size runs in a child process of its own under a time limit; the first that fails ends the sweep.  One JSON line per size on stdout; with --out
the lines go to that file (profiles/sig_sweep.txt).

    python tools/sig_sweep.py [--sizes 64k,16,256,1024] [--steps 20] [--sigs 2000] [--out profiles/sig_sweep.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261021


def size_of(item):
    return int(item[:-1]) << 10 if item.endswith("k") else int(item) << 20


def one(item, steps, num_sigs):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pfac_amd import api, hiprt
    from pfac_amd import workloads as wl
    from tests import sig_ref as ref

    n = size_of(item)
    cfg = wl.make_config("c3")
    sigs = ref.random_signatures(SEED, num_sigs)
    data = np.ascontiguousarray(cfg.input_slice(n, 0)).copy()
    ref.embed(sigs, data, SEED, per_sig=min(64, max(1, n >> 22)), near_misses=min(16, max(1, n >> 24)))
    h = api.PFAC.create()
    h.setPerfMode(cfg.perf_mode)
    sg = h.sigOpen(*ref.csr_of(sigs))
    anchor_id, anchor_off, _ = sg.anchors()

    d_in = torch.from_numpy(data).to("cuda:0")
    d_a, d_b, d_i, d_p = (torch.empty(n, dtype=torch.int32, device="cuda:0") for _ in range(4))
    got, runs = {}, {}

    def median_ms(fn, reps):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(reps):
            a, b = hiprt.Event(), hiprt.Event()
            a.record(0)
            fn()
            b.record(0)
            torch.cuda.synchronize()
            t.append(a.elapsed_ms(b))
        return float(np.median(t))

    def reduce_call():
        got["pairs"] = h.matchFromDeviceReduce(d_in.data_ptr(), n, d_a.data_ptr(), d_b.data_ptr())[1]

    def sig_call():
        got["sig"] = sg.match_device(d_in.data_ptr(), n, d_i.data_ptr(), d_p.data_ptr(), n)[1]

    def pairs_call():
        got["pairs_listed"] = sg.pairs_device(d_in.data_ptr(), n, d_a.data_ptr(), d_b.data_ptr(), got["pairs"], d_i.data_ptr(), d_p.data_ptr(), n)[1]

    # the signatures behind a longest pair of anchor q: those of every anchor that is a prefix of q's bytes (its chain)
    anchors = ref.model_anchors(sigs)[1]
    of_anchor = {}
    for i in range(1, len(sigs) + 1):
        of_anchor.setdefault(int(anchor_id[i]), []).append(i)
    by_anchor = {q: [i for r, short in enumerate(anchors, 1) if long.startswith(short) for i in of_anchor.get(r, ())]
                 for q, long in enumerate(anchors, 1)}

    def diy_wall_ms():
        t0 = time.perf_counter()
        k = h.matchFromDeviceReduce(d_in.data_ptr(), n, d_a.data_ptr(), d_b.data_ptr())[1]
        ids, pos = d_a[:k].cpu().numpy(), d_b[:k].cpu().numpy().astype(np.int64)
        found = 0
        order = np.argsort(ids, kind="stable")
        ids, pos = ids[order], pos[order]
        cuts = np.flatnonzero(np.diff(ids)) + 1
        for q, at in zip(ids[np.concatenate(([0], cuts))].tolist() if k else [], np.split(pos, cuts) if k else []):
            for i in by_anchor.get(q, ()):
                v, m = sigs[i - 1]
                s = at - int(anchor_off[i])
                s = s[(s >= 0) & (s + len(v) <= n)]
                for c in range(0, s.size, 1 << 16):
                    window = data[s[c:c + (1 << 16), None] + np.arange(len(v))[None, :]]
                    found += int((((window ^ v) & m) == 0).all(axis=1).sum())
        got["diy"] = found
        return (time.perf_counter() - t0) * 1e3

    calls = {"reduce": reduce_call, "sig": sig_call, "pairs": pairs_call}
    for _ in range(2):                      # interleaved rounds: a drift of the clocks hits every call alike
        for k, fn in calls.items():
            if k == "pairs":
                reduce_call()
            runs.setdefault(k, []).append(median_ms(fn, steps))
    runs["diy"] = [float(np.median([diy_wall_ms() for _ in range(3)]))]
    info = h.info()
    scratch, tables = int(info.deviceScratchBytes), int(info.deviceTableBytes)
    sg.close()
    h.destroy()
    best = {k: min(v) for k, v in runs.items()}
    assert got["pairs_listed"] == got["sig"] == got["diy"], got
    extra = best["sig"] - best["reduce"]
    rec = {"input": "c3 stream, seeded signatures embedded", "size": item, "bytes": n, "signatures": len(sigs), "anchors": int(anchor_id.max()),
           "pairs": got["pairs"], "listed": got["sig"]}
    for k, v in best.items():
        rec[k + "_ms"] = round(v, 4)
    rec.update({"sig_over_reduce": round(best["sig"] / best["reduce"], 4), "extra_over_reduce_ms": round(extra, 4),
                "extra_ns_per_pair": round(extra * 1e6 / got["pairs"], 3) if got["pairs"] else None, "extra_ns_per_byte": round(extra * 1e6 / n, 5),
                "diy_over_sig": round(best["diy"] / best["sig"], 3), "device_scratch_bytes": scratch, "device_table_bytes": tables,
                "runs_ms": {k: [round(x, 4) for x in v] for k, v in runs.items()}})
    print(json.dumps(rec), flush=True)


def fit(lines):
    """extra = fixed + per_pair * pairs over the sizes, least squares -> a record, or None with fewer than two sizes"""
    recs = [json.loads(ln) for ln in lines if '"extra_over_reduce_ms"' in ln]
    if len(recs) < 2:
        return None
    x = [float(r["pairs"]) for r in recs]
    y = [float(r["extra_over_reduce_ms"]) for r in recs]
    mx, my = sum(x) / len(x), sum(y) / len(y)
    sxx = sum((a - mx) ** 2 for a in x)
    slope = sum((a - mx) * (b - my) for a, b in zip(x, y)) / sxx if sxx else 0.0
    fixed = my - slope * mx
    worst = max(abs(b - (fixed + slope * a)) for a, b in zip(x, y))
    per_byte = [r["extra_ns_per_byte"] for r in recs]
    return {"fit": "extra_over_reduce = fixed + per_pair * pairs", "fixed_us": round(fixed * 1e3, 2), "per_pair_ns": round(slope * 1e6, 3),
            "worst_residual_us": round(worst * 1e3, 2), "extra_ns_per_byte_by_size": per_byte,
            "extra_follows_pairs_not_bytes": bool(worst <= max(0.010, 0.25 * max(y)) and per_byte[-1] < per_byte[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64k,16,256,1024", help="MiB, or KiB with a k: slices of C3's stream")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sigs", type=int, default=2000)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per size")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a.one, a.steps, a.sigs)
        return 0
    lines = []
    rc = 0
    for item in [s for s in a.sizes.split(",") if s]:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", item, "--steps", str(a.steps), "--sigs", str(a.sigs)], cwd=ROOT,
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
    fitted = fit(lines)
    if fitted:
        lines.append(json.dumps(fitted))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/sig_sweep.py: PFACX_sigMatchFromDevice (sig) against PFAC_matchFromDeviceReduce (reduce) on the same handle of the same build (the\n"
                    "# signature calls do not touch that path, so its timing stands in for the parent commit's); pairs: PFACX_sigPairsFromDevice over the reduce\n"
                    "# call's list, the passes alone; diy: reduce, the pairs to the host, a numpy masked compare (wall clock).  %d seeded signatures of 16 - 200\n"
                    "# bytes with 0 - 20 %% wildcard bytes, embedded in C3's stream.  Median of %d event-timed calls after warm-up, the better of two interleaved\n"
                    "# rounds.  The last line fits the extra over reduce against the pairs.\n" % (a.sigs, a.steps))
            for ln in lines:
                f.write(ln + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
