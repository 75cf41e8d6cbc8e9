"""tools/gapsig_sweep.py -- what the gapped-signature calls cost (GPU box only).  A seeded set of gapped signatures (tests/gapsig_ref.py:
random_signatures; 2 - 4 parts, gaps up to 16 wide) over C3's stream with embeddings, decoys and near misses at seeded places.
PFACX_gapsigMatchFromDevice (gapsig) against
  reduce   PFAC_matchFromDeviceReduce on the same handle over the same bytes -- the same scan over the anchors; its code is untouched by the
           gapped-signature calls, so its timing stands in for the parent commit's
  sig      PFACX_sigMatchFromDevice over the same set with every gap fixed at lo and written as ?? bytes, on a handle of its own over the same
           bytes, next to the reduce call of THAT handle (sig_reduce: its anchors are not the same -- a run may cross a gap {0}): the extra of
           gapsig over its reduce less the extra of sig over its reduce is the price of the search over the widths
and the passes alone: PFACX_gapsigPairsFromDevice over the list the reduce call left (pairs).
The device calls are timed alone with HIP events around them; the median of --steps calls after warm-up, the better of two interleaved rounds.
The last line fits extra = fixed + per_pair * pairs over the sizes and says whether the extra follows the pairs rather than the bytes.
Every size runs in a child process of its own under a time limit; the first that fails ends the sweep.  One JSON line per size on stdout; with
--out the lines go to that file (profiles/gapsig_sweep.txt).

    python tools/gapsig_sweep.py [--sizes 64k,16,256,1024] [--steps 20] [--sigs 2000] [--out profiles/gapsig_sweep.txt]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261022


def size_of(item):
    return int(item[:-1]) << 10 if item.endswith("k") else int(item) << 20


def fixed_gaps(sigs):
    """every gap at lo, written as wildcard bytes: one (values, masks) per signature, as PFACX_sigOpen takes them"""
    import numpy as np
    out = []
    for parts, gaps in sigs:
        values, masks = [], []
        for j, (v, m) in enumerate(parts):
            values.append(np.asarray(v, dtype=np.uint8))
            masks.append(np.asarray(m, dtype=np.uint8))
            if j < len(gaps):
                values.append(np.zeros(gaps[j][0], dtype=np.uint8))
                masks.append(np.zeros(gaps[j][0], dtype=np.uint8))
        out.append((np.concatenate(values), np.concatenate(masks)))
    return out


def one(item, steps, num_sigs):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pfac_amd import api, hiprt
    from pfac_amd import workloads as wl
    from tests import gapsig_ref as ref
    from tests import sig_ref

    n = size_of(item)
    cfg = wl.make_config("c3")
    sigs = ref.random_signatures(SEED, num_sigs, max_parts=4, max_gap=16, min_parts=2)
    data = np.ascontiguousarray(cfg.input_slice(n, 0)).copy()
    ref.embed(sigs, data, SEED, per_sig=min(64, max(2, n >> 22)), near_misses=min(16, max(1, n >> 24)))
    h = api.PFAC.create()
    h.setPerfMode(cfg.perf_mode)
    gs = h.gapsigOpen(*ref.csr_of(sigs))
    h2 = api.PFAC.create()
    h2.setPerfMode(cfg.perf_mode)
    sg = h2.sigOpen(*sig_ref.csr_of(fixed_gaps(sigs)))

    d_in = torch.from_numpy(data).to("cuda:0")
    d_a, d_b, d_i, d_p, d_e = (torch.empty(n, dtype=torch.int32, device="cuda:0") for _ in range(5))
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

    def gapsig_call():
        got["gapsig"] = gs.match_device(d_in.data_ptr(), n, d_i.data_ptr(), d_p.data_ptr(), d_e.data_ptr(), n)[1]

    def pairs_call():
        got["pairs_listed"] = gs.pairs_device(d_in.data_ptr(), n, d_a.data_ptr(), d_b.data_ptr(), got["pairs"], d_i.data_ptr(), d_p.data_ptr(),
                                              d_e.data_ptr(), n)[1]

    def sig_reduce_call():
        got["sig_pairs"] = h2.matchFromDeviceReduce(d_in.data_ptr(), n, d_a.data_ptr(), d_b.data_ptr())[1]

    def sig_call():
        got["sig"] = sg.match_device(d_in.data_ptr(), n, d_i.data_ptr(), d_p.data_ptr(), n)[1]

    calls = {"reduce": reduce_call, "gapsig": gapsig_call, "pairs": pairs_call, "sig_reduce": sig_reduce_call, "sig": sig_call}
    for _ in range(2):                      # interleaved rounds: a drift of the clocks hits every call alike
        for k, fn in calls.items():
            if k == "pairs":
                reduce_call()
            runs.setdefault(k, []).append(median_ms(fn, steps))
    info = h.info()
    scratch, tables = int(info.deviceScratchBytes), int(info.deviceTableBytes)
    anchors, sig_anchors = int(gs.anchors()[0].max()), int(sg.anchors()[0].max())
    gs.close()
    sg.close()
    h.destroy()
    h2.destroy()
    best = {k: min(v) for k, v in runs.items()}
    assert got["pairs_listed"] == got["gapsig"], got
    extra, sig_extra = best["gapsig"] - best["reduce"], best["sig"] - best["sig_reduce"]
    rec = {"input": "c3 stream, seeded gapped signatures embedded", "size": item, "bytes": n, "signatures": len(sigs), "anchors": anchors,
           "pairs": got["pairs"], "listed": got["gapsig"], "sig_anchors": sig_anchors, "sig_pairs": got["sig_pairs"], "sig_listed": got["sig"]}
    for k, v in best.items():
        rec[k + "_ms"] = round(v, 4)
    rec.update({"gapsig_over_reduce": round(best["gapsig"] / best["reduce"], 4), "extra_over_reduce_ms": round(extra, 4),
                "extra_ns_per_pair": round(extra * 1e6 / got["pairs"], 3) if got["pairs"] else None, "extra_ns_per_byte": round(extra * 1e6 / n, 5),
                "sig_extra_over_its_reduce_ms": round(sig_extra, 4), "search_price_ms": round(extra - sig_extra, 4),
                "device_scratch_bytes": scratch, "device_table_bytes": tables,
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
            f.write("# tools/gapsig_sweep.py: PFACX_gapsigMatchFromDevice (gapsig) against PFAC_matchFromDeviceReduce (reduce) on the same handle of the same\n"
                    "# build (the gapped-signature calls do not touch that path, so its timing stands in for the parent commit's); pairs:\n"
                    "# PFACX_gapsigPairsFromDevice over the reduce call's list, the passes alone; sig / sig_reduce: PFACX_sigMatchFromDevice over the same set\n"
                    "# with every gap fixed at lo and written as ?? bytes, and the reduce call of that handle; search_price = (gapsig - reduce) - (sig -\n"
                    "# sig_reduce).  %d seeded signatures of 2 - 4 parts, gaps up to 16 wide, embedded in C3's stream.  Median of %d event-timed calls\n"
                    "# after warm-up, the better of two interleaved rounds.  The last line fits the extra over reduce against the pairs.\n" % (a.sigs, a.steps))
            for ln in lines:
                f.write(ln + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
