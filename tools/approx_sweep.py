"""tools/approx_sweep.py -- what the approximate calls cost (GPU box only).  Two seeded sets (tests/approx_ref.py: random_patterns, embed):
  text   keywords of 12 - 40 printable bytes with budgets 1 - 2, embedded with exactly k, k + 1 and 0 substitutions in slices of C3's stream
  fixed  the text set again with the NUMBER of embedded occurrences held fixed (4 rounds) whatever the size: in the text runs the embedding
         rounds grow with the bytes up to 256 MiB, so there the pairs and the bytes grow together; here the bytes grow 64 times and the pairs
         do not
  acgt   reads of 100 letters over ACGT with budget 4, embedded the same way in seeded ACGT
PFACX_approxMatchFromDevice (approx) against PFAC_matchFromDeviceReduce (reduce) on the same handle over the same bytes -- the same scan over the
pieces; its code is untouched by the approximate calls, so its timing stands in for the parent commit's.  The passes alone:
PFACX_approxPairsFromDevice over the list the reduce call left (pairs).  The do-it-yourself path (diy): the reduce call, its pairs copied to the
host, then per (pattern, piece) a numpy Hamming distance at the starts its piece's pairs give, over a host copy of the input, and the distinct
(pattern, start) counted (wall clock, the copy of the input not counted).
The device calls are timed alone with HIP events around them; the median of --steps calls after warm-up, the better of two interleaved rounds.  The
expectation the record checks: the extra of approx over reduce follows the candidates (the pairs), not the bytes.  The last line fits
extra = fixed + per_pair * pairs over the text sizes and puts next to it what the fixed runs give: how much the extra grows where only the bytes
grow (fixed: 16 MiB -> 1 GiB) against where the pairs grow with them (text: the same sizes).  The verdict compares those two growths and names
what it rests on; no ratio is set beforehand.
Every run is a child process of its own under a time limit; the first that fails ends the sweep.  One JSON line per run on stdout; with --out the
lines go to that file (profiles/approx_sweep.txt).

    python tools/approx_sweep.py [--runs text:64k,text:16,text:256,text:1024,fixed:16,fixed:256,fixed:1024,acgt:256] [--steps 20] [--patterns 2000] [--out profiles/approx_sweep.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261021
FIXED_ROUNDS = 4                            # the embedding rounds of a `fixed` run, whatever its size


def size_of(item):
    return int(item[:-1]) << 10 if item.endswith("k") else int(item) << 20


def one(run, steps, num_patterns):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pfac_amd import api, hiprt
    from pfac_amd import workloads as wl
    from tests import approx_ref as ref

    kind, item = run.split(":")
    n = size_of(item)
    cfg = wl.make_config("c3")
    if kind in ("text", "fixed"):
        patterns, _ = ref.random_patterns(SEED, ref.PRINTABLE, num_patterns, 12, 40)
        budgets = np.random.default_rng(SEED + 3).integers(1, 3, num_patterns).tolist()
        data, alphabet = np.ascontiguousarray(cfg.input_slice(n, 0)).copy(), ref.PRINTABLE
    else:
        patterns, _ = ref.random_patterns(SEED, ref.ACGT, num_patterns, 100, 100)
        budgets = [4] * num_patterns
        alphabet = ref.ACGT
        data = alphabet[np.random.default_rng(SEED + 2).integers(0, 4, n, dtype=np.uint8)]
    for r in range(FIXED_ROUNDS if kind == "fixed" else min(64, max(1, n >> 22))):
        ref.embed(patterns, budgets, data, alphabet, SEED + 10 * r)
    h = api.PFAC.create()
    h.setPerfMode(cfg.perf_mode)
    ap = h.approxOpen(patterns, budgets)
    piece_off, piece_id, piece_start, _ = ap.pieces()

    d_in = torch.from_numpy(data).to("cuda:0")
    d_a, d_b, d_i, d_p, d_m = (torch.empty(n, dtype=torch.int32, device="cuda:0") for _ in range(5))
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

    def approx_call():
        got["approx"] = ap.match_device(d_in.data_ptr(), n, d_i.data_ptr(), d_p.data_ptr(), d_m.data_ptr(), n)[1]

    def pairs_call():
        got["pairs_listed"] = ap.pairs_device(d_in.data_ptr(), n, d_a.data_ptr(), d_b.data_ptr(), got["pairs"], d_i.data_ptr(), d_p.data_ptr(),
                                              d_m.data_ptr(), n)[1]

    # the (pattern, piece start) entries behind a longest pair of piece q: those of every piece that is a prefix of q's bytes (its chain)
    pieces = ref.model_pieces(patterns, budgets)[1]
    of_piece = {}
    for i in range(1, len(patterns) + 1):
        for e in range(int(piece_off[i]), int(piece_off[i + 1])):
            of_piece.setdefault(int(piece_id[e]), []).append((i, int(piece_start[e])))
    by_prefix = {}
    for r, short in enumerate(pieces, 1):
        by_prefix.setdefault(short, []).extend(of_piece.get(r, ()))
    lengths = sorted({len(p) for p in pieces})
    by_piece = {q: [e for m in lengths if m <= len(long) for e in by_prefix.get(long[:m], ())] for q, long in enumerate(pieces, 1)}
    arrays = [np.frombuffer(p, dtype=np.uint8) for p in patterns]

    def diy_wall_ms():
        t0 = time.perf_counter()
        k = h.matchFromDeviceReduce(d_in.data_ptr(), n, d_a.data_ptr(), d_b.data_ptr())[1]
        ids, pos = d_a[:k].cpu().numpy(), d_b[:k].cpu().numpy().astype(np.int64)
        found = []
        order = np.argsort(ids, kind="stable")
        ids, pos = ids[order], pos[order]
        cuts = np.flatnonzero(np.diff(ids)) + 1
        for q, at in zip(ids[np.concatenate(([0], cuts))].tolist() if k else [], np.split(pos, cuts) if k else []):
            for i, start in by_piece.get(q, ()):
                v = arrays[i - 1]
                s = at - start
                s = s[(s >= 0) & (s + v.size <= n)]
                for c in range(0, s.size, 1 << 16):
                    part = s[c:c + (1 << 16)]
                    d = (data[part[:, None] + np.arange(v.size)[None, :]] != v).sum(axis=1)
                    found.append(part[d <= budgets[i - 1]] + (i << 32))
        got["diy"] = int(np.unique(np.concatenate(found)).size) if found else 0
        return (time.perf_counter() - t0) * 1e3

    calls = {"reduce": reduce_call, "approx": approx_call, "pairs": pairs_call}
    for _ in range(2):                      # interleaved rounds: a drift of the clocks hits every call alike
        for k, fn in calls.items():
            if k == "pairs":
                reduce_call()
            runs.setdefault(k, []).append(median_ms(fn, steps))
    runs["diy"] = [float(np.median([diy_wall_ms() for _ in range(3)]))]
    mis = np.bincount(d_m[:got["approx"]].cpu().numpy(), minlength=5).tolist()
    info = h.info()
    scratch, tables = int(info.deviceScratchBytes), int(info.deviceTableBytes)
    ap.close()
    h.destroy()
    best = {k: min(v) for k, v in runs.items()}
    assert got["pairs_listed"] == got["approx"] == got["diy"], got
    extra = best["approx"] - best["reduce"]
    rec = {"set": kind, "input": "seeded ACGT" if kind == "acgt" else "c3 stream", "size": item, "bytes": n, "patterns": len(patterns),
           "embedding_rounds": FIXED_ROUNDS if kind == "fixed" else min(64, max(1, n >> 22)), "pieces": len(pieces), "pairs": got["pairs"], "listed": got["approx"], "listed_by_distance": mis}
    for k, v in best.items():
        rec[k + "_ms"] = round(v, 4)
    rec.update({"approx_over_reduce": round(best["approx"] / best["reduce"], 4), "extra_over_reduce_ms": round(extra, 4),
                "extra_ns_per_pair": round(extra * 1e6 / got["pairs"], 3) if got["pairs"] else None, "extra_ns_per_byte": round(extra * 1e6 / n, 5),
                "diy_over_approx": round(best["diy"] / best["approx"], 3), "device_scratch_bytes": scratch, "device_table_bytes": tables,
                "runs_ms": {k: [round(x, 4) for x in v] for k, v in runs.items()}})
    print(json.dumps(rec), flush=True)


def fit(lines):
    """extra = fixed + per_pair * pairs over the text sizes, least squares, and the growth of the extra where only the bytes grow (the fixed
    runs) next to its growth where the pairs grow too (the text runs of the same sizes) -> a record, or None with fewer than two text sizes"""
    every = [json.loads(ln) for ln in lines if '"extra_over_reduce_ms"' in ln]
    recs = [r for r in every if r["set"] == "text"]
    if len(recs) < 2:
        return None
    x = [float(r["pairs"]) for r in recs]
    y = [float(r["extra_over_reduce_ms"]) for r in recs]
    mx, my = sum(x) / len(x), sum(y) / len(y)
    sxx = sum((a - mx) ** 2 for a in x)
    slope = sum((a - mx) * (b - my) for a, b in zip(x, y)) / sxx if sxx else 0.0
    fixed = my - slope * mx
    worst = max(abs(b - (fixed + slope * a)) for a, b in zip(x, y))
    out = {"fit": "extra_over_reduce = fixed + per_pair * pairs (text set)", "fixed_us": round(fixed * 1e3, 2), "per_pair_ns": round(slope * 1e6, 3),
           "worst_residual_us": round(worst * 1e3, 2), "extra_ns_per_byte_by_size": [r["extra_ns_per_byte"] for r in recs]}
    held = sorted((r for r in every if r["set"] == "fixed"), key=lambda r: r["bytes"])
    grown = {r["bytes"]: r for r in recs}
    if len(held) >= 2 and held[0]["bytes"] in grown and held[-1]["bytes"] in grown:
        lo, hi = held[0], held[-1]
        bytes_only = hi["extra_over_reduce_ms"] - lo["extra_over_reduce_ms"]
        with_pairs = grown[hi["bytes"]]["extra_over_reduce_ms"] - grown[lo["bytes"]]["extra_over_reduce_ms"]
        out.update({"bytes_grow_pairs_held": {"sizes": [r["size"] for r in held], "pairs": [r["pairs"] for r in held],
                                              "extra_us": [round(r["extra_over_reduce_ms"] * 1e3, 1) for r in held]},
                    "extra_growth_us_bytes_alone": round(bytes_only * 1e3, 1), "extra_growth_us_bytes_and_pairs": round(with_pairs * 1e3, 1),
                    "extra_follows_pairs_not_bytes": {"held": bool(bytes_only < with_pairs),
                                                      "rests_on": "%s -> %s: the growth of the extra with the embedded occurrences held fixed against its "
                                                                  "growth with the occurrences growing too; one set, one round" % (lo["size"], hi["size"])}})
    else:
        out["extra_follows_pairs_not_bytes"] = {"held": None, "rests_on": "no fixed runs: in the text runs pairs and bytes grow together but for the last step"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="text:64k,text:16,text:256,text:1024,fixed:16,fixed:256,fixed:1024,acgt:256", help="set:size; MiB, or KiB with a k")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--patterns", type=int, default=2000)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per run")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a.one, a.steps, a.patterns)
        return 0
    lines = []
    rc = 0
    for item in [s for s in a.runs.split(",") if s]:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", item, "--steps", str(a.steps), "--patterns", str(a.patterns)],
                               cwd=ROOT, timeout=a.timeout, stdout=subprocess.PIPE)
        except subprocess.TimeoutExpired:
            lines.append(json.dumps({"run": item, "error": "time limit"}))
            rc = 124
            break
        out = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
        lines.extend(out)
        for ln in out:
            print(ln, flush=True)
        if p.returncode != 0:
            lines.append(json.dumps({"run": item, "error": "exit %d" % p.returncode}))
            rc = p.returncode if p.returncode > 0 else 1
            break
    fitted = fit(lines)
    if fitted:
        lines.append(json.dumps(fitted))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/approx_sweep.py: PFACX_approxMatchFromDevice (approx) against PFAC_matchFromDeviceReduce (reduce) on the same handle of the same build\n"
                    "# (the approximate calls do not touch that path, so its timing stands in for the parent commit's); pairs: PFACX_approxPairsFromDevice over the\n"
                    "# reduce call's list, the passes alone; diy: reduce, the pairs to the host, a numpy Hamming distance at the candidates (wall clock).  text: %d\n"
                    "# seeded keywords of 12 - 40 bytes with budgets 1 - 2 embedded in C3's stream, the rounds of embedding growing with the size; fixed: the same with 4\n"
                    "# rounds at every size; acgt: as many reads of 100 letters with budget 4 in seeded ACGT.\n"
                    "# Median of %d event-timed calls after warm-up, the better of two interleaved rounds.  The last line fits the extra over reduce against the pairs.\n"
                    % (a.patterns, a.steps))
            for ln in lines:
                f.write(ln + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
