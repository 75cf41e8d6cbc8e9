"""tools/case_sweep.py -- what the case calls cost (GPU box only).  PFACX_caseMatchFromDevice, the list (case) and PFACX_CASE_ALL (case_all), against
PFAC_matchFromDeviceReduce (reduce) and PFACX_matchAllFromDevice (all) on the same caseless handle over the same bytes -- they run the same scan:
C3's set with every second line marked sensitive and its letters case-flipped at random, over C3's stream with a quarter of its letters flipped.
The passes alone: PFACX_casePairsFromDevice over the list the reduce call left (pairs, pairs_all; also as pairs per second).  The same passes with
no sensitive line (nosens_pairs_all: a second case object, all flags 0) next to PFACX_wordsPairsFromDevice with PFACX_WORDS_ALL under the empty
class over the same list (words_pairs_all): the expectation is that they cost the same.  The do-it-yourself path (diy): a caseless handle of the
caseless lines and a plain handle of the sensitive lines, one PFAC_matchFromDeviceReduce each, then the merge of the two lists in torch (concatenate,
sort by position -- it cannot give "the longest per position" where the longest sits in the other list, and is timed as the lower bound it is).
All calls are timed alone with HIP events around them; the median of --steps calls after warm-up, the better of two interleaved rounds.  The
expectation the record checks: the extra of case_all over all follows the pairs and the compared bytes, not the input size (extra_ns_per_pair next
to extra_ns_per_byte over the sizes).
Every size runs in a child process of its own under a time limit; the first that fails ends the sweep.  One JSON line per size on stdout; with --out
the lines go to that file (profiles/case_sweep.txt).

    python tools/case_sweep.py [--sizes 64k,16,256,1024] [--steps 20] [--out profiles/case_sweep.txt]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def size_of(item):
    return int(item[:-1]) << 10 if item.endswith("k") else int(item) << 20


def flip_case(p, rng):
    out = bytearray(p)
    for i, c in enumerate(out):
        if 0x41 <= c <= 0x5A or 0x61 <= c <= 0x7A:
            out[i] = (c & ~0x20) if rng.integers(0, 2) else (c | 0x20)
    return bytes(out)


def one(item, steps):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pfac_amd import api, hiprt
    from pfac_amd import workloads as wl

    n = size_of(item)
    rng = np.random.Generator(np.random.PCG64(55))
    cfg = wl.make_config("c3")
    pats = [flip_case(p, rng) for p in cfg.patterns]
    sens = np.zeros(len(pats) + 1, dtype=np.uint8)
    sens[2::2] = 1                                                      # every second line
    text = b"".join(p + b"\n" for p in pats)
    h = api.PFAC.create()
    h.setPerfMode(cfg.perf_mode)
    h.readPatternFromMemoryEx(text, api.PFACX_READ_NOCASE)
    cs = h.caseOpen(text, sens)
    nosens = h.caseOpen(text, np.zeros(len(pats) + 1, dtype=np.uint8))
    # the do-it-yourself pair of handles
    hc, hs = api.PFAC.create(), api.PFAC.create()
    for x in (hc, hs):
        x.setPerfMode(cfg.perf_mode)
    hc.readPatternFromMemoryEx(b"".join(p + b"\n" for k, p in enumerate(pats, 1) if not sens[k]), api.PFACX_READ_NOCASE)
    hs.readPatternFromMemoryEx(b"".join(p + b"\n" for k, p in enumerate(pats, 1) if sens[k]), 0)

    d_in = torch.from_numpy(np.ascontiguousarray(cfg.input_slice(n, 0))).to("cuda:0")
    letter = ((d_in >= 0x41) & (d_in <= 0x5A)) | ((d_in >= 0x61) & (d_in <= 0x7A))
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(55)
    d_in ^= (letter & (torch.randint(0, 4, d_in.shape, dtype=torch.uint8, device="cuda:0", generator=gen) == 0)).to(torch.uint8) * 0x20
    del letter
    most = max(1, cs.max_matches_per_position)
    cap = n * most if n * most <= (1 << 29) else n                      # 8 bytes per entry of the capacity; a longer list is counted, not written
    d_a, d_b, d_c, d_d = (torch.empty(n, dtype=torch.int32, device="cuda:0") for _ in range(4))
    d_i, d_p = (torch.empty(cap, dtype=torch.int32, device="cuda:0") for _ in range(2))
    empty = api.word_class(b"")
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
        got["all"] = h.matchAllFromDevice(d_in.data_ptr(), n, d_i.data_ptr(), d_p.data_ptr(), cap, check=False)[1]

    def case_call():
        got["case"] = cs.match_device(d_in.data_ptr(), n, 0, d_i.data_ptr(), d_p.data_ptr(), cap)[1]

    def case_all_call():
        got["case_all"] = cs.match_device(d_in.data_ptr(), n, api.PFACX_CASE_ALL, d_i.data_ptr(), d_p.data_ptr(), cap)[1]

    def pairs_of(obj, flags, key):
        def call():
            got[key] = obj.pairs_device(d_in.data_ptr(), n, flags, d_a.data_ptr(), d_b.data_ptr(), got["pairs"], d_i.data_ptr(), d_p.data_ptr(), cap)[1]
        return call

    def words_pairs_all_call():
        got["words_pairs_all"] = h.wordsPairsFromDevice(d_in.data_ptr(), n, empty, api.PFACX_WORDS_ALL, d_a.data_ptr(), d_b.data_ptr(), got["pairs"],
                                                        d_i.data_ptr(), d_p.data_ptr(), cap, check=False)[1]

    def diy_call():
        k1 = hc.matchFromDeviceReduce(d_in.data_ptr(), n, d_c.data_ptr(), d_d.data_ptr())[1]
        k2 = hs.matchFromDeviceReduce(d_in.data_ptr(), n, d_i.data_ptr(), d_p.data_ptr())[1]
        pos = torch.cat((d_d[:k1], d_p[:k2]))
        ids = torch.cat((d_c[:k1], d_i[:k2]))
        order = torch.argsort(pos, stable=True)
        merged_pos, merged_ids = pos[order], ids[order]
        got["diy"] = int(merged_pos.numel())
        assert merged_ids.numel() == got["diy"]

    calls = {"reduce": reduce_call, "all": all_call, "case": case_call, "case_all": case_all_call,
             # the list the reduce call left in d_a / d_b
             "pairs": pairs_of(cs, 0, "pairs_listed"), "pairs_all": pairs_of(cs, api.PFACX_CASE_ALL, "pairs_all_listed"),
             "nosens_pairs_all": pairs_of(nosens, api.PFACX_CASE_ALL, "nosens_listed"), "words_pairs_all": words_pairs_all_call, "diy": diy_call}
    for _ in range(2):                      # interleaved rounds: a drift of the clocks hits every call alike
        for k, fn in calls.items():
            if k == "pairs":
                reduce_call()
            runs.setdefault(k, []).append(median_ms(fn))
    info = h.info()
    scratch, tables = int(info.deviceScratchBytes), int(info.deviceTableBytes)
    for x in (h, hc, hs):
        x.destroy()
    best = {k: min(v) for k, v in runs.items()}
    pairs = got["pairs"]
    assert got["pairs_listed"] == got["case"] and got["pairs_all_listed"] == got["case_all"], got
    assert got["nosens_listed"] == got["words_pairs_all"] == got["all"], got
    rec = {"input": "c3, every second line sensitive", "size": item, "bytes": n, "patterns": len(pats), "max_per_position": most, "pairs": pairs,
           "all_listed": got["all"], "case_listed": got["case"], "case_all_listed": got["case_all"], "diy_listed": got["diy"]}
    for k, v in best.items():
        rec[k + "_ms"] = round(v, 4)
    extra = best["case_all"] - best["all"]
    rec.update({"case_over_reduce": round(best["case"] / best["reduce"], 4), "case_all_over_all": round(best["case_all"] / best["all"], 4),
                "extra_over_all_ms": round(extra, 4), "extra_ns_per_pair": round(extra * 1e6 / pairs, 3) if pairs else None,
                "extra_ns_per_byte": round(extra * 1e6 / n, 4),
                "passes_Mpairs_per_s": round(pairs / best["pairs_all"] / 1e3, 1) if pairs else None,
                "nosens_over_words_pairs_all": round(best["nosens_pairs_all"] / best["words_pairs_all"], 4),
                "diy_over_case": round(best["diy"] / best["case"], 4)})
    rec["device_scratch_bytes"] = scratch
    rec["device_table_bytes"] = tables
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
            f.write("# tools/case_sweep.py: PFACX_caseMatchFromDevice (case: the list; case_all: PFACX_CASE_ALL) against PFAC_matchFromDeviceReduce (reduce) and\n"
                    "# PFACX_matchAllFromDevice (all) on the same caseless handle of the same build (this change does not touch those paths, so their timing stands\n"
                    "# in for the parent commit's); pairs / pairs_all: PFACX_casePairsFromDevice over the reduce call's list, the passes alone; nosens_pairs_all: the\n"
                    "# same with no sensitive line, next to words_pairs_all: PFACX_wordsPairsFromDevice, PFACX_WORDS_ALL, the empty class; diy: a caseless handle of\n"
                    "# the caseless lines + a plain handle of the sensitive lines + a torch merge.  C3's set, every second line sensitive, letters case-flipped at\n"
                    "# random, over its stream with a quarter of its letters flipped.  Median of %d event-timed calls after warm-up, the better of two interleaved rounds.\n" % a.steps)
            for ln in lines:
                f.write(ln + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
