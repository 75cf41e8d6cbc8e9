"""tools/ruleseq_sweep.py -- what ordered rule members (PFACX_rulesOpenSeq) cost a rules call (GPU box only).  C3's set (30 000
Snort-style patterns, hashed) over its HTTP stream, the seeded rule file of tools/rules_sweep.py (10 000 rules of 1 to 4 patterns), 16 MiB cut into
segments of 1.5 KiB and 64 KiB, the rules opened in three forms:

    seq      as they are, through PFACX_rulesOpenSeq: no member is relative, so the set is the conditioned set PFACX_rulesOpenEx makes of the same
             members and launches its kernels.  With --parent-lib DIR (libpfac.so and libpfac_gfx950.so built from the parent commit) that call runs
             in the parent's build twice (`parent`, `parent2`): `seq` is expected inside the spread of those two rounds
    chain    every second member of a rule {PFACX_RULE_RELATIVE, distance 0, within 0}: "somewhere behind the member in front"
    chain64  the same with within 64

Every call is synchronous and timed alone with HIP events around it; the median of --steps calls after 2 warm-ups is reported with the fastest and
the slowest.  `candidates` is the number of (segment, rule) pairs the two passes verify -- the entries of the `seq` list whose rule has a chain in
the chained forms --, `fired` what is left of them and of the rules without a chain.  Every (shape, mode) runs in a child process of its own under a
time limit; the first that fails ends the sweep.  One JSON line per shape on stdout; with --out the lines go to that file
(profiles/ruleseq_sweep.txt).

    python tools/ruleseq_sweep.py [--shapes 16777216:1536,16777216:65536] [--steps 11] [--parent-lib DIR] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
SHAPES = "16777216:1536,16777216:65536"


def one(mode, n, seg, steps):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import rules_sweep
    from pfac_amd import api, hiprt
    from pfac_amd import workloads as wl

    cfg = wl.make_config("c3")
    pf = wl.write_pattern_file(os.path.join(tempfile.mkdtemp(), "c3.pat"), cfg.patterns)
    h = api.PFAC.create()
    h.setPerfMode(cfg.perf_mode)
    h.readPatternFromFile(pf)
    F = int(h.info().numOfPatterns)
    segs = n // seg
    n = segs * seg
    data = cfg.input_slice(max(n, 4096), 0)[:n]
    d_in = torch.from_numpy(np.ascontiguousarray(data)).to("cuda:0")
    d_off = torch.from_numpy((np.arange(segs + 1, dtype=np.int64) * seg)).to("cuda:0")
    rule_off, rule_pats = rules_sweep.make_rules(F)
    plain = rules_sweep.make_members(rule_off, rule_pats, False)
    result = {}

    def fired_list(r):
        _, total = r.match_device(d_in.data_ptr(), n, d_off.data_ptr(), segs, None, None, 0, None, check=False)
        d_seg = torch.empty(max(1, total), dtype=torch.int32, device="cuda:0")
        d_rule = torch.empty(max(1, total), dtype=torch.int32, device="cuda:0")
        d_first = torch.empty(segs + 1, dtype=torch.int64, device="cuda:0")
        return total, d_seg, d_rule, d_first

    if mode in ("parent", "parent2"):
        r = h.rulesOpenEx(rule_off, plain)
    else:
        members = np.zeros(plain.size, dtype=api.rule_seq_member_dtype())
        for name in ("pattern", "flags", "offset", "depth"):
            members[name] = plain[name]
        if mode != "seq":
            index_in_rule = np.arange(plain.size) - np.repeat(rule_off[:-1], np.diff(rule_off))
            second = index_in_rule % 2 == 1
            members["flags"][second] |= api.PFACX_RULE_RELATIVE
            members["within"][second] = 64 if mode == "chain64" else 0
            base = h.rulesOpenSeq(rule_off, _without_relative(members))
            total, d_seg, d_rule, d_first = fired_list(base)
            base.match_device(d_in.data_ptr(), n, d_off.data_ptr(), segs, d_seg.data_ptr(), d_rule.data_ptr(), total, d_first.data_ptr())
            torch.cuda.synchronize()
            chained = torch.from_numpy(np.diff(rule_off) >= 2).to("cuda:0")
            result["candidates"] = int(chained[d_rule[:total].long()].sum().item())
            base.close()
        r = h.rulesOpenSeq(rule_off, members)
    fired, d_seg, d_rule, d_first = fired_list(r)

    def call():
        result["fired"] = r.match_device(d_in.data_ptr(), n, d_off.data_ptr(), segs, d_seg.data_ptr(), d_rule.data_ptr(), fired, d_first.data_ptr())[1]

    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(steps):
        a, b = hiprt.Event(), hiprt.Event()
        t0 = time.perf_counter()
        a.record(0)
        call()
        b.record(0)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6)
        ev.append(a.elapsed_ms(b) * 1e3)
    h.destroy()
    ev = np.array(ev)
    print(json.dumps({"mode": mode, "bytes": n, "segment": seg, "segments": segs, **result,
                      "event_us": round(float(np.median(ev)), 2), "event_us_min": round(float(ev.min()), 2), "event_us_max": round(float(ev.max()), 2),
                      "wall_us": round(float(np.median(wall)), 2)}), flush=True)


def _without_relative(members):
    """the members with the flag, distance and within taken off again: the set whose fired list is the candidates"""
    from pfac_amd import api
    base = members.copy()
    base["flags"] &= 0xFFFFFFFF ^ api.PFACX_RULE_RELATIVE
    base["distance"] = 0
    base["within"] = 0
    return base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="bytes:segment, comma separated")
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--parent-lib", default="", help="directory with the parent commit's libpfac.so and libpfac_gfx950.so")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        mode, n, seg = a.one.split(":")
        one(mode, int(n), int(seg), a.steps)
        return 0
    lines = []
    rc = 0
    for shape in a.shapes.split(","):
        row = {"shape": shape}
        for mode in ["seq"] + (["parent", "parent2"] if a.parent_lib else []) + ["chain", "chain64"]:
            env = dict(os.environ)
            if mode.startswith("parent"):
                env["PFAC_HOST_LIB"] = os.path.join(os.path.abspath(a.parent_lib), "libpfac.so")
                env["PFAC_AB_OLD_LIBS"] = "1"
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", f"{mode}:{shape}", "--steps", str(a.steps)],
                                   cwd=ROOT, env=env, timeout=a.timeout, stdout=subprocess.PIPE)
            except subprocess.TimeoutExpired:
                row["error"] = f"{mode}: time limit"
                rc = 124
                break
            out = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not out:
                row["error"] = f"{mode}: exit {p.returncode}"
                rc = p.returncode if p.returncode > 0 else 1
                break
            r = json.loads(out[-1])
            row[mode + "_us"] = r["event_us"]
            row[mode + "_us_range"] = [r["event_us_min"], r["event_us_max"]]
            row["segments"] = r["segments"]
            for k in ("fired", "candidates"):
                if k in r:
                    row[mode + "_" + k] = r[k]
        for mode in ("chain", "chain64"):
            if "seq_us" in row and mode + "_us" in row:
                row[mode + "_over_seq"] = round(row[mode + "_us"] / row["seq_us"], 3)
        if "seq_us" in row and "parent_us" in row and "parent2_us" in row:
            row["seq_over_parent"] = round(row["seq_us"] / row["parent_us"], 3)
            row["parent2_over_parent"] = round(row["parent2_us"] / row["parent_us"], 3)
        ln = json.dumps(row)
        lines.append(ln)
        print(ln, flush=True)
        if rc:
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/ruleseq_sweep.py: PFACX_rulesMatchFromDevice per batch of a set opened by PFACX_rulesOpenSeq; C3 set and stream, the 10 000 seeded\n"
                    "# rules of tools/rules_sweep.py; microseconds, median of %d event-timed calls after 2 warm-ups, *_us_range = fastest and slowest of them.\n"
                    "# seq: no relative member (the kernels of PFACX_rulesOpenEx); parent, parent2: PFACX_rulesOpenEx over the same members in the parent commit's\n"
                    "# build, two rounds -- parent2_over_parent is its run-to-run spread, seq_over_parent what is compared with it; chain: every second member\n"
                    "# {RELATIVE, distance 0, within 0}; chain64: within 64; *_candidates = the (segment, rule) pairs verified, *_over_seq = the cost as a multiple\n"
                    "# of the plain-member form\n" % a.steps)
            for ln in lines:
                f.write(ln + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
