"""tools/rules_sweep.py -- what a rules call (PFACX_rulesMatchFromDevice) costs against (a) PFACX_matchAllBatchFromDevice over the same buffer
and offsets -- the raw material a user has without it -- and (b) the do-it-yourself path in torch behind that call: expand the all-match list
through the inverted rule index, sort and reduce by (segment, rule) (GPU box only).  C3's set (30 000 Snort-style patterns, hashed) over its HTTP
stream; a seeded synthetic rule file of 10 000 rules of 1 to 4 patterns drawn from the set; buffers of 16 MiB and 256 MiB cut into segments of
1.5 KiB and 64 KiB.  Every call is synchronous and timed alone with HIP events around it; the median of --steps calls after 2 warm-ups is reported
with the fastest and the slowest.  With --parent-lib DIR (libpfac.so and libpfac_gfx950.so built from the parent commit) (a) and the call inside
(b) run in the parent's build, as the baseline.  Every (shape, mode) runs in a child process of its own under a time limit; the first that fails
ends the sweep.  One JSON line per shape on stdout; with --out the lines go to that file (profiles/rules_sweep.txt).  `memberships` is the number
of (pair on a prefix chain, rule that names its pattern) steps the pass takes per call: the design claim is that the extra over (a) follows it.

Conditioned sets (PFACX_rulesOpenEx), with --cond: the same rules opened three more ways -- `cond0`: every member {id, 0, 0, 0}, so
the fired list is that of `rules` and the difference is what the window test costs (one position and one length load per chain member, 8 bytes per
membership); `condw`: seeded windows, a fifth of the members negated; and, with --parent-lib, `rules` again in the parent commit's build, twice
(`parent`, `parent2`): plain sets launch the instantiation they always have, so `rules` is expected inside the spread of those two rounds.

    python tools/rules_sweep.py [--shapes 16777216:1536,...] [--steps 11] [--parent-lib DIR] [--cond] [--modes rules,cond0,...] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = "16777216:1536,16777216:65536,268435456:1536,268435456:65536"
NUM_RULES, SEED = 10000, 20261018


def make_rules(num_patterns):
    """(rule_off, rule_patterns): NUM_RULES rules of 1 - 4 distinct pattern ids, seeded"""
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(SEED))
    rules = [sorted({int(i) for i in rng.integers(1, num_patterns + 1, size=int(rng.integers(1, 5)))}) for _ in range(NUM_RULES)]
    off = np.zeros(NUM_RULES + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in rules])
    return off, np.array([i for r in rules for i in r], dtype=np.int32)


def make_members(rule_off, rule_pats, windows):
    """the rules of make_rules as PFACX_rule_member_t; windows: a seeded window per member -- a quarter from the end, offset 0 .. 255, depth 0 for
    half of them, else 64 .. 1023 -- and a fifth of the members negated (never a rule's first)"""
    import numpy as np
    from pfac_amd import api
    members = np.zeros(rule_pats.size, dtype=api.rule_member_dtype())
    members["pattern"] = rule_pats
    if windows:
        rng = np.random.Generator(np.random.PCG64(SEED + 1))
        k = rule_pats.size
        first = np.zeros(k, dtype=bool)
        first[rule_off[:-1]] = True
        members["flags"] = np.where((rng.integers(0, 5, size=k) == 0) & ~first, api.PFACX_RULE_NOT, 0) | \
            np.where(rng.integers(0, 4, size=k) == 0, api.PFACX_RULE_FROM_END, 0)
        members["offset"] = rng.integers(0, 256, size=k)
        members["depth"] = np.where(rng.integers(0, 2, size=k) == 0, 0, rng.integers(64, 1024, size=k))
    return members


def one(mode, n, seg, steps):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pfac_amd import api, hiprt
    from pfac_amd import workloads as wl

    cfg = wl.make_config("c3")
    pf = wl.write_pattern_file(os.path.join(tempfile.mkdtemp(), "c3.pat"), cfg.patterns)
    h = api.PFAC.create()
    h.setPerfMode(cfg.perf_mode)
    h.readPatternFromFile(pf)
    info = h.info()
    F = int(info.numOfPatterns)
    segs = n // seg
    n = segs * seg
    data = cfg.input_slice(max(n, 4096), 0)[:n]
    d_in = torch.from_numpy(np.ascontiguousarray(data)).to("cuda:0")
    d_off = torch.from_numpy((np.arange(segs + 1, dtype=np.int64) * seg)).to("cuda:0")
    rule_off, rule_pats = make_rules(F)
    result = {}

    # the inverted index, by the ids the library reports (duplicate lines: the highest id)
    by_bytes = {}
    for i, p in enumerate(cfg.patterns):
        by_bytes[bytes(p)] = i + 1
    resolved = np.array([by_bytes[bytes(cfg.patterns[i - 1])] for i in rule_pats], dtype=np.int64)
    rule_of = np.repeat(np.arange(NUM_RULES, dtype=np.int64), np.diff(rule_off))
    bit_of = np.arange(rule_pats.size, dtype=np.int64) - rule_off[:-1][rule_of]
    order = np.lexsort((rule_of, resolved))
    member = torch.from_numpy((rule_of[order] << 5 | bit_of[order])).to("cuda:0")
    member_off = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(resolved, minlength=F + 1))]).astype(np.int64)).to("cuda:0")
    need = torch.from_numpy(((1 << np.diff(rule_off).astype(np.int64)) - 1)).to("cuda:0")

    if mode in ("rules", "parent", "parent2", "cond0", "condw"):
        r = h.rulesOpenEx(rule_off, make_members(rule_off, rule_pats, mode == "condw")) if mode.startswith("cond") else h.rulesOpen(rule_off, rule_pats)
        _, fired = r.match_device(d_in.data_ptr(), n, d_off.data_ptr(), segs, None, None, 0, None, check=False)
        d_seg = torch.empty(max(1, fired), dtype=torch.int32, device="cuda:0")
        d_rule = torch.empty(max(1, fired), dtype=torch.int32, device="cuda:0")
        d_first = torch.empty(segs + 1, dtype=torch.int64, device="cuda:0")

        def call():
            result["fired"] = r.match_device(d_in.data_ptr(), n, d_off.data_ptr(), segs, d_seg.data_ptr(), d_rule.data_ptr(), fired, d_first.data_ptr())[1]
    else:
        cap = n * max(1, int(info.maxMatchesPerPosition))
        d_ids = torch.empty(cap, dtype=torch.int32, device="cuda:0")
        d_pos = torch.empty(cap, dtype=torch.int32, device="cuda:0")
        d_first = torch.empty(segs + 1, dtype=torch.int64, device="cuda:0")

        def all_batch():
            result["pairs"] = h.matchAllBatchFromDevice(d_in.data_ptr(), n, d_off.data_ptr(), segs, d_ids.data_ptr(), d_pos.data_ptr(), cap, d_first.data_ptr())[1]

        def diy():
            all_batch()
            p = result["pairs"]
            ids = d_ids[:p].long()
            seg_of = torch.searchsorted(d_first[1:], torch.arange(p, device="cuda:0"), right=True)
            cnt = member_off[ids + 1] - member_off[ids]
            which = torch.repeat_interleave(torch.arange(p, device="cuda:0"), cnt)
            inside = torch.arange(which.numel(), device="cuda:0") - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
            m = member[member_off[ids[which]] + inside]
            key = torch.unique(seg_of[which] * (NUM_RULES << 5) + m)                  # (segment, rule, bit) once each, sorted
            pair, inverse = torch.unique_consecutive(key >> 5, return_inverse=True)
            mask = torch.zeros(pair.numel(), dtype=torch.int64, device="cuda:0").scatter_add_(0, inverse, 1 << (key & 31))
            fired = pair[mask == need[pair % NUM_RULES]]
            result["fired"] = int(fired.numel())
            result["memberships"] = int(which.numel())

        call = all_batch if mode == "allbatch" else diy

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="bytes:segment, comma separated")
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--parent-lib", default="", help="directory with the parent commit's libpfac.so and libpfac_gfx950.so")
    ap.add_argument("--cond", action="store_true", help="also the conditioned sets (and, with --parent-lib, the plain call in the parent's build)")
    ap.add_argument("--modes", default="", help="comma separated, instead of the default list")
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
        modes = ["rules", "allbatch", "diy"]
        if a.cond:
            modes = ["rules", "cond0", "condw"] + (["parent", "parent2"] if a.parent_lib else []) + modes[1:]
        for mode in (a.modes.split(",") if a.modes else modes):
            env = dict(os.environ)
            if a.parent_lib and mode not in ("rules", "cond0", "condw"):
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
            row[mode + "_wall_us"] = r["wall_us"]
            row["segments"] = r["segments"]
            for k in ("fired", "pairs", "memberships"):
                if k in r:
                    row[mode + "_" + k] = r[k]
        if "rules_us" in row and "allbatch_us" in row:
            row["rules_over_allbatch"] = round(row["rules_us"] / row["allbatch_us"], 3)
            row["extra_us"] = round(row["rules_us"] - row["allbatch_us"], 2)
        if "rules_us" in row and "diy_us" in row:
            row["diy_over_rules"] = round(row["diy_us"] / row["rules_us"], 2)
        for mode in ("cond0", "condw"):
            if "rules_us" in row and mode + "_us" in row:
                row[mode + "_over_rules"] = round(row[mode + "_us"] / row["rules_us"], 3)
        if "rules_us" in row and "parent_us" in row and "parent2_us" in row:
            row["rules_over_parent"] = round(row["rules_us"] / row["parent_us"], 3)
            row["parent2_over_parent"] = round(row["parent2_us"] / row["parent_us"], 3)
        ln = json.dumps(row)
        lines.append(ln)
        print(ln, flush=True)
        if rc:
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/rules_sweep.py: PFACX_rulesMatchFromDevice per batch against (a) PFACX_matchAllBatchFromDevice over the same buffer and offsets\n"
                    "# (allbatch) and (b) that call plus the expansion through the inverted index, a sort and a reduce by (segment, rule) in torch (diy); C3 set\n"
                    "# and stream, %d seeded rules of 1 - 4 patterns; microseconds, median of %d event-timed calls after 2 warm-ups, *_us_range = fastest and\n"
                    "# slowest of them, *_wall_us = the host's clock; allbatch and diy %s\n"
                    % (NUM_RULES, a.steps, "in the parent commit's build" if a.parent_lib else "in this build"))
            if a.cond:
                f.write("# cond0: the same rules through PFACX_rulesOpenEx, every member {id, 0, 0, 0} (the same fired list); condw: seeded windows, a fifth of the\n"
                        "# members negated; parent, parent2: the plain call in the parent commit's build, two rounds\n")
            for ln in lines:
                f.write(ln + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
