"""tools/host_frames_sweep.py -- what the host forms that share the list frame of pfac_host.h (sortedSegmentLists, touchedRuleMasks) cost, this
build against another one: CPU only, host-only handles on PFAC_PLATFORM_CPU, one thread.

Rows, each where the post-pass is not hidden behind the scan:
  flowrules           PFACX_flowRulesPairsFromHost over a seeded pair list of 2^20 pairs in 4096 pieces, 64 patterns in prefix chains of 4, 512
                      rules of 1 - 4 patterns; capacity 0, so every call is truncated, commits nothing and does the same work again: pure post-pass
  rules, rules-cond   PFACX_rulesMatchFromHost over the nested set a, aa, ..., 8 a's and 4 MiB of `a` in segments of 64 bytes: 8 rules {a .. k a's},
                      plain (PFACX_rulesOpen) and with a window on every member (PFACX_rulesOpenEx, offset 1, every other one from the end)
  countbatch,         PFACX_countBatchFromHost over the same set and buffer, without and with PFACX_COUNT_LONGEST
  countbatch-longest
The rules and count-batch calls get arrays that hold their whole list.  A row is timed in a process of its own: the median of --steps calls after 3
warm-ups, milliseconds of wall time, with the fastest and the slowest.  With --parent-lib DIR (a libpfac.so built from the parent commit, loaded
through PFAC_HOST_LIB) every row runs new, parent, parent, and gets the verdict of the earlier refactor sweeps: ok when the new median lies
inside the parent's fastest-to-slowest range, or differs from a parent median by no more than the two parent medians differ, or is faster.

    python tools/host_frames_sweep.py [--rows flowrules,rules,...] [--steps 11] [--parent-lib DIR] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ["flowrules", "rules", "rules-cond", "countbatch", "countbatch-longest"]
SEED = 20261020


def one(row, steps):
    sys.path.insert(0, ROOT)
    import numpy as np
    from pfac_amd import api

    h = api.PFAC.createHostOnly()
    h.setPlatform(api.PFAC_PLATFORM_CPU)
    rng = np.random.Generator(np.random.PCG64(SEED))
    result = {}
    if row == "flowrules":
        pats = [bytes([65 + k]) * d for k in range(16) for d in (2, 4, 6, 8)]                # 16 chains of 4: the longest pair stands for 4 patterns
        h.readPatternFromMemory(b"".join(p + b"\n" for p in pats))
        rules = [sorted({int(i) for i in rng.integers(1, len(pats) + 1, size=int(rng.integers(1, 5)))}) for _ in range(512)]
        off = np.zeros(len(rules) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(r) for r in rules])
        pieces, pairs = 4096, 1 << 20
        fl = h.flowRulesOpen(off, np.array([i for r in rules for i in r], dtype=np.int32), pieces)
        ids = rng.integers(1, len(pats) + 1, size=pairs).astype(np.int32)
        first = (np.arange(pieces + 1, dtype=np.int64) * (pairs // pieces)).astype(np.int32)
        flows = rng.permutation(pieces).astype(np.uint32)
        fired_first = np.zeros(pieces + 1, dtype=np.uintp)

        def call():
            result["entries"] = fl.pairs_host(ids.ctypes.data, pairs, first.ctypes.data, flows.ctypes.data, pieces, None, None, 0, fired_first.ctypes.data,
                                              check=False)[1]
    else:
        h.readPatternFromMemory(b"".join(b"a" * k + b"\n" for k in range(1, 9)))
        n, seg = 4 << 20, 64
        segs = n // seg
        data = np.full(n, ord("a"), dtype=np.uint8)
        offsets = (np.arange(segs + 1, dtype=np.int64) * seg).astype(np.uintp)
        seg_first = np.zeros(segs + 1, dtype=np.uintp)
        if row.startswith("rules"):
            rule_off = np.zeros(9, dtype=np.int32)
            rule_off[1:] = np.cumsum(np.arange(1, 9))
            rule_pats = np.array([i for k in range(1, 9) for i in range(1, k + 1)], dtype=np.int32)
            if row == "rules-cond":
                members = np.zeros(rule_pats.size, dtype=api.rule_member_dtype())
                members["pattern"], members["offset"] = rule_pats, 1
                members["flags"] = np.where(np.arange(rule_pats.size) % 2 == 1, api.PFACX_RULE_FROM_END, 0)
                r = h.rulesOpenEx(rule_off, members)
            else:
                r = h.rulesOpen(rule_off, rule_pats)
            capacity = segs * 8
            out_a, out_b = np.zeros(capacity, dtype=np.int32), np.zeros(capacity, dtype=np.int32)

            def call():
                result["entries"] = r.match_host(data.ctypes.data, n, offsets.ctypes.data, segs, out_a.ctypes.data, out_b.ctypes.data, capacity,
                                                 seg_first.ctypes.data)[1]
        else:
            flags = api.PFACX_COUNT_LONGEST if row == "countbatch-longest" else 0
            capacity = segs * 8
            out_a, out_b = np.zeros(capacity, dtype=np.int32), np.zeros(capacity, dtype=np.uint32)

            def call():
                result["entries"] = h.countBatchFromHost(data.ctypes.data, n, offsets.ctypes.data, segs, flags, out_a.ctypes.data, out_b.ctypes.data, capacity,
                                                         seg_first.ctypes.data)[1]
    for _ in range(3):
        call()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    h.destroy()
    print(json.dumps({"row": row, **result, "ms": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per child")
    ap.add_argument("--parent-lib", default="", help="directory with the parent commit's libpfac.so")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a.one, a.steps)
        return 0
    lines = ["%-20s %10s %22s %22s %10s  %s" % ("row", "new", "parent 1 (min .. max)", "parent 2 (min .. max)", "entries", "verdict")]
    outside = 0
    for row in a.rows.split(","):
        got = []
        for build in ["new"] + (["parent", "parent"] if a.parent_lib else []):
            env = dict(os.environ, OMP_NUM_THREADS="1")
            if build == "parent":
                env["PFAC_HOST_LIB"] = os.path.join(os.path.abspath(a.parent_lib), "libpfac.so")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", row, "--steps", str(a.steps)], cwd=ROOT, env=env,
                               timeout=a.timeout, stdout=subprocess.PIPE)
            out = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not out:
                print(f"{row}/{build}: exit {p.returncode}", file=sys.stderr)
                return p.returncode if p.returncode > 0 else 1
            got.append(json.loads(out[-1]))
        new = got[0]
        if len(got) == 3:
            p1, p2 = got[1], got[2]
            assert new["entries"] == p1["entries"] == p2["entries"], (row, new, p1, p2)
            lo, hi = min(p1["ms_min"], p2["ms_min"]), max(p1["ms_max"], p2["ms_max"])
            spread = abs(p1["ms"] - p2["ms"])
            ok = lo <= new["ms"] <= hi or min(abs(new["ms"] - p1["ms"]), abs(new["ms"] - p2["ms"])) <= spread or new["ms"] < min(p1["ms"], p2["ms"])
            outside += not ok
            lines.append("%-20s %10.3f %22s %22s %10d  %s" % (row, new["ms"], "%.3f (%.3f .. %.3f)" % (p1["ms"], p1["ms_min"], p1["ms_max"]),
                                                             "%.3f (%.3f .. %.3f)" % (p2["ms"], p2["ms_min"], p2["ms_max"]), new["entries"],
                                                             "ok" if ok else "OUTSIDE"))
        else:
            lines.append("%-20s %10.3f %22s %22s %10d" % (row, new["ms"], "-", "-", new["entries"]))
        print(lines[-1], flush=True)
    lines.append(f"# outside: {outside}")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
