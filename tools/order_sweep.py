"""tools/order_sweep.py -- what PFACX_orderHitsFromDevice costs (GPU box only).  Real hit lists -- the class-signature list (id, start, end) and the
edit list (id, start, end, distance) of tests/order_ref.py over 256 KiB of seeded text each, as the device calls return them: in anchor order, with
equal starts and local descents -- repeated with the text's size added to the positions until the list has 10^3, 10^5, 10^6, 10^7 hits.
order: the call over all the list's columns, without and with PFACX_ORDER_TIES_BY_ID.  diy: the do-it-yourself path on the same arrays:
torch.sort(stable=True) of the start column (with ties: of start << 32 | id) plus one index_select per column.  ordered: the call over the list it
has just ordered, the already-ordered exit.  Every timed call starts from a fresh copy of the list (the copy is not timed); HIP events around the
call, the median of --steps calls after warm-up, the better of two interleaved rounds.  The last lines fit order = fixed + per_hit * hits per list
kind and flag.  Every size runs in a child process under a time limit; the first that fails ends the sweep.  One JSON line per size, list and flag.

    python tools/order_sweep.py [--hits 1000,100000,1000000,10000000] [--steps 20] [--out profiles/order_sweep.txt]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = 256 * 1024


def base_lists():
    """-> {"clsig": (start, id, end), "edit": (start, id, end, dist)} as the device calls list them"""
    import numpy as np
    import torch
    from pfac_amd import api
    from tests import cover_ref
    from tests import order_ref as ref

    out = {}
    h = api.PFAC.create()
    try:
        for kind in ("clsig", "edit"):
            text = cover_ref.token_text(7, TEXT) if kind == "clsig" else ref.edit_text(5, TEXT)
            d_in = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to("cuda:0")
            cols = [torch.zeros(TEXT, dtype=torch.int32, device="cuda:0") for _ in range(4)]
            p = [c.data_ptr() for c in cols]
            if kind == "clsig":
                with h.clsigOpenText(b"".join(r + b"\n" for r in ref.CLSIG_RULES)) as sg:
                    _, count = sg.match_device(d_in.data_ptr(), TEXT, p[0], p[1], p[2], TEXT)
                torch.cuda.synchronize()
                out[kind] = tuple(cols[k][:count].cpu().numpy() for k in (1, 0, 2))
            else:
                with h.editOpen(ref.EDIT_PATTERNS, ref.EDIT_BUDGETS) as es:
                    _, count = es.match_device(d_in.data_ptr(), TEXT, p[0], p[1], p[2], p[3], TEXT)
                torch.cuda.synchronize()
                out[kind] = tuple(cols[k][:count].cpu().numpy() for k in (1, 0, 2, 3))
    finally:
        h.destroy()
    return out


def one(hits, steps):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pfac_amd import api, hiprt

    h = api.PFAC.create()
    for kind, base in base_lists().items():
        reps = -(-hits // base[0].size)
        shift = (np.arange(reps, dtype=np.int64) * TEXT).repeat(base[0].size)[:hits]
        cols = []
        for k, c in enumerate(base):
            v = np.tile(c.astype(np.int64), reps)[:hits]
            cols.append((v + shift if k in (0, 2) else v).astype(np.int32))          # start and end move with the text, id and distance do not
        pristine = [torch.from_numpy(c).to("cuda:0") for c in cols]
        work = [torch.empty_like(c) for c in pristine]
        ptr = [w.data_ptr() for w in work] + [None] * (4 - len(work))
        got = {}

        def fresh():
            for w, c in zip(work, pristine):
                w.copy_(c)

        def timed(fn, prepare):
            def once():
                prepare()
                torch.cuda.synchronize()
                a, b = hiprt.Event(), hiprt.Event()
                a.record(0)
                fn()
                b.record(0)
                torch.cuda.synchronize()
                return a.elapsed_ms(b)
            for _ in range(3):
                once()
            return float(np.median([once() for _ in range(steps)]))

        for ties in (False, True):
            flags = api.PFACX_ORDER_TIES_BY_ID if ties else 0

            def order_call():
                got["was"] = h.orderHitsFromDevice(ptr[0], ptr[1], ptr[2], ptr[3], hits, flags)[1]

            def diy_call():
                key = work[0] if not ties else (work[0].to(torch.int64) << 32) | (work[1].to(torch.int64) & 0xFFFFFFFF) ^ 0x80000000
                perm = torch.sort(key, stable=True)[1]
                got["diy"] = [torch.index_select(w, 0, perm) for w in work]

            runs = {"order": [], "diy": [], "ordered": []}
            for _ in range(2):
                runs["order"].append(timed(order_call, fresh))
                was = got["was"]
                ordered = [w.clone() for w in work]
                runs["ordered"].append(timed(order_call, lambda: None))
                assert got["was"] == 1
                runs["diy"].append(timed(diy_call, fresh))
                assert all(torch.equal(a, b) for a, b in zip(ordered, got["diy"])), "the two paths disagree"
            best = {k: min(v) for k, v in runs.items()}
            rec = {"list": kind, "columns": len(work), "hits": hits, "ties": ties, "was_ordered": was}
            for k, v in best.items():
                rec[k + "_ms"] = round(v, 4)
            rec.update({"order_over_diy": round(best["order"] / best["diy"], 3), "order_ns_per_hit": round(best["order"] * 1e6 / hits, 3),
                        "device_scratch_bytes": int(h.info().deviceScratchBytes), "runs_ms": {k: [round(x, 4) for x in v] for k, v in runs.items()}})
            print(json.dumps(rec), flush=True)
    h.destroy()


def fits(lines):
    recs = [json.loads(ln) for ln in lines if '"order_ms"' in ln]
    out = []
    for kind in ("clsig", "edit"):
        for ties in (False, True):
            rs = [r for r in recs if r["list"] == kind and r["ties"] == ties]
            if len(rs) < 2:
                continue
            x, y = [float(r["hits"]) for r in rs], [float(r["order_ms"]) for r in rs]
            mx, my = sum(x) / len(x), sum(y) / len(y)
            sxx = sum((a - mx) ** 2 for a in x)
            slope = sum((a - mx) * (b - my) for a, b in zip(x, y)) / sxx if sxx else 0.0
            out.append({"fit": "order = fixed + per_hit * hits", "list": kind, "ties": ties, "fixed_us": round((my - slope * mx) * 1e3, 2),
                        "per_hit_ns": round(slope * 1e6, 4), "order_over_diy_by_hits": [r["order_over_diy"] for r in rs],
                        "ordered_exit_ms_by_hits": [r["ordered_ms"] for r in rs]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hits", default="1000,100000,1000000,10000000")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per size")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a.one, a.steps)
        return 0
    lines, rc = [], 0
    for item in [s for s in a.hits.split(",") if s]:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", item, "--steps", str(a.steps)], cwd=ROOT, timeout=a.timeout,
                               stdout=subprocess.PIPE)
        except subprocess.TimeoutExpired:
            lines.append(json.dumps({"hits": item, "error": "time limit"}))
            rc = 124
            break
        out = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
        lines.extend(out)
        for ln in out:
            print(ln, flush=True)
        if p.returncode != 0:
            lines.append(json.dumps({"hits": item, "error": "exit %d" % p.returncode}))
            rc = p.returncode if p.returncode > 0 else 1
            break
    for f in fits(lines):
        lines.append(json.dumps(f))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/order_sweep.py: PFACX_orderHitsFromDevice (order) over real class-signature (3 columns) and edit (4 columns) lists repeated to the\n"
                    "# given number of hits, against torch.sort(stable=True) plus one index_select per column on the same arrays (diy); ordered: the call over\n"
                    "# an ordered list (the exit behind the probe).  Median of %d event-timed calls after warm-up, the better of two interleaved rounds; the\n"
                    "# copy that restores the list is not timed.  The last lines fit order = fixed + per_hit * hits.\n" % a.steps)
            for ln in lines:
                f.write(ln + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
