"""tools/nocase_sweep.py -- what a caseless pattern set (PFACX_READ_NOCASE) costs (GPU box only).

A caseless handle over the raw stream is timed against a plain handle loaded from the folded set over the pre-folded stream (folded
here with torch, not by the library): both compute the same result -- checked -- so the difference is the fold alone.  C3's set with its
patterns' letters case-flipped at random, over C3's HTTP stream with a quarter of its letters flipped.
  fold        PFACX_foldInput alone, 1 GiB into handle-sized scratch (aligned source, and a source one byte off: the funnelled path);
              TB/s of bytes read + written
  full        PFAC_matchFromDevice, 1 GiB
  compacted   PFAC_matchFromDeviceReduce, 1 GiB
  host        PFAC_matchFromHost from pinned buffers and PFAC_matchFromHostReduce, 256 MiB (wall clock)
  small       PFAC_matchFromDevice, 64 KiB: microseconds added
Each figure is the median of 2 x --steps calls in two interleaved rounds (plain, caseless, plain, caseless), after warm-up.  One JSON
line per case on stdout; with --out they go to that file too (profiles/nocase_sweep.txt).

    python tools/nocase_sweep.py [--cases fold,full,compacted,host,small] [--steps 10] [--out profiles/nocase_sweep.txt]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TARGETS = {"fold": ">= 5.0 TB/s", "full": "<= 1.45x", "compacted": "<= 1.6x", "host_pinned": "<= 1.05x", "host_reduce": "<= 1.05x",
           "small": "<= 10 us added"}


def flip_case(p, rng):
    out = bytearray(p)
    for i, c in enumerate(out):
        if 0x41 <= c <= 0x5A or 0x61 <= c <= 0x7A:
            out[i] = (c & ~0x20) if rng.integers(0, 2) else (c | 0x20)
    return bytes(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="fold,full,compacted,host,small")
    ap.add_argument("--steps", type=int, default=10, help="calls per side and round (two rounds)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    cases = a.cases.split(",")

    import numpy as np
    import torch
    from pfac_amd import api, hiprt
    from pfac_amd import workloads as wl

    torch.cuda.set_device(0)
    rng = np.random.Generator(np.random.PCG64(55))
    cfg = wl.make_config("c3")
    pats = [flip_case(p, rng) for p in cfg.patterns]
    folded_pats = list(dict.fromkeys(p.lower() for p in pats))
    tmp = tempfile.mkdtemp()
    pf = os.path.join(tmp, "c3_mixed.pat")
    with open(pf, "wb") as f:
        f.write(b"".join(p + b"\n" for p in pats))
    ff = os.path.join(tmp, "c3_folded.pat")
    with open(ff, "wb") as f:                          # the folded set, duplicates kept: pattern IDs are those of the caseless set
        f.write(b"".join(p.lower() + b"\n" for p in pats))

    def handles():
        hc, hp = api.PFAC.create(), api.PFAC.create()
        for h in (hc, hp):
            h.setPerfMode(cfg.perf_mode)
        hc.readPatternFromFileEx(pf, api.PFACX_READ_NOCASE)
        hp.readPatternFromFile(ff)
        return hc, hp

    def mixed_stream(n):
        d = torch.from_numpy(np.ascontiguousarray(cfg.input_slice(n, 0))).to("cuda:0")
        letter = ((d >= 0x41) & (d <= 0x5A)) | ((d >= 0x61) & (d <= 0x7A))
        flip = letter & (torch.randint(0, 4, d.shape, dtype=torch.uint8, device="cuda:0") == 0)
        d ^= flip.to(torch.uint8) * 0x20
        del letter, flip
        f = torch.where((d >= 0x41) & (d <= 0x5A), d + 32, d)
        torch.cuda.synchronize()
        return d, f

    def ev_ms(fn):
        e0, e1 = hiprt.Event(), hiprt.Event()
        e0.record(0)
        fn()
        e1.record(0)
        torch.cuda.synchronize()
        return e0.elapsed_ms(e1)

    def wall_ms(fn):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def interleaved(plain_fn, nocase_fn, clock=ev_ms):
        for fn in (plain_fn, nocase_fn):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        tp, tc = [], []
        for _ in range(2):
            tp += [clock(plain_fn) for _ in range(a.steps)]
            tc += [clock(nocase_fn) for _ in range(a.steps)]
        return float(np.median(tp)), float(np.median(tc))

    lines = []

    def emit(d):
        d["target"] = TARGETS.get(d["case"], "")
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    n = 1 << 30
    if "fold" in cases or "full" in cases or "compacted" in cases:
        d_raw, d_fold = mixed_stream(n)
        hc, hp = handles()
        if "fold" in cases:
            mod = C.CDLL(api.library_paths()[1])
            mod.PFACX_foldInput.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
            mod.PFACX_foldInput.restype = C.c_int
            dst = torch.empty(n + 256, dtype=torch.uint8, device="cuda:0")
            for off in (0, 1):
                m = n - off
                assert mod.PFACX_foldInput(hc._h, d_raw.data_ptr() + off, dst.data_ptr(), m) == 0
                torch.cuda.synchronize()
                assert torch.equal(dst[:m], d_fold[off:off + m])
                t = []
                for _ in range(3):
                    mod.PFACX_foldInput(hc._h, d_raw.data_ptr() + off, dst.data_ptr(), m)
                for _ in range(2 * a.steps):
                    t.append(ev_ms(lambda: mod.PFACX_foldInput(hc._h, d_raw.data_ptr() + off, dst.data_ptr(), m)))
                ms = float(np.median(t))
                emit({"case": "fold", "source_offset": off, "bytes": m, "ms": round(ms, 4), "tb_per_s_read_write": round(2 * m / ms / 1e9, 3)})
            del dst
        if "full" in cases:
            out_p = torch.empty(n, dtype=torch.int32, device="cuda:0")
            out_c = torch.empty(n, dtype=torch.int32, device="cuda:0")
            hp.matchFromDevice(d_fold.data_ptr(), n, out_p.data_ptr())
            hc.matchFromDevice(d_raw.data_ptr(), n, out_c.data_ptr())
            torch.cuda.synchronize()
            assert torch.equal(out_p, out_c), "caseless != plain on the folded stream"
            matches = int(torch.count_nonzero(out_p))
            tp, tc = interleaved(lambda: hp.matchFromDevice(d_fold.data_ptr(), n, out_p.data_ptr()),
                                 lambda: hc.matchFromDevice(d_raw.data_ptr(), n, out_c.data_ptr()))
            emit({"case": "full", "bytes": n, "matches": matches, "plain_ms": round(tp, 4), "nocase_ms": round(tc, 4), "ratio": round(tc / tp, 4)})
            del out_p, out_c
        if "compacted" in cases:
            ids_p = torch.empty(n, dtype=torch.int32, device="cuda:0")
            pos_p = torch.empty(n, dtype=torch.int32, device="cuda:0")
            ids_c = torch.empty(n, dtype=torch.int32, device="cuda:0")
            pos_c = torch.empty(n, dtype=torch.int32, device="cuda:0")
            _, kp = hp.matchFromDeviceReduce(d_fold.data_ptr(), n, ids_p.data_ptr(), pos_p.data_ptr())
            _, kc = hc.matchFromDeviceReduce(d_raw.data_ptr(), n, ids_c.data_ptr(), pos_c.data_ptr())
            assert kp == kc and torch.equal(ids_p[:kp], ids_c[:kc]) and torch.equal(pos_p[:kp], pos_c[:kc])
            tp, tc = interleaved(lambda: hp.matchFromDeviceReduce(d_fold.data_ptr(), n, ids_p.data_ptr(), pos_p.data_ptr()),
                                 lambda: hc.matchFromDeviceReduce(d_raw.data_ptr(), n, ids_c.data_ptr(), pos_c.data_ptr()))
            emit({"case": "compacted", "bytes": n, "pairs": kp, "plain_ms": round(tp, 4), "nocase_ms": round(tc, 4), "ratio": round(tc / tp, 4)})
            del ids_p, pos_p, ids_c, pos_c
        hc.destroy()
        hp.destroy()
        del d_raw, d_fold
        torch.cuda.empty_cache()

    if "host" in cases:
        m = 256 << 20
        d_raw, d_fold = mixed_stream(m)
        h_raw, h_fold = d_raw.cpu().pin_memory(), d_fold.cpu().pin_memory()
        del d_raw, d_fold
        hc, hp = handles()
        out_p = torch.empty(m, dtype=torch.int32).pin_memory()
        out_c = torch.empty(m, dtype=torch.int32).pin_memory()
        hp.matchFromHost(h_fold.data_ptr(), m, out_p.data_ptr())
        hc.matchFromHost(h_raw.data_ptr(), m, out_c.data_ptr())
        assert torch.equal(out_p, out_c)
        tp, tc = interleaved(lambda: hp.matchFromHost(h_fold.data_ptr(), m, out_p.data_ptr()),
                             lambda: hc.matchFromHost(h_raw.data_ptr(), m, out_c.data_ptr()), wall_ms)
        emit({"case": "host_pinned", "bytes": m, "plain_ms": round(tp, 4), "nocase_ms": round(tc, 4), "ratio": round(tc / tp, 4)})
        ids_p, pos_p = torch.empty(m, dtype=torch.int32).pin_memory(), torch.empty(m, dtype=torch.int32).pin_memory()
        ids_c, pos_c = torch.empty(m, dtype=torch.int32).pin_memory(), torch.empty(m, dtype=torch.int32).pin_memory()
        _, kp = hp.matchFromHostReduce(h_fold.data_ptr(), m, ids_p.data_ptr(), pos_p.data_ptr())
        _, kc = hc.matchFromHostReduce(h_raw.data_ptr(), m, ids_c.data_ptr(), pos_c.data_ptr())
        assert kp == kc and torch.equal(ids_p[:kp], ids_c[:kc]) and torch.equal(pos_p[:kp], pos_c[:kc])
        tp, tc = interleaved(lambda: hp.matchFromHostReduce(h_fold.data_ptr(), m, ids_p.data_ptr(), pos_p.data_ptr()),
                             lambda: hc.matchFromHostReduce(h_raw.data_ptr(), m, ids_c.data_ptr(), pos_c.data_ptr()), wall_ms)
        emit({"case": "host_reduce", "bytes": m, "pairs": kp, "plain_ms": round(tp, 4), "nocase_ms": round(tc, 4), "ratio": round(tc / tp, 4)})
        hc.destroy()
        hp.destroy()

    if "small" in cases:
        m = 64 << 10
        d_raw, d_fold = mixed_stream(m)
        hc, hp = handles()
        out_p = torch.empty(m, dtype=torch.int32, device="cuda:0")
        out_c = torch.empty(m, dtype=torch.int32, device="cuda:0")
        hp.matchFromDevice(d_fold.data_ptr(), m, out_p.data_ptr())
        hc.matchFromDevice(d_raw.data_ptr(), m, out_c.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(out_p, out_c)
        tp, tc = interleaved(lambda: hp.matchFromDevice(d_fold.data_ptr(), m, out_p.data_ptr()),
                             lambda: hc.matchFromDevice(d_raw.data_ptr(), m, out_c.data_ptr()))
        emit({"case": "small", "bytes": m, "plain_us": round(tp * 1e3, 2), "nocase_us": round(tc * 1e3, 2), "added_us": round((tc - tp) * 1e3, 2)})
        hc.destroy()
        hp.destroy()

    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/nocase_sweep.py: a caseless handle (PFACX_READ_NOCASE) on the raw stream against a plain handle loaded from the folded\n"
                    "# set on the pre-folded stream (identical results, checked); C3's %d patterns case-flipped (%d distinct when folded),\n"
                    "# its stream with a quarter of its letters flipped.  Median of 2 x %d calls in two interleaved rounds.\n"
                    % (len(pats), len(folded_pats), a.steps))
            for ln in lines:
                f.write(ln + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
