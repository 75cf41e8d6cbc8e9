"""tools/flowrules_sweep.py -- what a flow-rules call (PFACX_flowRulesPairsFromDevice) costs next to the PFACX_flowsMatchFromDevice call that
produced its pairs (GPU box only).  C3's set (30 000 Snort-style patterns, hashed) over its HTTP stream; one batch of --pieces
pieces of --piece-bytes bytes, every piece the first of a flow of its own; 10 000 seeded rules of two distinct patterns each.  Both calls are
synchronous and timed alone with HIP events around them: the median of --steps calls after 2 warm-ups, with the fastest and the slowest.  The
flow set and the flow-rule set are reset in front of every call, outside the timed region, so every call does the same work (and the rules call
runs all three of its passes: the list always fits).  One JSON line on stdout.

    python tools/flowrules_sweep.py [--pieces 4096] [--piece-bytes 1400] [--steps 11]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_RULES, SEED = 10000, 20261020


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pieces", type=int, default=4096)
    ap.add_argument("--piece-bytes", type=int, default=1400)
    ap.add_argument("--steps", type=int, default=11)
    a = ap.parse_args()
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
    F, M = int(info.numOfPatterns), int(info.maxPatternLen)
    P, n = a.pieces, a.pieces * a.piece_bytes
    d_in = torch.from_numpy(np.ascontiguousarray(cfg.input_slice(max(n, 4096), 0)[:n])).to("cuda:0")
    offsets = np.arange(P + 1, dtype=np.uintp) * a.piece_bytes
    flow_ids = np.arange(P, dtype=np.uint32)
    piece_offs = np.zeros(P, dtype=np.uint64)
    cap = n + P * (M - 1)
    d_ids = torch.empty(cap, dtype=torch.int32, device="cuda:0")
    d_pos = torch.empty(cap, dtype=torch.int32, device="cuda:0")
    d_first = torch.empty(P + 1, dtype=torch.int32, device="cuda:0")
    rng = np.random.Generator(np.random.PCG64(SEED))
    one = rng.integers(0, F, size=NUM_RULES)
    two = (one + rng.integers(1, F, size=NUM_RULES)) % F                    # another pattern
    rules = np.sort(np.stack([one, two], axis=1).astype(np.int32) + 1, axis=1)
    flows = h.flowsOpen(P)
    fr = h.flowRulesOpen(np.arange(NUM_RULES + 1, dtype=np.int32) * 2, rules.reshape(-1), P)
    result = {}

    def flows_call():
        result["pairs"] = flows.match_device(d_in.data_ptr(), n, offsets.ctypes.data, flow_ids.ctypes.data, P, d_ids.data_ptr(), d_pos.data_ptr(), cap,
                                             d_first.data_ptr(), piece_offs.ctypes.data)[1]

    flows_call()
    fired = fr.pairs_device(d_ids.data_ptr(), result["pairs"], d_first.data_ptr(), flow_ids.ctypes.data, P, None, None, 0, None)[1]
    d_piece = torch.empty(max(1, fired), dtype=torch.int32, device="cuda:0")
    d_rule = torch.empty(max(1, fired), dtype=torch.int32, device="cuda:0")
    d_ff = torch.empty(P + 1, dtype=torch.int64, device="cuda:0")

    def rules_call():
        result["fired"] = fr.pairs_device(d_ids.data_ptr(), result["pairs"], d_first.data_ptr(), flow_ids.ctypes.data, P, d_piece.data_ptr(),
                                          d_rule.data_ptr(), max(1, fired), d_ff.data_ptr())[1]

    def timed(call, reset):
        ev = []
        for k in range(a.steps + 2):
            reset()
            torch.cuda.synchronize()
            x, y = hiprt.Event(), hiprt.Event()
            x.record(0)
            call()
            y.record(0)
            torch.cuda.synchronize()
            if k >= 2:
                ev.append(x.elapsed_ms(y) * 1e3)
        ev = np.array(ev)
        return round(float(np.median(ev)), 2), [round(float(ev.min()), 2), round(float(ev.max()), 2)]

    flows_us, flows_range = timed(flows_call, flows.reset)
    rules_us, rules_range = timed(rules_call, fr.reset)
    fr.close()
    flows.close()
    h.destroy()
    print(json.dumps({"pieces": P, "piece_bytes": a.piece_bytes, "bytes": n, "patterns": F, "rules": NUM_RULES, **result,
                      "flows_us": flows_us, "flows_us_range": flows_range, "flowrules_us": rules_us, "flowrules_us_range": rules_range,
                      "flowrules_over_flows": round(rules_us / flows_us, 3)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
