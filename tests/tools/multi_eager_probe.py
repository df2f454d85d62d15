#!/usr/bin/env python3
"""tests/tools/multi_eager_probe.py -- what eager-output sets cost and save on the many-DFA front (run on the GPU box):

  corpus   the 22 automata of tests/golden/eager with their own lines: one fsm_hip_exec_batch_eager_offsets call per automaton
           (fsm_hip_dfa_create included, as a driver that builds a DFA per record pays it) against ONE fsm_hip_exec_multi_eager
  bulk     K jobs on the eager40 table (354 states x 27 classes: the LDS form) x NL lines of 64 B, prepared: the launch with
           and without eager_out, taken in turns
  single   the yardstick for the bulk ratio: the same table's own fronts on one batch, fsm_hip_exec_batch_eager_offsets_device
           against fsm_hip_exec_batch_offsets_device, in the same run

Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(torch, fns, reps):
    """ms per call of each fn, the fns taken in turns (one device, one clock): median and spread over reps"""
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for _ in fns]
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    for r in range(reps):
        for k, fn in enumerate(fns):
            ev[k][r][0].record()
            fn()
            ev[k][r][1].record()
    torch.cuda.synchronize()
    ms = [[a.elapsed_time(b) for a, b in row] for row in ev]
    return [{"median_ms": round(float(np.median(m)), 4), "min_ms": round(min(m), 4), "max_ms": round(max(m), 4)} for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--nl", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import libfsm_amd as hip
    from common import GOLDEN, Golden, eager_golden_paths
    res = {}

    # ---- the reference's eager corpus: one automaton at a time against one submission
    gs = [Golden(p) for p in eager_golden_paths()]
    packed = [g.packed() for g in gs]

    def one_by_one():
        for g, (base, off) in zip(gs, packed):
            d = hip.HipDfa(g.flat)
            d.exec_offsets_eager(base, off)
            d.close()

    def multi():
        ds = [hip.HipDfa(g.flat, hip.DEFER_UPLOAD) for g in gs]
        hip.exec_multi_eager(ds, [g.strings() for g in gs], 1)
        for d in ds:
            d.close()
    t = {}
    for name, fn in (("one_by_one", one_by_one), ("multi", multi)):
        fn()
        ts = []
        for _ in range(10):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        t[name] = ts
    res["corpus"] = {"dfas": len(gs), "lines": sum(len(o) - 1 for _, o in packed), "launches_multi": hip.multi_last_launches(),
                     "ms_one_by_one": round(float(np.median(t["one_by_one"])), 3), "ms_multi": round(float(np.median(t["multi"])), 3),
                     "speedup": round(float(np.median(t["one_by_one"]) / np.median(t["multi"])), 1),
                     "note": "wall time of a pass over the 22 records, fsm_hip_dfa_create included; median of 10"}

    # ---- bulk: K eager40 jobs x NL lines of 64 B, prepared, with and without eager_out
    z = np.load(os.path.join(GOLDEN, "bench", "eager40.npz"))
    flat, pats = hip.FlatDfa.load(z), bytes(z["patterns"]).split(b"\n")
    K, nl, ll = a.k, a.nl, 64
    stream = torch.cuda.current_stream().cuda_stream
    text = torch.empty(K * nl * ll + 16, dtype=torch.uint8, device="cuda")
    hip.gen_inputs_device(text.data_ptr(), K * nl, ll, 0, 0x40, b"abcdefghijklmnopqrstuvwxyz", pats[0], 5)
    off = torch.arange(nl + 1, device="cuda", dtype=torch.int64) * ll
    ends = torch.empty(K * nl, dtype=torch.int32, device="cuda")
    sets = torch.empty(K * nl, dtype=torch.int64, device="cuda")
    ds = [hip.HipDfa(flat, hip.DEFER_UPLOAD) for _ in range(K)]
    plain = [(text.data_ptr() + q * nl * ll, off.data_ptr(), nl, ends.data_ptr() + q * nl * 4, 0, 0) for q in range(K)]
    eager = [j + (sets.data_ptr() + q * nl * 8,) for q, j in enumerate(plain)]
    pp, pe = hip.MultiPrepared(ds, plain, 1), hip.MultiPrepared(ds, eager, 1)
    pe.launch(stream)
    torch.cuda.synchronize()
    launches, fused = hip.multi_last_launches(), hip.multi_last_fused_jobs()
    hits = int((sets[:nl] != 0).sum())
    tp, te = timed(torch, [lambda: pp.launch(stream), lambda: pe.launch(stream)], a.reps)
    pp.close()
    pe.close()
    for d in ds:
        d.close()
    res["bulk"] = {"jobs": K, "lines_per_job": nl, "line_bytes": ll, "launches": launches, "fused_jobs": fused,
                   "lines_with_outputs_in_job_0": hits, "plain": tp, "eager": te,
                   "eager_over_plain": round(te["median_ms"] / tp["median_ms"], 4),
                   "walked_GBps_plain": round(K * nl * ll / tp["median_ms"] / 1e6, 1), "walked_GBps_eager": round(K * nl * ll / te["median_ms"] / 1e6, 1)}

    # ---- the yardstick: the table's own fronts over the same lines as ONE batch (as many as 2^31 offsets allow)
    n1 = min(K * nl, 20_000_000)
    off1 = torch.arange(n1 + 1, device="cuda", dtype=torch.int64) * ll
    one = hip.HipDfa(flat)
    sp, se = timed(torch, [lambda: one.exec_batch_offsets_device(text.data_ptr(), off1.data_ptr(), n1, ends.data_ptr(), 0, stream=stream),
                           lambda: one.exec_offsets_device_front("eager", text.data_ptr(), off1.data_ptr(), n1, ends.data_ptr(), sets.data_ptr(), stream=stream)], a.reps)
    res["single"] = {"lines": n1, "layout": one.info()["layout_name"], "plain": sp, "eager": se, "eager_over_plain": round(se["median_ms"] / sp["median_ms"], 4),
                     "walked_GBps_plain": round(n1 * ll / sp["median_ms"] / 1e6, 1), "walked_GBps_eager": round(n1 * ll / se["median_ms"] / 1e6, 1)}
    one.close()
    out = json.dumps(res)
    print(out, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
