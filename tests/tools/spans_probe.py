#!/usr/bin/env python3
"""tests/tools/spans_probe.py -- what the accept-position walk costs beside the end-state walk it is modelled on, on one device:
TEXT_BYTES (default 1 GiB) of 8-64-byte lines and of 0-1024-byte lines (text_probe.py's texts), the automaton
tests/test_gpu_spans.py calls lds_full (affine, 1 023 states x 16 classes: the largest LDS image):

 (a) every line walked forward by walk_pos (fsm_hip_exec_accept_pos_device, first and last asked for), HIP events;
 (b) the SAME lines and automaton through one-job fsm_hip_exec_multi_device (end states), in a process of its own that loads
     PARENT_LIB (default: this tree's library -- multi.hip and the walk kernels are not touched by the positions), the two
     sides taking turns three times; whether the job rode the fused walk_multi launch (fused_jobs) or went to its dfa's own
     kernel (its name) is recorded with the time, which includes the submission's descriptor copy;
 (c) one round of spans (fsm_hip_text_hits_spans: two walks, one close) at one hit in 1 000, by fsm_hip_text_spans_ms.
The expectation to judge (NOTES.md): the chain gains an `and` and a shift-or per byte on an LDS-latency-bound walk, so (a) / (b)
should be near 1.  Best of three after a warm-up.

usage: spans_probe.py [out.json]   (default: profiles/spans_probe.json)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

TEXTS = {"8_64": (8, 64, 5), "0_1024": (0, 1024, 6)}


def setup(which, size):
    import torch
    import libfsm_amd as hip
    from global_ref import affine
    from text_probe import make_text
    torch.cuda.set_device(0)
    lo, hi, seed = TEXTS[which]
    text = make_text(torch, size, lo, hi, seed)
    torch.cuda.synchronize()
    t = hip.HipText(d_text=text.data_ptr(), nbytes=size, delim=0x0A)
    return torch, hip, text, t, affine(1023, 16)[0]


def timed(torch, fn, reps=4):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms[1:])


def multi_side(which, size):
    """the child: the end-state walk of the same lines by the library this process loaded"""
    torch, hip, text, t, flat = setup(which, size)
    dfa = hip.HipDfa(flat)
    end = torch.empty(t.lines, dtype=torch.int32, device="cuda")
    ms = timed(torch, lambda: hip.exec_multi_device([dfa], [(text.data_ptr(), t.d_off, t.lines, end.data_ptr(), 0)]))
    print(json.dumps({"ms": ms, "kernel": dfa.last_kernel_name(), "fused_jobs": hip.multi_last_fused_jobs()}))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--multi-side":
        if os.environ.get("PARENT_LIB"):
            import libfsm_amd.capi as capi
            capi._lib = capi.load_library(os.environ["PARENT_LIB"])      # every binding of this process goes to that library
        return multi_side(sys.argv[2], int(sys.argv[3]))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "spans_probe.json")
    size = int(os.environ.get("TEXT_BYTES", 1 << 30))
    res = {"bytes": size, "parent_lib": os.environ.get("PARENT_LIB", "this tree's"), "texts": {}}
    for which in TEXTS:
        torch, hip, text, t, flat = setup(which, size)
        res["device"] = torch.cuda.get_device_name(0)
        n = t.lines
        pd = hip.PosDfa.from_flat(flat)
        first = torch.empty(n, dtype=torch.int64, device="cuda")
        last = torch.empty(n, dtype=torch.int64, device="cuda")
        pos, multi, kernel = [], [], None
        for _ in range(3):                                     # the two sides take turns
            pos.append(timed(torch, lambda: pd.accept_pos_device(text.data_ptr(), t.d_off, n, first.data_ptr(), last.data_ptr(), limit=size)))
            r = json.loads(subprocess.run([sys.executable, os.path.abspath(__file__), "--multi-side", which, str(size)], check=True,
                                          capture_output=True, text=True, timeout=600).stdout.strip().split("\n")[-1])
            multi.append(r["ms"])
            kernel = (r["kernel"], r["fused_jobs"])
        # one round of spans at one hit in 1 000: the two images are the same automaton (the cost, not the answer, is the point)
        from hits_probe import pack
        g = torch.Generator(device="cuda")
        g.manual_seed(29)
        bm = pack(torch, torch.randint(0, 1000, (n,), device="cuda", generator=g) == 0)
        hits = t.hits_device(bm.data_ptr(), want_bytes=False)
        rounds = []
        for _ in range(4):
            sp = hip.HipSpans(hits, pd, pd)
            rounds.append(sp.ms())
            sp.close()
        res["texts"][which] = {"lines": n, "walk_pos_ms": round(min(pos), 4), "end_state_walk_ms": round(min(multi), 4),
                               "end_state_kernel": kernel[0], "end_state_fused_jobs": kernel[1], "ratio": round(min(pos) / min(multi), 3),
                               "hits": hits.count, "spans_round_ms": round(min(rounds[1:]), 4)}
        print(which, res["texts"][which], flush=True)
        hits.close()
        pd.close()
        t.close()
        del text, first, last, bm
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
