#!/usr/bin/env python3
"""tests/tools/context_probe.py -- what context lines cost beside the select, on one device: TEXT_BYTES (default 1 GiB) of
8-64-byte lines (text_probe.py's text), one line in 1000 selected, contexts (0, 0), (2, 2) and (1000, 1000):

 (a) fsm_hip_text_hits_context_ms (the widening and the marks: five kernels, HIP events) beside the select's own time from the SAME
     handle (fsm_hip_text_hits_ms minus fsm_hip_text_hits_gather_ms), and the gather's;
 (b) the plain hits of fsm_hip_text_hits_device on the same bitmap: its select and its gather.
The expectation to judge (NOTES.md): the added passes move n / 8 bytes each against the select's 8 n bytes of offsets, so (a)'s first
figure should stay below its second, and should not move with the context.  Best of three after a warm-up, the sides interleaved.
Small runs (TEXT_BYTES <= 64 MiB) double as a check against tests/context_ref.py.

usage: context_probe.py [out.json]   (default: profiles/context_probe.json)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))


def main():
    import torch
    import libfsm_amd as hip
    from context_ref import context_witness, marks_ref
    from hits_probe import pack
    from text_probe import make_text
    hip.load_library()
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "context_probe.json")
    size = int(os.environ.get("TEXT_BYTES", 1 << 30))
    torch.cuda.set_device(0)
    text = make_text(torch, size, 8, 64, 5)
    torch.cuda.synchronize()
    t = hip.HipText(d_text=text.data_ptr(), nbytes=size, delim=0x0A)
    n = t.lines
    g = torch.Generator(device="cuda")
    g.manual_seed(23)
    bits = torch.randint(0, 1000, (n,), device="cuda", generator=g) == 0
    bm = pack(torch, bits)
    torch.cuda.synchronize()
    res = {"bytes": size, "device": torch.cuda.get_device_name(0), "lines": n, "selected": int(bits.sum()),
           "scan_block": hip.text_context_scan_block(), "contexts": {}}
    for before, after in ((0, 0), (2, 2), (1000, 1000)):
        ctx, sel, gat, psel, pgat = [], [], [], [], []
        m = nb = groups = 0
        for rep in range(4):
            h = t.hits_context_device(bm.data_ptr(), before, after)
            ctx.append(h.context_ms())
            sel.append(h.ms() - h.gather_ms())
            gat.append(h.gather_ms())
            m, nb, groups = h.count, h.nbytes, h.groups
            assert h.core_count == res["selected"]
            if size <= (64 << 20) and rep == 0:
                host = bits.cpu().numpy()
                W = context_witness(host, before, after)
                lines, core, group = marks_ref(host, W)
                assert np.array_equal(h.lines(), lines) and np.array_equal(h.core(), core) and np.array_equal(h.group(), group)
            h.close()
            p = t.hits_device(bm.data_ptr())
            psel.append(p.ms() - p.gather_ms())
            pgat.append(p.gather_ms())
            p.close()
        res["contexts"]["%d_%d" % (before, after)] = {
            "hits": m, "bytes": nb, "groups": groups, "context_ms": round(min(ctx[1:]), 4), "select_ms_same_handle": round(min(sel[1:]), 4),
            "gather_ms_same_handle": round(min(gat[1:]), 4), "context_over_select": round(min(ctx[1:]) / min(sel[1:]), 3),
            "plain_select_ms": round(min(psel[1:]), 4), "plain_gather_ms": round(min(pgat[1:]), 4)}
        print(f"-B {before} -A {after}: {m} hits in {groups} groups, {nb} bytes; context {min(ctx[1:]):.3f} ms, select {min(sel[1:]):.3f} ms, "
              f"gather {min(gat[1:]):.3f} ms; plain hits: select {min(psel[1:]):.3f} ms, gather {min(pgat[1:]):.3f} ms", flush=True)
    t.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
