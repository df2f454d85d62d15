#!/usr/bin/env python3
"""tests/tools/files_probe.py -- what the files of a text cost, on one device: TEXT_BYTES (default 1 GiB) of 8-64-byte lines
(text_probe.make_text) as 10^3 files and as 10^6 files, the file ends drawn uniformly (almost all of them inside a line):

 (a) the added kernels of the open (files_mark + files_scan + files_merge: fsm_hip_text_files_ms) beside the delimiter scan of
     the SAME text (fsm_hip_text_scan_ms), and the scan of the plain text over the same bytes (its code did not change: the figure
     belongs inside the box-to-box spread of earlier records);
 (b) hits_file_first (fsm_hip_text_hits_file_first_ms) beside the select's three kernels (fsm_hip_text_hits_ms under NO_BYTES), one
     line in 8 selected;
 (c) for 10^3 files only: host memory to per-file counts with the c3 automaton, wall clock: ONE fsm_hip_text_open_files +
     fsm_hip_text_hits(NO_BYTES) + fsm_hip_text_hits_file_first, against a loop of fsm_hip_text_open + fsm_hip_text_hits(NO_BYTES) +
     fsm_hip_text_hits_count per file.
Best of three after a warm-up, the sides interleaved.

usage: files_probe.py [out.json]   (default: profiles/files_probe.json)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))


def main():
    import torch
    import libfsm_amd as hip
    from common import GOLDEN, Golden
    from files_ref import files_ref
    from hits_probe import pack
    from text_probe import make_text
    hip.load_library()
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "files_probe.json")
    size = int(os.environ.get("TEXT_BYTES", 1 << 30))
    torch.cuda.set_device(0)
    c3 = Golden(os.path.join(GOLDEN, "c3.npz")).flat
    res = {"bytes": size, "device": torch.cuda.get_device_name(0), "files_block": hip.text_files_block(), "files": {}}
    g = torch.Generator(device="cuda")
    g.manual_seed(23)
    text = make_text(torch, size, 8, 64, 5)
    torch.cuda.synchronize()
    plain_ms = []
    for nfiles in (1000, 1000000):
        inner = torch.sort(torch.randint(0, size + 1, (nfiles - 1,), device="cuda", generator=g, dtype=torch.int64))[0]
        fo = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), inner, torch.full((1,), size, dtype=torch.int64, device="cuda")])
        torch.cuda.synchronize()
        files_ms, scan_ms, sel_ms, ff_ms = [], [], [], []
        for rep in range(4):
            p = hip.HipText(d_text=text.data_ptr(), nbytes=size, delim=0x0A)
            plain_ms.append(p.scan_ms())
            plain_lines = p.lines
            p.close()
            t = hip.HipText(d_text=text.data_ptr(), nbytes=size, delim=0x0A, file_off=fo.data_ptr(), nfiles=nfiles)
            files_ms.append(t.files_ms())
            scan_ms.append(t.scan_ms())
            n = t.lines
            if rep == 0:
                bits = torch.randint(0, 8, (n,), device="cuda", generator=g) == 0
                bm = pack(torch, bits)
                torch.cuda.synchronize()
                if size <= (64 << 20):      # small runs double as a check against the reference
                    off, fl = files_ref(text.cpu().numpy(), 0x0A, fo.cpu().numpy().astype(np.uint64))
                    assert np.array_equal(t.offsets(), off) and np.array_equal(t.file_lines(), fl)
            h = t.hits_device(bm.data_ptr(), want_bytes=False)
            sel_ms.append(h.ms())
            ff_ms.append(h.file_first_ms())
            first = h.file_first()
            assert int(first[-1]) == h.count == int(bits.sum())
            h.close()
            t.close()
        r = res["files"][str(nfiles)] = {"lines": n, "lines_added_by_file_ends": n - plain_lines, "files_ms": round(min(files_ms[1:]), 4),
                                         "scan_ms_same_text": round(min(scan_ms[1:]), 4), "select_ms": round(min(sel_ms[1:]), 4),
                                         "hits_file_first_ms": round(min(ff_ms[1:]), 4)}
        print(f"{nfiles} files: {n} lines ({n - plain_lines} added); files {r['files_ms']:.3f} ms beside scan {r['scan_ms_same_text']:.3f} ms; "
              f"file_first {r['hits_file_first_ms']:.3f} ms beside select {r['select_ms']:.3f} ms", flush=True)
        if nfiles == 1000:      # (c) host memory to per-file counts
            host = text.cpu().numpy()
            hfo = fo.cpu().numpy().astype(np.uint64)
            ld = hip.LinesDfa(c3, 0x0A)
            one_s, loop_s = [], []
            for rep in range(4):
                t0 = time.perf_counter()
                t = hip.HipText(host, 0x0A, file_off=hfo)
                h = t.hits(ld, want_bytes=False)
                counts = np.diff(h.file_first().astype(np.int64))
                one_s.append(time.perf_counter() - t0)
                h.close()
                t.close()
                t0 = time.perf_counter()
                each = np.zeros(nfiles, np.int64)
                for j in range(nfiles):
                    tj = hip.HipText(host[int(hfo[j]):int(hfo[j + 1])], 0x0A)
                    hj = tj.hits(ld, want_bytes=False)
                    each[j] = hj.count
                    hj.close()
                    tj.close()
                loop_s.append(time.perf_counter() - t0)
                assert np.array_equal(counts, each)
            r["end_to_end_c3"] = {"selected": int(counts.sum()), "open_files_hits_file_first_s": [round(x, 4) for x in one_s],
                                  "loop_of_open_hits_per_file_s": [round(x, 4) for x in loop_s]}
            print(f"  end to end (c3, {int(counts.sum())} lines in {nfiles} files): one text {min(one_s[1:]):.3f} s, a text per file {min(loop_s[1:]):.3f} s",
                  flush=True)
            del host
        del inner, fo, bits, bm
    res["plain_scan_ms"] = round(min(plain_ms[1:]), 4)
    res["plain_scan_ms_all"] = [round(x, 4) for x in plain_ms]
    print(f"plain text over the same bytes: scan {res['plain_scan_ms']:.3f} ms", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
