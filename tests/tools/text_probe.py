#!/usr/bin/env python3
"""tests/tools/text_probe.py -- what the text front costs, on one device, for a text of TEXT_BYTES (default 1 GiB) of 8-64-byte
lines and one of 0-1024-byte lines (lowercase letters and digits, '\\n' between them):

 (a) the three scan kernels together (HIP events around them, fsm_hip_text_scan_ms) beside 2 x fsm_hip_stream_read_probe_ms
     over the same bytes -- the scan reads the text twice, so that is its denominator;
 (b) fsm_hip_last_kernel_ms of the walk over the twin automaton on the untouched text against the ORIGINAL dfa on the
     squeezed text with hipgrep-style offsets: same lines, interleaved, with the layout and kernel each got;
 (c) end to end from host memory: fsm_hip_text_open + fsm_hip_text_exec against the loop of examples/hipgrep.c:69-90
     (restated below, gcc -O2) followed by fsm_hip_exec_batch_offsets; wall clock, three interleaved runs.

usage: text_probe.py [out.json]   (default: profiles/text_probe.json)"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# the host loop of examples/hipgrep.c (lines 69-90): walk the buffer byte by byte, squeeze every line over the newlines before it,
# build the u64 offsets.  off must hold one entry more than there are lines; returns the number of lines.
SQUEEZE_C = r"""
#include <stddef.h>
#include <stdint.h>
#include <string.h>
size_t squeeze(unsigned char *buf, size_t len, uint64_t *off)
{
	size_t i, n = 0, start = 0;
	for (i = 0; i <= len; i++) {
		if (i == len ? start < len : buf[i] == '\n') {
			if (n == 0) {
				off[0] = 0;
			}
			memmove(buf + off[n], buf + start, i - start);
			off[n + 1] = off[n] + (i - start);
			n++;
			start = i + 1;
		}
	}
	return n;
}
"""


def make_text(torch, size, lo, hi, seed):
    """`size` bytes on the device: lines of lo..hi random bytes of [a-z0-9], a '\\n' behind each (the last line may be cut)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    mean = (lo + hi) / 2 + 1
    nl = int(size / mean * 1.05) + 16
    lens = torch.randint(lo, hi + 1, (nl,), device="cuda", generator=g, dtype=torch.int64)
    ends = torch.cumsum(lens + 1, 0) - 1                   # position of every line's newline
    ends = ends[ends < size]
    r = torch.randint(0, 36, (size,), device="cuda", generator=g, dtype=torch.uint8)
    text = torch.where(r < 26, r + 97, r + 22)            # a-z, 0-9
    del r
    text[ends] = 0x0A
    return text


def main():
    import torch
    import libfsm_amd as hip
    from common import GOLDEN, Golden
    from text_ref import split_ref
    hip.load_library()
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "text_probe.json")
    size = int(os.environ.get("TEXT_BYTES", 1 << 30))
    torch.cuda.set_device(0)
    scratch = torch.zeros(64, dtype=torch.int32, device="cuda")
    td = tempfile.mkdtemp(prefix="textprobe")
    open(os.path.join(td, "squeeze.c"), "w").write(SQUEEZE_C)
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-shared", "-fPIC", os.path.join(td, "squeeze.c"), "-o", os.path.join(td, "squeeze.so")])
    sq_lib = ctypes.CDLL(os.path.join(td, "squeeze.so"))
    sq_lib.squeeze.restype = ctypes.c_size_t
    sq_lib.squeeze.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    automata = {"c1": Golden(os.path.join(GOLDEN, "c1.npz")).flat, "c3": Golden(os.path.join(GOLDEN, "c3.npz")).flat}
    res = {"bytes": size, "device": torch.cuda.get_device_name(0), "block_bytes": hip.text_block_bytes(), "texts": {}}
    for tname, lo, hi in (("lines_8_64", 8, 64), ("lines_0_1024", 0, 1024)):
        text = make_text(torch, size, lo, hi, 5)
        torch.cuda.synchronize()
        r = res["texts"][tname] = {}
        # (a) the scan
        read_ms = size / hip.stream_read_probe_gbps(text.data_ptr(), size, scratch.data_ptr()) / 1e6
        scan = []
        for rep in range(4):
            t = hip.HipText(d_text=text.data_ptr(), nbytes=size, delim=0x0A)
            scan.append(t.scan_ms())
            if rep < 3:
                t.close()
        n = t.lines
        r["lines"] = n
        r["scan_ms"] = [round(x, 4) for x in scan]
        r["stream_read_ms_x2"] = round(2 * read_ms, 4)
        r["scan_over_two_reads"] = round(min(scan[1:]) / (2 * read_ms), 3)
        print(f"{tname}: {n} lines; scan {min(scan[1:]):.3f} ms, 2 x stream read {2 * read_ms:.3f} ms", flush=True)
        if size <= (64 << 20):      # small runs double as a check against the reference splitter
            assert np.array_equal(t.offsets(), split_ref(text.cpu().numpy(), 0x0A))
        # the squeezed copy and its offsets, on the device (hipgrep.c's batch)
        off = torch.from_numpy(t.offsets().astype(np.int64)).cuda()
        sq = text[text != 0x0A]
        off_sq = off - torch.arange(n + 1, dtype=torch.int64, device="cuda")       # k delimiters lie before off[k] ...
        if int(text[-1]) != 0x0A:
            off_sq[n] += 1                                                         # ... but for a last line without one
        end_a = torch.empty(n, dtype=torch.int32, device="cuda")
        end_b = torch.empty(n, dtype=torch.int32, device="cuda")
        # (b) the walk: twin on the untouched text, original on the squeezed one
        r["walk"] = {}
        for aname, flat in automata.items():
            ld, dfa = hip.LinesDfa(flat, 0x0A), hip.HipDfa(flat)
            ms_t, ms_o = [], []
            for rep in range(4):
                t.exec_device(ld, end_a.data_ptr())
                ms_t.append(ld.inner.last_kernel_ms())
                dfa.exec_batch_offsets_device(sq.data_ptr(), off_sq.data_ptr(), n, end_b.data_ptr())
                ms_o.append(dfa.last_kernel_ms())
            torch.cuda.synchronize()
            assert torch.equal(end_a, end_b), "twin on the text != original on the squeezed copy"
            a, b = min(ms_t[1:]), min(ms_o[1:])
            r["walk"][aname] = {"twin_ms": [round(x, 4) for x in ms_t], "original_squeezed_ms": [round(x, 4) for x in ms_o],
                                "twin_over_original": round(a / b, 4), "accepts": int((end_a != -1).sum()),
                                "twin": {"layout": ld.inner.info()["layout_name"], "classes": ld.inner.info()["nclasses"], "kernel": ld.inner.last_kernel_name()},
                                "original": {"layout": dfa.info()["layout_name"], "classes": dfa.info()["nclasses"], "kernel": dfa.last_kernel_name()}}
            print(f"  {aname}: twin {a:.3f} ms ({ld.inner.last_kernel_name()}), original on squeezed {b:.3f} ms ({dfa.last_kernel_name()})", flush=True)
        t.close()
        del sq, off_sq, off, end_b
        # (c) end to end from host memory
        host = text.cpu().numpy()
        ld, dfa = hip.LinesDfa(automata["c3"], 0x0A), hip.HipDfa(automata["c3"])
        new_s, old_s, old_loop_s = [], [], []
        for rep in range(3):
            t0 = time.perf_counter()
            ht = hip.HipText(host, 0x0A)
            got = ht.exec(ld)["end"]
            new_s.append(time.perf_counter() - t0)
            ht.close()
            buf = host.copy()
            offs = np.empty(n + 2, np.uint64)
            t0 = time.perf_counter()
            k = sq_lib.squeeze(buf.ctypes.data, size, offs.ctypes.data)
            t1 = time.perf_counter()
            want, _ = dfa.exec_batch_offsets(buf[:int(offs[k])], offs[:k + 1], want_bitmap=False)
            old_s.append(time.perf_counter() - t0)
            old_loop_s.append(t1 - t0)
            assert k == n and np.array_equal(got, want)
        r["end_to_end"] = {"text_open_exec_s": [round(x, 4) for x in new_s], "host_loop_then_offsets_s": [round(x, 4) for x in old_s],
                           "host_loop_alone_s": [round(x, 4) for x in old_loop_s]}
        print(f"  end to end (c3): text front {min(new_s):.3f} s, host loop + offsets {min(old_s):.3f} s (loop alone {min(old_loop_s):.3f} s)", flush=True)
        del text, host, end_a
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
