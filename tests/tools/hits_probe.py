#!/usr/bin/env python3
"""tests/tools/hits_probe.py -- what the hits of the text front cost, on one device, for the two texts of text_probe.py
(TEXT_BYTES, default 1 GiB, of 8-64-byte and of 0-1024-byte lines), at three selectivities (one line in 1000, one in 8, all):

 (a) the three select kernels (HIP events, fsm_hip_text_hits_ms under NO_BYTES) beside fsm_hip_stream_read_probe_ms scaled to
     the bytes they read: twice the bitmap plus twice the 8 * (n + 1) offsets;
 (b) the gather alone (fsm_hip_text_hits_gather_ms) beside a device-to-device copy of the same number of bytes (torch's
     copy_ of contiguous bytes: hipMemcpyDtoDAsync), HIP events around it; at "all lines" the gather IS that copy, so the ratio
     there is the price of the ragged form;
 (c) host memory to printed lines with the c3 automaton: fsm_hip_text_open + fsm_hip_text_hits + fsm_hip_text_hits_copy against
     fsm_hip_text_open + fsm_hip_text_exec(end states) + fsm_hip_text_offsets + the host loop hipgrep_text.c would need to print
     lines (restated below, gcc -O2); wall clock;
 and one row for a single 64 MiB line selected alone, against the same copy.
Best of three after a warm-up, the sides interleaved.

usage: hits_probe.py [out.json]   (default: profiles/hits_probe.json)"""
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
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

# the loop a caller of fsm_hip_text_exec needs to get the matching lines' bytes: one pass over the n end states, a memcpy per hit
PRINT_C = r"""
#include <stddef.h>
#include <stdint.h>
#include <string.h>
size_t collect(const unsigned char *text, const uint64_t *off, const uint32_t *end, size_t n, unsigned char *out, size_t *m)
{
	size_t i, o = 0, k = 0;
	for (i = 0; i < n; i++) {
		if (end[i] != 0xFFFFFFFFu) {
			memcpy(out + o, text + off[i], off[i + 1] - off[i]);
			o += off[i + 1] - off[i];
			k++;
		}
	}
	*m = k;
	return o;
}
"""


def pack(torch, bits):
    """bool tensor of n lines -> the bitmap of ceil(n / 64) words on the device"""
    n = bits.numel()
    full = torch.zeros((n + 63) // 64 * 64, dtype=torch.int64, device="cuda")
    full[:n] = bits
    return (full.view(-1, 64) << torch.arange(64, dtype=torch.int64, device="cuda")).sum(1)     # distinct bits: the sum is the OR


def copy_ms(torch, nbytes):
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    dst.copy_(src)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def select_and_gather(torch, hip, t, bm, nbytes_hint=None):
    """best of three after a warm-up, interleaved: select ms (NO_BYTES), gather ms, copy ms of the gathered bytes"""
    sel, gat, cop = [], [], []
    m = nb = 0
    for rep in range(4):
        h = t.hits_device(bm.data_ptr(), want_bytes=False)
        sel.append(h.ms())
        h.close()
        h = t.hits_device(bm.data_ptr())
        gat.append(h.gather_ms())
        m, nb = h.count, h.nbytes
        h.close()
        cop.append(copy_ms(torch, max(nb, 1)))
    return m, nb, min(sel[1:]), min(gat[1:]), min(cop[1:])


def main():
    import torch
    import libfsm_amd as hip
    from common import GOLDEN, Golden
    from hits_ref import hits_ref
    from text_probe import make_text
    hip.load_library()
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hits_probe.json")
    size = int(os.environ.get("TEXT_BYTES", 1 << 30))
    torch.cuda.set_device(0)
    scratch = torch.zeros(64, dtype=torch.int32, device="cuda")
    td = tempfile.mkdtemp(prefix="hitsprobe")
    open(os.path.join(td, "collect.c"), "w").write(PRINT_C)
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-shared", "-fPIC", os.path.join(td, "collect.c"), "-o", os.path.join(td, "collect.so")])
    clib = ctypes.CDLL(os.path.join(td, "collect.so"))
    clib.collect.restype = ctypes.c_size_t
    clib.collect.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2
    c3 = Golden(os.path.join(GOLDEN, "c3.npz")).flat
    res = {"bytes": size, "device": torch.cuda.get_device_name(0), "block_lines": hip.text_hits_block_lines(),
           "block_bytes": hip.text_hits_block_bytes(), "texts": {}}
    g = torch.Generator(device="cuda")
    g.manual_seed(17)
    for tname, lo, hi in (("lines_8_64", 8, 64), ("lines_0_1024", 0, 1024)):
        text = make_text(torch, size, lo, hi, 5)
        torch.cuda.synchronize()
        t = hip.HipText(d_text=text.data_ptr(), nbytes=size, delim=0x0A)
        n = t.lines
        r = res["texts"][tname] = {"lines": n, "select": {}}
        read_bytes = 2 * ((n + 63) // 64 * 8) + 2 * 8 * (n + 1)
        gbps = hip.stream_read_probe_gbps(t.d_off, 8 * (n + 1), scratch.data_ptr())
        r["select_reads_bytes"] = read_bytes
        r["stream_read_ms_of_those_bytes"] = round(read_bytes / gbps / 1e6, 4)
        for sname, one_in in (("1_in_1000", 1000), ("1_in_8", 8), ("all", 1)):
            bits = torch.randint(0, one_in, (n,), device="cuda", generator=g) == 0
            bm = pack(torch, bits)
            torch.cuda.synchronize()
            m, nb, sel, gat, cop = select_and_gather(torch, hip, t, bm)
            assert m == int(bits.sum())
            if size <= (64 << 20):      # small runs double as a check against the reference
                h = t.hits_device(bm.data_ptr())
                want = hits_ref(text.cpu().numpy(), 0x0A, bits.cpu().numpy())
                assert np.array_equal(h.lines(), want[0]) and np.array_equal(h.offsets(), want[1]) and np.array_equal(h.bytes(), want[2])
                h.close()
            r["select"][sname] = {"selected": m, "bytes": nb, "select_ms": round(sel, 4), "select_over_stream_read": round(sel / (read_bytes / gbps / 1e6), 3),
                                  "gather_ms": round(gat, 4), "copy_ms": round(cop, 4), "gather_over_copy": round(gat / cop, 3),
                                  "gather_gbps_out": round(nb / gat / 1e6, 1) if gat > 0 else None}
            print(f"{tname} {sname}: m = {m}, {nb} bytes; select {sel:.3f} ms (stream read of its bytes {read_bytes / gbps / 1e6:.3f} ms); "
                  f"gather {gat:.3f} ms, copy {cop:.3f} ms", flush=True)
            del bits, bm
        t.close()
        # (c) host memory to the matching lines' bytes, c3
        host = text.cpu().numpy()
        ld = hip.LinesDfa(c3, 0x0A)
        new_s, old_s, loop_s = [], [], []
        for rep in range(4):
            t0 = time.perf_counter()
            ht = hip.HipText(host, 0x0A)
            h = ht.hits(ld)
            lines, off, got = h.lines(), h.offsets(), h.bytes()
            new_s.append(time.perf_counter() - t0)
            h.close()
            ht.close()
            t0 = time.perf_counter()
            ht = hip.HipText(host, 0x0A)
            end = ht.exec(ld)["end"]
            offs = ht.offsets()
            t1 = time.perf_counter()
            out = np.empty(size, np.uint8)
            m = ctypes.c_size_t(0)
            nb = clib.collect(host.ctypes.data, offs.ctypes.data, end.ctypes.data, n, out.ctypes.data, ctypes.byref(m))
            old_s.append(time.perf_counter() - t0)
            loop_s.append(time.perf_counter() - t1)
            ht.close()
            assert m.value == len(lines) and nb == len(got) and np.array_equal(out[:nb], got)
        r["end_to_end_c3"] = {"selected": len(lines), "bytes": len(got), "open_hits_copy_s": [round(x, 4) for x in new_s],
                              "open_exec_offsets_loop_s": [round(x, 4) for x in old_s], "host_loop_alone_s": [round(x, 4) for x in loop_s]}
        print(f"  end to end (c3, {len(lines)} lines): hits {min(new_s[1:]):.3f} s, exec + offsets + host loop {min(old_s[1:]):.3f} s "
              f"(loop alone {min(loop_s[1:]):.3f} s)", flush=True)
        del text, host, out
        torch.cuda.empty_cache()
    # one 64 MiB line between short ones, selected alone
    big = 64 << 20
    text = make_text(torch, big + (2 << 20), 8, 64, 9)
    text[1 << 20:(1 << 20) + big - 1] = 0x61
    text[(1 << 20) - 1] = 0x0A
    text[(1 << 20) + big - 1] = 0x0A
    torch.cuda.synchronize()
    t = hip.HipText(d_text=text.data_ptr(), nbytes=text.numel(), delim=0x0A)
    off = torch.from_numpy(t.offsets().astype(np.int64)).cuda()
    bits = (off[1:] - off[:-1]) == big
    assert int(bits.sum()) == 1
    m, nb, sel, gat, cop = select_and_gather(torch, hip, t, pack(torch, bits))
    assert m == 1 and nb == big
    res["one_line_64MiB"] = {"lines": t.lines, "select_ms": round(sel, 4), "gather_ms": round(gat, 4), "copy_ms": round(cop, 4),
                             "gather_over_copy": round(gat / cop, 3)}
    print(f"one 64 MiB line: select {sel:.3f} ms, gather {gat:.3f} ms, copy {cop:.3f} ms", flush=True)
    t.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
