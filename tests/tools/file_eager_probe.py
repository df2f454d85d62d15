#!/usr/bin/env python3
"""tests/tools/file_eager_probe.py -- fsm_hip_match_buffer_big against fsm_hip_match_buffer_big_eager on the same in-memory input
(1 GiB by default: FILE_BYTES) with the eager40 automaton (fsm_union_repeated_pattern_group over 40 unanchored literals, one eager
id each: tests/golden/bench/eager40.npz), lowercase text with a pattern planted every 4 KiB.  Prints the time of each call, its
windows and passes, and the eager call's ratio to the plain one; a second line splits the eager call's cost: one resumed eager walk
of a window's pieces, the same walk without sets, and the per-piece zeroing.  (Under tests/: the oracle is the checker.)"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import libfsm_amd as hip
    from oracle.pyoracle import Oracle
    hip.load_library()
    size = int(os.environ.get("FILE_BYTES", 1 << 30))
    reps = int(os.environ.get("REPS", 3))
    z = np.load(os.path.join(ROOT, "tests", "golden", "bench", "eager40.npz"))
    flat = hip.FlatDfa.load(z)
    pats = bytes(z["patterns"]).split(b"\n")
    rng = np.random.RandomState(5)
    data = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)[rng.randint(0, 26, size, dtype=np.uint8)]
    for k, at in enumerate(range(1000, size - 8, 4096)):
        p = pats[k % len(pats)]
        data[at:at + len(p)] = np.frombuffer(p, np.uint8)
    buf = (C.c_char * size).from_buffer(data)
    dfa = hip.HipDfa(flat)
    lib, h = dfa._lib, C.c_void_p(dfa._h)
    W = dfa.eager_words()
    eo = np.zeros(W, np.uint64)
    end = C.c_uint32(0)
    dfa.match_buffer(b"warm up")
    print(f"eager40: {flat.nstates} states, {dfa.eager_id_count()} eager ids, W = {W}, layout {dfa.info()['layout_name']}; {size} bytes in memory", flush=True)
    res = {}
    for rep in range(reps):
        for name in ("plain", "eager"):
            t0 = time.perf_counter()
            if name == "plain":
                r = lib.fsm_hip_match_buffer_big(h, buf, C.c_size_t(size), C.byref(end))
            else:
                r = lib.fsm_hip_match_buffer_big_eager(h, buf, C.c_size_t(size), C.byref(end), eo.ctypes.data_as(C.c_void_p))
            t = time.perf_counter() - t0
            w, p = dfa.match_last_passes()
            res.setdefault(name, []).append(t)
            print(f"{name:5s} fsm_hip_match_buffer_big{'_eager' if name == 'eager' else '      '}: -> {r} end {end.value:#x} in {t * 1e3:8.1f} ms = "
                  f"{size / t / 1e9:6.2f} GB/s  ({w} windows, {p} passes, {p / max(w, 1):.2f} a window)"
                  + (f"  ids {int(np.unpackbits(eo.view(np.uint8)).sum())}" if name == "eager" else ""), flush=True)
    tp, te = min(res["plain"]), min(res["eager"])
    print(f"best of {reps}: plain {tp * 1e3:.1f} ms, eager {te * 1e3:.1f} ms: eager / plain = {te / tp:.3f}", flush=True)

    # where the eager call's time goes: one window of pieces (32 MiB as 32768 x 1 KiB) on the device, the walks timed alone
    n, L = 32768, 1024
    d_in = torch.from_numpy(data[:n * L].copy()).cuda()
    d_st = torch.empty(n, dtype=torch.int32, device="cuda")
    d_sets = torch.zeros(n * W, dtype=torch.int64, device="cuda")
    st0 = torch.full((n,), -3, dtype=torch.int32, device="cuda")   # FSM_HIP_STATE_START
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn, k=10):
        fn()
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(k):
            d_st.copy_(st0)
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            best = min(best, ev[0].elapsed_time(ev[1]))
        return best

    t_eager = timed(lambda: lib.fsm_hip_exec_batch_eager_resume_device(h, C.c_void_p(d_in.data_ptr()), C.c_size_t(L), None, None, C.c_size_t(n),
                                                                        C.c_void_p(d_st.data_ptr()), None, C.c_void_p(d_sets.data_ptr()), None))
    k_eager = dfa.last_kernel_name()
    t_plain = timed(lambda: lib.fsm_hip_exec_batch_resume_device(h, C.c_void_p(d_in.data_ptr()), C.c_size_t(L), None, C.c_size_t(n),
                                                                  C.c_void_p(d_st.data_ptr()), None, None, None))
    k_plain = dfa.last_kernel_name()
    t_zero = timed(lambda: d_sets.zero_())
    print(f"one window ({n} x {L} B) on the device: resumed eager walk {t_eager:.3f} ms ({n * L / t_eager / 1e6:.0f} GB/s, {k_eager}), "
          f"resumed plain walk {t_plain:.3f} ms ({n * L / t_plain / 1e6:.0f} GB/s, {k_plain}), zeroing the per-piece sets {t_zero:.3f} ms", flush=True)

    # the answer, checked: the oracle over the last 64 MiB as its own input against the eager call on the same bytes
    k = min(size, 64 << 20)
    tail = data[size - k:]
    ret, wend, sets = Oracle(flat).exec_eager(tail[None, :], cap=48)
    r, e, ids = dfa.match_buffer_big_eager(tail.tobytes())
    ok = (r, e) == (int(ret[0]), int(wend[0])) and np.array_equal(ids, sets[0])
    print(f"check: the last {k} bytes as one input: HIP == oracle: {ok} ({len(ids)} ids)", flush=True)
    dfa.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
