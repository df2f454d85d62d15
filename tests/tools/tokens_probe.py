#!/usr/bin/env python3
"""tests/tools/tokens_probe.py -- what cutting every line into tokens costs, on one device (not run by pytest):
TEXT_BYTES (default 1 GiB) of 8-64-byte lines and of 0-1024-byte lines, with
  words     the word lexer of tests/test_tokens_abi.py (a trie over a ab abcda b bc bcdab c ca cab d dd ddabc) on lines over
            abcdx, x at 4 %: many short tokens, a bad byte now and then;
  dying1023 the largest LDS image (affine, 1 023 states x 16 classes, holes and sinks: tests/test_gpu_tokens.py) on random bytes:
            long tokens, long overruns,
each by default (a line stops at its first bad byte) and under FSM_HIP_TOKENS_SKIP_BAD.  Reported per case:
  count_ms, scan_ms, emit_ms   the three passes by the object's own HIP events (fsm_hip_tokens_pass_ms), best of three after a warm-up;
  tokens, tokens_per_s         over count + scan + emit;
  walked_ratio                 bytes walked / text bytes, by the CPU judge (tests/tokens_ref.py) on the text's first SAMPLE lines;
  walk_pos_ms                  walk_pos forward over the same lines with the same table (fsm_hip_exec_accept_pos_device, last asked
                               for): one walk of every byte until it stops -- what the count pass is measured against;
  count_over_pos               count_ms / walk_pos_ms, to be read beside walked_ratio.
No ratio is fixed in advance.

usage: tokens_probe.py [out.json]   (default: profiles/tokens_probe.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TEXTS = {"8_64": (8, 64, 5), "0_1024": (0, 1024, 6)}
WORDS = [w.encode() for w in "a ab abcda b bc bcdab c ca cab d dd ddabc".split()]
SAMPLE = 1500


def make_text(torch, size, lo, hi, seed, words):
    """`size` bytes on the device: lines of lo..hi bytes, a '\\n' behind each (the last line may be cut); words: over abcdx with
    x at 4 %, else any byte but the newline"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    nl = int(size / ((lo + hi) / 2 + 1) * 1.05) + 16
    lens = torch.randint(lo, hi + 1, (nl,), device="cuda", generator=g, dtype=torch.int64)
    ends = torch.cumsum(lens + 1, 0) - 1
    ends = ends[ends < size]
    if words:
        r = torch.randint(0, 100, (size,), device="cuda", generator=g, dtype=torch.uint8)
        text = torch.where(r < 96, (r // 24) + 97, torch.full_like(r, 120))      # a b c d at 24 % each, x at 4 %
    else:
        text = torch.randint(0, 256, (size,), device="cuda", generator=g, dtype=torch.uint8)
        text[text == 0x0A] = 0x0B
    text[ends] = 0x0A
    return text


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


def main():
    import numpy as np
    import torch
    import libfsm_amd as hip
    import tokens_ref
    from global_ref import affine
    from span_ref import rows_of
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tokens_probe.json")
    size = int(os.environ.get("TEXT_BYTES", 1 << 30))
    torch.cuda.set_device(0)
    words_auto, sets = tokens_ref.trie_lexer(WORDS)
    autos = {"words": (words_auto, sets), "dying1023": (affine(1023, 16, holes=8, sinks=4, endids=True), None)}
    res = {"bytes": size, "device": torch.cuda.get_device_name(0), "sample_lines": SAMPLE, "cases": {}}
    for which, (lo, hi, seed) in TEXTS.items():
        for name, (auto, sets) in autos.items():
            text = make_text(torch, size, lo, hi, seed, name == "words")
            torch.cuda.synchronize()
            t = hip.HipText(d_text=text.data_ptr(), nbytes=size, delim=0x0A)
            n = t.lines
            td = hip.TokDfa.from_flat(auto[0])
            pd = hip.PosDfa.from_flat(auto[0])
            assert td.in_lds and pd.in_lds
            last = torch.empty(n, dtype=torch.int64, device="cuda")
            pos_ms = timed(torch, lambda: pd.accept_pos_device(text.data_ptr(), t.d_off, n, 0, last.data_ptr(), trim_byte=0x0A, limit=size))
            # the judge on the first lines: the re-walk factor, and the device's answer for them while we are here
            off = t.offsets()[:SAMPLE + 1].astype(np.int64)
            raw = text[:int(off[-1])].cpu().numpy().tobytes()
            lines = [raw[off[i]:off[i + 1]].rstrip(b"\n") for i in range(len(off) - 1)]
            judge = tokens_ref.Judge(auto, *rows_of(lines))
            ids = tokens_ref.state_ids(auto, tokens_ref.EARLIEST, sets)
            for mode, flags in (("default", 0), ("skip_bad", hip.TOKENS_SKIP_BAD)):
                want = judge.run(flags, ids)
                passes = []
                for rep in range(4):
                    tk = td.text_tokens(t, flags=flags)
                    passes.append([tk.pass_ms(k) for k in range(3)])
                    total = tk.total
                    if rep == 0:
                        goff = np.empty(n + 1, np.uint64)
                        hip.capi._call("fsm_hip_tokens_copy", tk.handle, hip.capi._ptr(goff), None, None, None)
                        assert np.array_equal(goff[:len(lines) + 1], want["off"]), "the device's counts differ from the judge's on the sample"
                    tk.close()
                count_ms, scan_ms, emit_ms = (min(p[k] for p in passes[1:]) for k in range(3))
                case = {"lines": n, "tokens": total, "count_ms": round(count_ms, 4), "scan_ms": round(scan_ms, 4), "emit_ms": round(emit_ms, 4),
                        "tokens_per_s": round(total / ((count_ms + scan_ms + emit_ms) * 1e-3)), "walked_ratio": round(want["walked"] / max(len(raw), 1), 3),
                        "walk_pos_ms": round(pos_ms, 4), "count_over_pos": round(count_ms / pos_ms, 3)}
                res["cases"]["%s/%s/%s" % (which, name, mode)] = case
                print(which, name, mode, case, flush=True)
            td.close()
            pd.close()
            t.close()
            del text, last
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
