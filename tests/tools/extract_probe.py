#!/usr/bin/env python3
"""tests/tools/extract_probe.py -- what extracting every match of every line costs on one device (not run by pytest): the four
texts of tests/tools/replace_probe.py, TEXT_BYTES (default 1 GiB) of 8-64-byte lines and of 0-1024-byte lines, the word ab, with
  dense    a text over abcd, uniform: ab begins at one position in 16, so about one match per 16 bytes;
  sparse   a text over c .. z with ab planted at the head of every line of two bytes or more: one match per line.
The matches are fsm_hip_text_matches' over EVERY line (DROP_EMPTY); they are made once per text and are not part of any figure.
Every match is kept, with '\\n' behind it (records of three bytes: a chunk of the write pass holds five) and without a separator
(records of two: eight).  Reported per case and separator, best of three after a warm-up:
  lengths_ms, scan_ms, offsets_ms, write_ms   the four passes by the object's own HIP events (fsm_hip_extracted_pass_ms);
  call_ms                                     the whole fsm_hip_text_extract call between two events on the stream: the passes AND
                                              the host's wait for the totals and the allocations;
  out_bytes, copy_ms, write_over_copy         a device-to-device copy of the output's size, same process, interleaved, and the
                                              write pass over it.
Per case, in the same process and interleaved with the above:
  gather_ms                                   fsm_hip_text_hits gathering every line of the same text (the hits of an inverted
                                              matcher of a word that does not occur): the whole text moved, for scale.
The device's answer is held against the CPU judge (tests/extract_ref.py over tests/matches_ref.py) on the first SAMPLE lines.  No
figure is a gate and no ratio is fixed in advance.

usage: extract_probe.py [out.json]   (default: profiles/extract_probe.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TEXTS = {"8_64": (8, 64, 5), "0_1024": (0, 1024, 6)}
WORDS = [b"ab"]
SAMPLE = 1500
SEPS = {"newline": 0x0A, "none": -1}


def make_text(torch, size, lo, hi, seed, dense):
    """`size` bytes on the device: lines of lo..hi bytes, a '\\n' behind each (the last line may be cut)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    nl = int(size / ((lo + hi) / 2 + 1) * 1.05) + 16
    lens = torch.randint(lo, hi + 1, (nl,), device="cuda", generator=g, dtype=torch.int64)
    ends = torch.cumsum(lens + 1, 0) - 1
    keep = ends < size
    if dense:
        text = torch.randint(97, 101, (size,), device="cuda", generator=g, dtype=torch.uint8)       # a b c d
    else:
        text = torch.randint(99, 123, (size,), device="cuda", generator=g, dtype=torch.uint8)       # c .. z
        first = (ends - lens)[keep & (lens >= 2)]                                                  # the line's first byte
        text[first] = 97
        text[first + 1] = 98
    text[ends[keep]] = 0x0A
    return text


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    import numpy as np
    import torch
    import libfsm_amd as hip
    import extract_ref
    import matches_ref
    import span_ref
    import tokens_ref
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "extract_probe.json")
    size = int(os.environ.get("TEXT_BYTES", 1 << 30))
    torch.cuda.set_device(0)
    starts_auto, (ends_auto, sets) = span_ref.starts_of(WORDS), tokens_ref.trie_lexer(WORDS)
    ids = tokens_ref.state_ids(ends_auto, tokens_ref.EARLIEST, sets)
    none_ld = hip.LinesDfa(span_ref.line_matcher_of([b"\x01\x02\x03"])[0], 0x0A)     # no line matches: inverted, every line is a hit
    starts_pd, ends_td = hip.PosDfa.from_flat(starts_auto[0]), hip.TokDfa.from_flat(ends_auto[0])
    res = {"bytes": size, "device": torch.cuda.get_device_name(0), "sample_lines": SAMPLE, "block_matches": hip.extracted_block_matches(), "cases": {}}

    for which, (lo, hi, seed) in TEXTS.items():
        for kind in ("dense", "sparse"):
            text = make_text(torch, size, lo, hi, seed, kind == "dense")
            torch.cuda.synchronize()
            t = hip.HipText(d_text=text.data_ptr(), nbytes=size, delim=0x0A)
            mt = ends_td.text_matches(starts_pd, t, flags=hip.MATCHES_DROP_EMPTY)
            m = mt.count
            # the judge's matches of the first lines
            off = t.offsets().astype(np.int64)
            raw = text[:int(off[SAMPLE])].cpu().numpy().tobytes()
            raw_lines = [raw[off[i]:off[i + 1]] for i in range(SAMPLE)]
            lines = [x.rstrip(b"\n") for x in raw_lines]
            rows, lens = span_ref.rows_of(lines)
            raw_rows, raws = span_ref.rows_of(raw_lines)
            want_m = matches_ref.matches(starts_auto, ends_auto, rows, lens, matches_ref.DROP_EMPTY, ids=ids)
            want_m = (want_m["off"], want_m["start"], want_m["end"], want_m["id"])
            case = {"lines": t.lines, "matches": mt.total, "seps": {}}
            gather = []
            for name, sep in SEPS.items():
                passes, call_ms, copy_ms, nout = [], [], [], 0
                for rep in range(4):
                    ms, ex = timed(torch, lambda: mt.text_extract(t, sep_byte=sep))
                    call_ms.append(ms)
                    passes.append([ex.pass_ms(k) for k in range(4)])
                    nout = ex.nbytes
                    if rep == 0:    # the judge on the first lines
                        want = extract_ref.extract(raw_rows, lens, raws, want_m, None, False, sep)
                        R = len(want[2])
                        goff, gbytes, gline, gmatch = ex.copy()
                        assert np.array_equal(goff[:R + 1], want[0]), "the device's offsets differ from the judge's on the sample"
                        assert np.array_equal(gbytes[:int(want[0][-1])], want[1]), "the device's bytes differ from the judge's on the sample"
                        assert np.array_equal(gline[:R], want[2]) and np.array_equal(gmatch[:R], want[3]), "line / match differ on the sample"
                        del goff, gbytes, gline, gmatch
                    dst, src = torch.empty(nout, dtype=torch.uint8, device="cuda"), torch.empty(nout, dtype=torch.uint8, device="cuda")
                    copy_ms.append(timed(torch, lambda: dst.copy_(src))[0])
                    del dst, src
                    ex.free()
                    if name == "newline":
                        hits = t.hits(none_ld, invert=True)
                        assert hits.count == m
                        gather.append(hits.gather_ms())
                        hits.close()
                lengths_ms, scan_ms, offsets_ms, write_ms = (min(p[k] for p in passes[1:]) for k in range(4))
                entry = {"out_bytes": nout, "lengths_ms": round(lengths_ms, 4), "scan_ms": round(scan_ms, 4), "offsets_ms": round(offsets_ms, 4),
                         "write_ms": round(write_ms, 4), "call_ms": round(min(call_ms[1:]), 4), "copy_ms": round(min(copy_ms[1:]), 4),
                         "write_over_copy": round(write_ms / min(copy_ms[1:]), 2)}
                case["seps"][name] = entry
                print(which, kind, name, entry, flush=True)
            case["gather_ms"] = round(min(gather[1:]), 4)
            res["cases"]["%s/%s" % (which, kind)] = case
            mt.free()
            t.close()
            del text
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
