#!/usr/bin/env python3
"""tests/tools/matches_probe.py -- what listing every match of every hit costs in one call, against the rounds, on one
device (not run by pytest): TEXT_BYTES (default 1 GiB) of 8-64-byte lines and of 0-1024-byte lines, the word ab, with
  dense    a text over abcd, uniform: ab begins at one position in 16, so about one match per 16 bytes;
  sparse   a text over c .. z with ab planted at the head of every line of two bytes or more: one match per line.
The lines are the hits of .*ab.* (FSM_HIP_HITS_NO_BYTES).  Reported per case:
  mark_ms, count_ms, scan_ms, emit_ms   the four passes by the object's own HIP events (fsm_hip_matches_pass_ms), best of three
                                        after a warm-up;
  matches, matches_per_s                over the four passes;
  call_ms                               the whole fsm_hip_text_matches call between two events on the stream: the four passes AND
                                        what the events of the passes leave out -- the host's wait for the total and the allocation
                                        of the three output arrays; best of three;
  scan_share                            scan_ms over the four passes (one workgroup: it dominates on short lines, as for tokens);
  rounds, rounds_ms                     the same hits advanced with fsm_hip_text_spans_next until fsm_hip_text_spans_count is 0,
                                        the whole loop between two events (its waits included: they are part of that path),
                                        in the same process, the runs interleaved with the one-call runs, best of three;
                                        the object's creation included, its release not -- as for call_ms;
  rounds_over_call                      rounds_ms / call_ms: like against like, both whole paths by the same two events;
  rounds_over_passes                    rounds_ms / (mark + count + scan + emit): the rounds' whole path against the one call's
                                        device work alone -- it flatters the one call, read rounds_over_call;
  walk_pos_back_ms, mark_over_pos       walk_pos<true> over the same lines with the same table, last asked for, and mark_ms over it.
The device's answer is held against the CPU judge (tests/matches_ref.py) on the first SAMPLE hits.  No figure is a gate.

usage: matches_probe.py [out.json]   (default: profiles/matches_probe.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TEXTS = {"8_64": (8, 64, 5), "0_1024": (0, 1024, 6)}
WORDS = [b"ab"]
SAMPLE = 1500


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
    import matches_ref
    import span_ref
    import tokens_ref
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "matches_probe.json")
    size = int(os.environ.get("TEXT_BYTES", 1 << 30))
    torch.cuda.set_device(0)
    starts_auto, (ends_auto, sets) = span_ref.starts_of(WORDS), tokens_ref.trie_lexer(WORDS)
    ids = tokens_ref.state_ids(ends_auto, tokens_ref.EARLIEST, sets)
    ld = hip.LinesDfa(span_ref.line_matcher_of(WORDS)[0], 0x0A)
    starts_pd, ends_pd, ends_td = hip.PosDfa.from_flat(starts_auto[0]), hip.PosDfa.from_flat(ends_auto[0]), hip.TokDfa.from_flat(ends_auto[0])
    assert starts_pd.in_lds and ends_td.in_lds
    res = {"bytes": size, "device": torch.cuda.get_device_name(0), "sample_hits": SAMPLE, "cases": {}}

    def rounds(hits):
        sp = hip.HipSpans(hits, starts_pd, ends_pd)
        k = 0
        while sp.count != 0:
            sp.next()
            k += 1
        return k, sp

    for which, (lo, hi, seed) in TEXTS.items():
        for kind in ("dense", "sparse"):
            text = make_text(torch, size, lo, hi, seed, kind == "dense")
            torch.cuda.synchronize()
            t = hip.HipText(d_text=text.data_ptr(), nbytes=size, delim=0x0A)
            hits = t.hits(ld, want_bytes=False)
            m = hits.count
            passes, call_ms, rounds_ms, nrounds, total = [], [], [], 0, 0
            for rep in range(4):
                ms, mt = timed(torch, lambda: ends_td.text_matches(starts_pd, t, hits, flags=hip.MATCHES_DROP_EMPTY))
                call_ms.append(ms)
                passes.append([mt.pass_ms(k) for k in range(4)])
                total = mt.total
                if rep == 0:    # the judge on the first hits
                    picks = hits.lines()[:SAMPLE].astype(np.int64)
                    off = t.offsets().astype(np.int64)
                    raw = text[:int(off[picks[-1] + 1])].cpu().numpy().tobytes()
                    lines = [raw[off[i]:off[i + 1]].rstrip(b"\n") for i in picks]
                    want = matches_ref.matches(starts_auto, ends_auto, *span_ref.rows_of(lines), matches_ref.DROP_EMPTY, ids=ids)
                    goff = np.empty(m + 1, np.uint64)
                    hip.capi._call("fsm_hip_matches_copy", mt.handle, hip.capi._ptr(goff), None, None, None)
                    assert np.array_equal(goff[:len(lines) + 1], want["off"]), "the device's counts differ from the judge's on the sample"
                mt.free()
                ms, (nrounds, sp) = timed(torch, lambda: rounds(hits))
                sp.close()
                rounds_ms.append(ms)
            last = torch.empty(m, dtype=torch.int64, device="cuda")
            pos_ms = min(timed(torch, lambda: starts_pd.accept_pos_device(text.data_ptr(), t.d_off, t.lines, 0, last.data_ptr(), d_pick=hits.lines_device,
                                                                           m=m, trim_byte=0x0A, backward=True, limit=size))[0] for _ in range(4))
            mark_ms, count_ms, scan_ms, emit_ms = (min(p[k] for p in passes[1:]) for k in range(4))
            all_ms = mark_ms + count_ms + scan_ms + emit_ms
            case = {"lines": t.lines, "hits": m, "matches": total, "mark_ms": round(mark_ms, 4), "count_ms": round(count_ms, 4),
                    "scan_ms": round(scan_ms, 4), "emit_ms": round(emit_ms, 4), "matches_per_s": round(total / (all_ms * 1e-3)),
                    "scan_share": round(scan_ms / all_ms, 3), "call_ms": round(min(call_ms[1:]), 4), "rounds": nrounds,
                    "rounds_ms": round(min(rounds_ms[1:]), 4), "rounds_over_call": round(min(rounds_ms[1:]) / min(call_ms[1:]), 2),
                    "rounds_over_passes": round(min(rounds_ms[1:]) / all_ms, 2), "walk_pos_back_ms": round(pos_ms, 4),
                    "mark_over_pos": round(mark_ms / pos_ms, 3)}
            res["cases"]["%s/%s" % (which, kind)] = case
            print(which, kind, case, flush=True)
            hits.close()
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
