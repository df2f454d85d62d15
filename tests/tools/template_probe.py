#!/usr/bin/env python3
"""tests/tools/template_probe.py -- what the match inside its replacement costs on one device (not run by pytest): the four texts of
tests/tools/replace_probe.py (TEXT_BYTES, default 1 GiB, of 8-64-byte and of 0-1024-byte lines, dense and sparse in the word ab),
the matches of EVERY line made once and not part of any figure, and three tables that all put four bytes where ab stood:
  tag      the template <&>: two literal bytes, one insert -- two of the four bytes are the match's own;
  twice    the template &&: no literal byte, two inserts at 0 -- all four are;
  plain    the plain table WXYZ: the yardstick, the same output length per match, in the same run.
Reported per case and table, best of three after a warm-up, the three tables interleaved rep by rep in one process:
  lengths_ms, scan_ms, offsets_ms, write_ms   the four passes by the object's own HIP events (fsm_hip_replaced_pass_ms);
  call_ms                                     the whole fsm_hip_text_replace call between two events on the stream;
  write_over_plain, lengths_over_plain, call_over_plain     against the plain table of the same case.
The device's answer is held against the CPU judge (tests/template_ref.py over tests/matches_ref.py) on the first SAMPLE lines.  No
figure is a gate.

usage: template_probe.py [out.json]   (default: profiles/template_probe.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SAMPLE = 1500
TABLES = {"tag": ([b"<>"], [[1]]), "twice": ([b""], [[0, 0]]), "plain": ([b"WXYZ"], None)}


def main():
    import numpy as np
    import torch
    import libfsm_amd as hip
    import matches_ref
    import span_ref
    import template_ref
    import tokens_ref
    from replace_probe import TEXTS, WORDS, make_text, timed
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "template_probe.json")
    size = int(os.environ.get("TEXT_BYTES", 1 << 30))
    torch.cuda.set_device(0)
    starts_auto, (ends_auto, sets) = span_ref.starts_of(WORDS), tokens_ref.trie_lexer(WORDS)
    ids = tokens_ref.state_ids(ends_auto, tokens_ref.EARLIEST, sets)
    starts_pd, ends_td = hip.PosDfa.from_flat(starts_auto[0]), hip.TokDfa.from_flat(ends_auto[0])
    repls = {k: hip.HipRepl.template(tab, ins) if ins is not None else hip.HipRepl(tab) for k, (tab, ins) in TABLES.items()}
    assert [repls[k].inserts for k in TABLES] == [1, 2, 0] and all(rp.in_lds for rp in repls.values())
    res = {"bytes": size, "device": torch.cuda.get_device_name(0), "sample_lines": SAMPLE, "cases": {}}

    for which, (lo, hi, seed) in TEXTS.items():
        for kind in ("dense", "sparse"):
            text = make_text(torch, size, lo, hi, seed, kind == "dense")
            torch.cuda.synchronize()
            t = hip.HipText(d_text=text.data_ptr(), nbytes=size, delim=0x0A)
            mt = ends_td.text_matches(starts_pd, t, flags=hip.MATCHES_DROP_EMPTY)
            off = t.offsets().astype(np.int64)
            raw = text[:int(off[SAMPLE])].cpu().numpy().tobytes()
            raw_lines = [raw[off[i]:off[i + 1]] for i in range(SAMPLE)]
            rows, lens = span_ref.rows_of([x.rstrip(b"\n") for x in raw_lines])
            raw_rows, raws = span_ref.rows_of(raw_lines)
            want_m = matches_ref.matches(starts_auto, ends_auto, rows, lens, matches_ref.DROP_EMPTY, ids=ids)
            want_m = (want_m["off"], want_m["start"], want_m["end"], want_m["id"])
            passes, calls, nout = {k: [] for k in TABLES}, {k: [] for k in TABLES}, {}
            for rep in range(4):                         # rep 0 is the warm-up and the judged one
                for name, rp in repls.items():
                    ms, rd = timed(torch, lambda: mt.text_replace(rp, t))
                    calls[name].append(ms)
                    passes[name].append([rd.pass_ms(k) for k in range(4)])
                    nout[name] = rd.nbytes
                    if rep == 0:
                        want = template_ref.replace(raw_rows, lens, raws, want_m, *TABLES[name])
                        goff, gbytes = rd.copy()
                        assert np.array_equal(goff[:SAMPLE + 1], want[0]), "the device's offsets differ from the judge's on the sample"
                        assert np.array_equal(gbytes[:int(want[0][-1])], want[1]), "the device's bytes differ from the judge's on the sample"
                        del goff, gbytes
                    rd.free()
            assert len(set(nout.values())) == 1          # four bytes per match, whichever table
            case = {"lines": t.lines, "matches": mt.total, "out_bytes": nout["plain"], "tables": {}}
            for name in TABLES:
                lengths_ms, scan_ms, offsets_ms, write_ms = (min(p[k] for p in passes[name][1:]) for k in range(4))
                case["tables"][name] = {"lengths_ms": round(lengths_ms, 4), "scan_ms": round(scan_ms, 4), "offsets_ms": round(offsets_ms, 4),
                                        "write_ms": round(write_ms, 4), "call_ms": round(min(calls[name][1:]), 4),
                                        "write_ms_repeats": [round(p[3], 4) for p in passes[name][1:]]}
            plain = case["tables"]["plain"]
            for name in ("tag", "twice"):
                e = case["tables"][name]
                e["write_over_plain"] = round(e["write_ms"] / plain["write_ms"], 3)
                e["lengths_over_plain"] = round(e["lengths_ms"] / plain["lengths_ms"], 3)
                e["call_over_plain"] = round(e["call_ms"] / plain["call_ms"], 3)
            for name in TABLES:
                print(which, kind, name, case["tables"][name], flush=True)
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
