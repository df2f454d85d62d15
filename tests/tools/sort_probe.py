#!/usr/bin/env python3
"""tests/tools/sort_probe.py -- what the sort of an extracted text costs on one device (not run by pytest): the four texts of
tests/tools/distinct_probe.py, TEXT_BYTES (default 1 GiB), and its two extractions, the records being fsm_hip_text_extract's with
'\\n' behind each, made once and part of no figure:
  ab       the word ab: every record is "ab\\n" -- one bucket that one round closes;
  lexer    the rule [a-z]+ : the records are the lines and nearly all of them differ.
Per extraction three sorts: the R records (fsm_hip_extracted_sort), and the D keys of their distinct object plain and by count
(fsm_hip_keys_sort, FSM_HIP_SORT_BY_COUNT).  Reported per sort, best of three after a warm-up:
  keys_ms, radix_ms, rebucket_ms, write_ms   the four passes by the object's own HIP events (fsm_hip_sorted_pass_ms), the first
                                             three summed over the rounds;
  call_ms                                    the whole call between two events on the stream: the passes AND a wait a round;
  rounds, passes_run, passes_skipped         fsm_hip_sorted_rounds and fsm_hip_sorted_radix_passes;
  host_ms                                    what a caller does without it, same process, between the device runs: _copy of off
                                             and the bytes + sorted() over the records on one core, whole path, run once;
  copy_ms                                    a device-to-device copy of the bytes one radix pass moves: 4 bytes a record.
Cross-check: order and groups equal the host path's.  No figure is a gate and no ratio is fixed in advance.

usage: sort_probe.py [out.json]   (default: profiles/sort_probe.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

from distinct_probe import NL, lexer  # noqa: E402
from extract_probe import TEXTS, WORDS, make_text, timed  # noqa: E402


def host_sort(np, off, data, major):
    """(order, groups) of the records off / data with their last byte trimmed, by sorted() on one core"""
    raw, o = data.tobytes(), off.tolist()
    keys = [raw[a:b - 1] for a, b in zip(o[:-1], o[1:])]
    if major is None:
        order = sorted(range(len(keys)), key=keys.__getitem__)
        groups = len(set(keys))
    else:
        mj = major.tolist()
        order = sorted(range(len(keys)), key=lambda r: (-mj[r], keys[r]))
        groups = len(set(zip(mj, keys)))
    return np.array(order, np.uint64), groups


def probe(np, torch, make, copy_out, major):
    """one sort four times: -> the entry"""
    passes, call_ms, copy_ms, host_ms = [], [], [], None
    for rep in range(4):
        ms, sx = timed(torch, make)
        call_ms.append(ms)
        passes.append([sx.pass_ms(k) for k in range(4)])
        R, rounds, run, skipped, nbytes = sx.records, sx.rounds, sx.radix_passes(), sx.radix_passes(True), sx.nbytes
        if rep == 1:                                                    # the host path, once, between the device runs
            t0 = time.perf_counter()
            h_off, h_data = copy_out()
            order, groups = host_sort(np, h_off, h_data, major)
            host_ms = (time.perf_counter() - t0) * 1e3
            got = sx.copy()[0]
            assert np.array_equal(got, order), "order differs from sorted()'s"
            assert sx.groups == groups, ("groups", sx.groups, groups)
            del h_off, h_data, order, got
        dst, src = torch.empty(max(R, 1), dtype=torch.int32, device="cuda"), torch.empty(max(R, 1), dtype=torch.int32, device="cuda")
        copy_ms.append(timed(torch, lambda: dst.copy_(src))[0])
        del dst, src
        sx.free()
    keys_ms, radix_ms, rebucket_ms, write_ms = (min(p[k] for p in passes[1:]) for k in range(4))
    best = min(call_ms[1:])
    return {"records": R, "out_bytes": nbytes, "rounds": rounds, "passes_run": run, "passes_skipped": skipped, "keys_ms": round(keys_ms, 4),
            "radix_ms": round(radix_ms, 4), "rebucket_ms": round(rebucket_ms, 4), "write_ms": round(write_ms, 4), "call_ms": round(best, 4),
            "host_ms": round(host_ms, 1), "copy_ms": round(min(copy_ms[1:]), 4), "host_over_call": round(host_ms / best, 1)}


def main():
    import numpy as np
    import torch
    import libfsm_amd as hip
    from libfsm_amd import capi
    import span_ref
    import tokens_ref
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sort_probe.json")
    size = int(os.environ.get("TEXT_BYTES", 1 << 30))
    torch.cuda.set_device(0)
    lex_starts, lex_ends = lexer(np, hip, span_ref)
    pairs = {"ab": (hip.PosDfa.from_flat(span_ref.starts_of(WORDS)[0]), hip.TokDfa.from_flat(tokens_ref.trie_lexer(WORDS)[0][0])),
             "lexer": (hip.PosDfa.from_flat(lex_starts), hip.TokDfa.from_flat(lex_ends))}
    res = {"bytes": size, "device": torch.cuda.get_device_name(0), "tile_records": hip.sort_tile_records(), "cases": {}}

    for which, (lo, hi, seed) in TEXTS.items():
        for kind in ("dense", "sparse"):
            text = make_text(torch, size, lo, hi, seed, kind == "dense")
            torch.cuda.synchronize()
            t = hip.HipText(d_text=text.data_ptr(), nbytes=size, delim=NL)
            for name, (pd, td) in pairs.items():
                mt = td.text_matches(pd, t, flags=hip.MATCHES_DROP_EMPTY)
                ex = mt.text_extract(t, sep_byte=NL)
                dx = ex.distinct(NL)

                def records_out():
                    h_off, h_data = np.empty(ex.count + 1, np.uint64), np.empty(ex.nbytes, np.uint8)
                    capi._call("fsm_hip_extracted_copy", ex.handle, capi._ptr(h_off), capi._ptr(h_data), None, None)
                    return h_off, h_data

                def keys_out():
                    _, _, _, doff, dbytes = dx.copy()
                    return doff, dbytes

                count = dx.copy()[1]
                for what, make, out, major in (("records", lambda: ex.sort(NL), records_out, None), ("keys", lambda: dx.sort(sep_byte=NL), keys_out, None),
                                               ("keys by count", lambda: dx.sort(by_count=True, sep_byte=NL), keys_out, count)):
                    entry = probe(np, torch, make, out, major)
                    res["cases"]["%s/%s/%s/%s" % (which, kind, name, what)] = entry
                    print(which, kind, name, what, entry, flush=True)
                dx.free()
                ex.free()
                mt.free()
                torch.cuda.empty_cache()
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
