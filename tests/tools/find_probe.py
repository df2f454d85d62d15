#!/usr/bin/env python3
"""tests/tools/find_probe.py -- what the lookup of an extracted text's records among the keys of a distinct object costs on one
device (not run by pytest): the four texts of tests/tools/extract_probe.py, TEXT_BYTES (default 1 GiB) of 8-64-byte lines and of
0-1024-byte lines, dense and sparse, and the two extractions of tests/tools/distinct_probe.py -- `ab` (every record is "ab\\n") and
the rule [a-z]+ (`lexer`: the records are the lines, nearly all differ) --, made once and part of no figure.  The cases:
  ab/all       every probe record present, against a dictionary with D = 1 (the key ab);
  lexer/half   the lexer records against the dictionary of their own first half: about half present, a table of R slots or more;
  ab/none, lexer/none   none present: the same dictionaries built WITHOUT a trim byte, so that every key keeps its '\\n' and no
               trimmed probe record equals one -- the chains are walked to their empty slot.
Reported per case, best of three after a warm-up:
  hash_ms, probe_ms, mark_ms, pick_ms   the four passes by the object's own HIP events (fsm_hip_found_pass_ms);
  call_ms                               the whole fsm_hip_keys_find_extracted call between two events on the stream;
Yardsticks, same process, interleaved with the device runs:
  host_ms      (a) what a caller does without it: fsm_hip_extracted_copy of the probe's off and bytes + one Python dict lookup per
               record on one core, run once; every class is checked equal to the device's;
  distinct_ms  (b) the hash and insert passes of fsm_hip_extracted_distinct over the same probe records: the alternative "make the
               probe distinct and compare";
  copy_ms      (c) a device-to-device copy of the probe's bytes.
No figure is a gate and no ratio is fixed in advance.

usage: find_probe.py [out.json]   (default: profiles/find_probe.json)"""
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

from distinct_probe import lexer  # noqa: E402
from extract_probe import TEXTS, WORDS, make_text, timed  # noqa: E402

NL = 0x0A


def main():
    import numpy as np
    import torch
    import libfsm_amd as hip
    from libfsm_amd import capi
    import span_ref
    import tokens_ref
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "find_probe.json")
    size = int(os.environ.get("TEXT_BYTES", 1 << 30))
    torch.cuda.set_device(0)
    lex_starts, lex_ends = lexer(np, hip, span_ref)
    pairs = {"ab": (hip.PosDfa.from_flat(span_ref.starts_of(WORDS)[0]), hip.TokDfa.from_flat(tokens_ref.trie_lexer(WORDS)[0][0])),
             "lexer": (hip.PosDfa.from_flat(lex_starts), hip.TokDfa.from_flat(lex_ends))}
    res = {"bytes": size, "device": torch.cuda.get_device_name(0), "long_bytes": hip.distinct_long_bytes(), "cases": {}}

    for which, (lo, hi, seed) in TEXTS.items():
        for kind in ("dense", "sparse"):
            text = make_text(torch, size, lo, hi, seed, kind == "dense")
            torch.cuda.synchronize()
            t = hip.HipText(d_text=text.data_ptr(), nbytes=size, delim=NL)
            for name, (pd, td) in pairs.items():
                mt = td.text_matches(pd, t, flags=hip.MATCHES_DROP_EMPTY)
                ex = mt.text_extract(t, sep_byte=NL)
                R, nbytes = ex.count, ex.nbytes
                for case in ("all" if name == "ab" else "half", "none"):
                    trim = -1 if case == "none" else NL          # none: the keys keep their '\n'
                    if name == "ab":
                        dx = hip.distinct([0, 3], b"ab\n", trim, None, trim)
                    else:
                        dx = hip.distinct_device(ex.off_ptr, ex.bytes_ptr, R // 2, nbytes, trim, 0, trim, 0, keep=(ex,))
                    torch.cuda.synchronize()
                    passes, call_ms, copy_ms, distinct_ms, host_ms, present = [], [], [], [], None, None
                    for rep in range(4):
                        ms, fx = timed(torch, lambda: dx.find_extracted(ex))
                        call_ms.append(ms)
                        passes.append([fx.pass_ms(k) for k in range(4)])
                        present = fx.present
                        if rep == 1:                                        # the host path, once, between the device runs
                            _, _, _, doff, dbytes = dx.copy()
                            keys, ko = dbytes.tobytes(), doff.tolist()
                            table = {keys[ko[d]:ko[d + 1]]: d for d in range(len(ko) - 1)}
                            cut = 1 if case == "none" else 0            # the probe's trimmed record against keys that kept theirs
                            t0 = time.perf_counter()
                            h_off, h_data = np.empty(R + 1, np.uint64), np.empty(nbytes, np.uint8)
                            capi._call("fsm_hip_extracted_copy", ex.handle, capi._ptr(h_off), capi._ptr(h_data), None, None)
                            raw, o = h_data.tobytes(), h_off.tolist()
                            ends = o[1:] if cut == 0 else [x - 1 for x in o[1:]]
                            h_cls = np.fromiter(map(table.get, map(raw.__getitem__, map(slice, o[:-1], ends)), itertools.repeat(hip.FOUND_NONE)), np.uint32, R)
                            host_ms = (time.perf_counter() - t0) * 1e3
                            assert np.array_equal(fx.copy()[0], h_cls), (which, kind, name, case, "class differs from the dictionary's")
                            del raw, o, ends, h_off, h_data, h_cls, table, keys, ko, doff, dbytes
                        fx.free()
                        other = ex.distinct(NL, hip.DISTINCT_NO_TEXT)
                        torch.cuda.synchronize()
                        distinct_ms.append(other.pass_ms(0) + other.pass_ms(1))
                        other.free()
                        dst, src = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
                        copy_ms.append(timed(torch, lambda: dst.copy_(src))[0])
                        del dst, src
                    hash_ms, probe_ms, mark_ms, pick_ms = (min(p[k] for p in passes[1:]) for k in range(4))
                    best = min(call_ms[1:])
                    entry = {"records": R, "in_bytes": nbytes, "keys": dx.count, "present": present, "hash_ms": round(hash_ms, 4),
                             "probe_ms": round(probe_ms, 4), "mark_ms": round(mark_ms, 4), "pick_ms": round(pick_ms, 4), "call_ms": round(best, 4),
                             "host_ms": round(host_ms, 1), "distinct_ms": round(min(distinct_ms[1:]), 4), "copy_ms": round(min(copy_ms[1:]), 4),
                             "host_over_call": round(host_ms / best, 1), "call_over_copy": round(best / min(copy_ms[1:]), 1)}
                    res["cases"]["%s/%s/%s/%s" % (which, kind, name, case)] = entry
                    print(which, kind, name, case, entry, flush=True)
                    dx.free()
                    torch.cuda.empty_cache()
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
