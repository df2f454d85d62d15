#!/usr/bin/env python3
"""tests/tools/distinct_probe.py -- what the distinct records of an extracted text cost on one device (not run by pytest): the
four texts of tests/tools/extract_probe.py, TEXT_BYTES (default 1 GiB) of 8-64-byte lines and of 0-1024-byte lines, dense (a text
over abcd) and sparse (a text over c .. z with ab at the head of every line).  Two cases per text, the records being
fsm_hip_text_extract's with '\\n' behind each, made once and part of no figure:
  ab       the word ab: every record is "ab\\n", ONE key -- the hot-key worst case: every wavefront's insert meets one slot and adds
           to one counter;
  lexer    the rule [a-z]+ : a line of letters is one token, so the records are the lines and nearly all of them differ -- the
           table-traffic worst case: every record claims a slot of its own.
Reported per case, best of three after a warm-up:
  hash_ms, insert_ms, number_ms, write_ms   the four passes by the object's own HIP events (fsm_hip_distinct_pass_ms); insert
                                            includes the clearing of the table and the counters;
  call_ms                                   the whole fsm_hip_extracted_distinct call between two events on the stream: the passes
                                            AND the host's wait for D and the allocations;
  host_ms                                   what a caller does without it, same process, between the device runs:
                                            fsm_hip_extracted_copy of off and the bytes + a Python dictionary (collections.Counter)
                                            over the records, one core, whole path, run once;
  copy_ms                                   a device-to-device copy of the input bytes.
Cross-check: D, and count[D] in the order of first appearance, equal the dictionary's (which keeps insertion order); the first
1 000 keys equal its first 1 000.  No figure is a gate and no ratio is fixed in advance.

usage: distinct_probe.py [out.json]   (default: profiles/distinct_probe.json)"""
import collections
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

from extract_probe import TEXTS, WORDS, make_text, timed  # noqa: E402

NL = 0x0A


def lexer(np, hip, span_ref):
    """(starts, ends) of [a-z]+: a match may begin at every letter and ends behind the last letter of its run"""
    dense = np.full((2, 256), -1, np.int64)
    dense[:, 97:123] = 1
    ends = hip.FlatDfa.from_dense(dense, 0, np.array([0, 1], np.uint8), endids={1: [0]})
    return span_ref.starts_of([bytes([c]) for c in range(97, 123)])[0], ends


def main():
    import numpy as np
    import torch
    import libfsm_amd as hip
    from libfsm_amd import capi
    import span_ref
    import tokens_ref
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "distinct_probe.json")
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
                passes, call_ms, copy_ms, host_ms = [], [], [], None
                for rep in range(4):
                    ms, dx = timed(torch, lambda: ex.distinct(NL))
                    call_ms.append(ms)
                    passes.append([dx.pass_ms(k) for k in range(4)])
                    if rep == 1:                                            # the host path, once, between the device runs
                        t0 = time.perf_counter()
                        h_off, h_data = np.empty(R + 1, np.uint64), np.empty(nbytes, np.uint8)
                        capi._call("fsm_hip_extracted_copy", ex.handle, capi._ptr(h_off), capi._ptr(h_data), None, None)
                        raw, o = h_data.tobytes(), h_off.tolist()
                        table = collections.Counter(map(raw.__getitem__, map(slice, o[:-1], o[1:])))
                        host_ms = (time.perf_counter() - t0) * 1e3
                        del raw, o, h_off, h_data
                        D = dx.count
                        _, count, _, doff, dbytes = dx.copy()
                        assert D == len(table), (which, kind, name, "D differs from the dictionary's", D, len(table))
                        assert np.array_equal(count, np.fromiter(table.values(), np.uint64, D)), "count differs from the dictionary's"
                        keys = dbytes.tobytes()
                        assert [keys[int(doff[d]):int(doff[d + 1])] for d in range(min(D, 1000))] == list(table)[:1000], "the first keys differ"
                        del table, count, doff, dbytes, keys
                    dst, src = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
                    copy_ms.append(timed(torch, lambda: dst.copy_(src))[0])
                    del dst, src
                    key_bytes = dx.nbytes
                    dx.free()
                hash_ms, insert_ms, number_ms, write_ms = (min(p[k] for p in passes[1:]) for k in range(4))
                best = min(call_ms[1:])
                entry = {"records": R, "in_bytes": nbytes, "distinct": D, "key_bytes": key_bytes, "hash_ms": round(hash_ms, 4),
                         "insert_ms": round(insert_ms, 4), "number_ms": round(number_ms, 4), "write_ms": round(write_ms, 4), "call_ms": round(best, 4),
                         "host_ms": round(host_ms, 1), "copy_ms": round(min(copy_ms[1:]), 4), "host_over_call": round(host_ms / best, 1),
                         "call_over_copy": round(best / min(copy_ms[1:]), 1)}
                res["cases"]["%s/%s/%s" % (which, kind, name)] = entry
                print(which, kind, name, entry, flush=True)
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
