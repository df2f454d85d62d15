#!/usr/bin/env python3
"""tests/tools/tally_probe.py -- what counting every match per rule and per group costs on one device (not run by pytest): the four
texts of tests/tools/extract_probe.py, TEXT_BYTES (default 1 GiB) of 8-64-byte lines and of 0-1024-byte lines, the word ab, dense
(about one match per 16 bytes) and sparse (one match per line).  The matches are fsm_hip_text_matches' over EVERY line
(DROP_EMPTY); they are made once per text and are not part of any figure.
Cases, each as count alone, lines alone and both, each timed between two events on the stream, best of three after a warm-up:
  one_group      the matches' own ids -- all rule 0, the hot bin -- into a table of 1 025 columns, one group
  groups_1000    the same into 1 000 groups of equally many inputs
  one_rule       the same with nrules = 1: two columns
  random_1024    the ids replaced by random ids below 1 024 (fsm_hip_tally_ids_device over the matches' off): counters in LDS
  random_100000  ... below 100 000: above the LDS cap, every entry adds to the table.  count alone has 100 001 columns; lines needs
                 C <= fsm_hip_tally_max_line_columns(), so lines and both run with nrules = that cap - 1 and the rest in "other"
Yardsticks, same process, interleaved, neither a target:
  host_ms        what a caller does without the tally: fsm_hip_matches_copy of off and id to the host + np.bincount, whole path
  copy_ms        a device-to-device copy of id[total] and off[m + 1]: the bytes the kernel must read
Cross-checks: count of every case equals np.bincount over a host copy of the ids (per group through the copied off); lines of
the cases over the matches' own ids equals the inputs with a match per group; lines of the random cases equals tests/tally_ref.py
on the first SAMPLE inputs.  No figure is a gate and no ratio is fixed in advance.

usage: tally_probe.py [out.json]   (default: profiles/tally_probe.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

from extract_probe import TEXTS, WORDS, make_text  # noqa: E402

SAMPLE = 1500
FORMS = {"count": (True, False), "lines": (False, True), "both": (True, True)}


def main():
    import numpy as np
    import torch
    import libfsm_amd as hip
    from libfsm_amd import capi
    import span_ref
    import tally_ref
    import tokens_ref
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tally_probe.json")
    size = int(os.environ.get("TEXT_BYTES", 1 << 30))
    torch.cuda.set_device(0)
    starts_auto, (ends_auto, _) = span_ref.starts_of(WORDS), tokens_ref.trie_lexer(WORDS)
    starts_pd, ends_td = hip.PosDfa.from_flat(starts_auto[0]), hip.TokDfa.from_flat(ends_auto[0])
    line_cap = hip.tally_max_line_columns()
    res = {"bytes": size, "device": torch.cuda.get_device_name(0), "window": hip.tally_window(), "span_inputs": hip.tally_span_inputs(),
           "lds_columns": hip.tally_lds_columns(), "max_line_columns": line_cap, "cases": {}}

    def timed(fn, reps=3):
        best = None
        for rep in range(reps + 1):                                         # the first: a warm-up
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if rep:
                best = a.elapsed_time(b) if best is None else min(best, a.elapsed_time(b))
        return best

    for which, (lo, hi, seed) in TEXTS.items():
        for kind in ("dense", "sparse"):
            text = make_text(torch, size, lo, hi, seed, kind == "dense")
            torch.cuda.synchronize()
            t = hip.HipText(d_text=text.data_ptr(), nbytes=size, delim=0x0A)
            mt = ends_td.text_matches(starts_pd, t, flags=hip.MATCHES_DROP_EMPTY)
            m, total = mt.count, mt.total
            case = {"lines": m, "matches": total, "runs": {}}

            # the two yardsticks, three times each, interleaved
            host_ms, copy_ms = [], []
            h_off, h_id = np.empty(m + 1, np.uint64), np.empty(total, np.uint32)
            src_id, dst_id = torch.empty(total, dtype=torch.int32, device="cuda"), torch.empty(total, dtype=torch.int32, device="cuda")
            src_off, dst_off = torch.empty(m + 1, dtype=torch.int64, device="cuda"), torch.empty(m + 1, dtype=torch.int64, device="cuda")
            for rep in range(4):
                t0 = time.perf_counter()
                capi._call("fsm_hip_matches_copy", mt.handle, capi._ptr(h_off), None, None, capi._ptr(h_id))
                by_rule = np.bincount(h_id, minlength=2)
                host_ms.append((time.perf_counter() - t0) * 1e3)
                copy_ms.append(timed(lambda: (dst_id.copy_(src_id), dst_off.copy_(src_off)), reps=1))
            del src_id, dst_id, src_off, dst_off
            assert by_rule.tolist() == [total, 0] or total == 0
            case["host_ms"], case["copy_ms"] = round(min(host_ms[1:]), 3), round(min(copy_ms[1:]), 4)
            per_input = np.diff(h_off.astype(np.int64))
            goff = np.linspace(0, m, 1001).astype(np.uint64)
            d_goff = torch.from_numpy(goff.view(np.int64).copy()).cuda()
            group_of_input = np.searchsorted(goff[:1000], np.arange(m), "right") - 1
            with_match = np.bincount(group_of_input[per_input > 0], minlength=1000)
            per_group = np.add.reduceat(np.concatenate([per_input, [0]]), np.minimum(goff[:1000].astype(np.int64), m))
            per_group[np.diff(goff.astype(np.int64)) == 0] = 0

            g = torch.Generator(device="cuda")
            g.manual_seed(seed + 100)
            random_ids = {top: torch.randint(0, top, (max(total, 1),), device="cuda", generator=g, dtype=torch.int32) for top in (1024, 100000)}

            def run(name, form, nrules, G, ids=None):
                """one case in one form: timed, read back, checked"""
                Cn = nrules + 1
                tabs = [torch.empty(G * Cn, dtype=torch.int64, device="cuda") if w else None for w in FORMS[form]]
                ptrs = [x.data_ptr() if x is not None else 0 for x in tabs]
                gp = d_goff.data_ptr() if G > 1 else 0
                if ids is None:
                    ms = timed(lambda: mt.tally_device(gp, G if gp else 0, nrules, ptrs[0], ptrs[1]))
                else:
                    ms = timed(lambda: hip.tally_ids_device(mt.off_ptr, ids.data_ptr(), m, total, gp, G if gp else 0, nrules, ptrs[0], ptrs[1]))
                got = [x.cpu().numpy().view(np.uint64).reshape(G, Cn) if x is not None else None for x in tabs]
                host_ids = h_id if ids is None else ids[:total].cpu().numpy().view(np.uint32)
                if got[0] is not None:
                    if G == 1:
                        want = np.bincount(np.minimum(host_ids, nrules), minlength=Cn)[None, :]
                    else:
                        want = np.zeros((G, Cn), np.int64)
                        want[:, 0] = per_group
                    assert np.array_equal(got[0], want.astype(np.uint64)), (name, form, "count differs from np.bincount")
                if got[1] is not None:
                    if ids is None:
                        want = np.zeros((G, Cn), np.int64)
                        want[:, 0] = with_match if G > 1 else int((per_input > 0).sum())
                        assert np.array_equal(got[1], want.astype(np.uint64)), (name, form, "lines differs from the inputs with a match")
                    else:                                                   # the judge on the first inputs
                        n = min(SAMPLE, m)
                        k = int(h_off[n])
                        small = torch.empty(Cn, dtype=torch.int64, device="cuda")
                        hip.tally_ids_device(mt.off_ptr, ids.data_ptr(), n, k, 0, 0, nrules, 0, small.data_ptr())
                        torch.cuda.synchronize()
                        want = tally_ref.tally(h_off[:n + 1], host_ids[:k], nrules)[1]
                        assert np.array_equal(small.cpu().numpy().view(np.uint64)[None, :], want), (name, form, "lines differs from the judge on the sample")
                entry = {"nrules": nrules, "groups": G, "ms": round(ms, 4), "over_copy": round(ms / case["copy_ms"], 2),
                         "host_over": round(case["host_ms"] / ms, 1)}
                case["runs"].setdefault(name, {})[form] = entry
                print(which, kind, name, form, entry, flush=True)

            for form in FORMS:
                run("one_group", form, 1024, 1)
                run("groups_1000", form, 1, 1000)
                run("one_rule", form, 1, 1)
                run("random_1024", form, 1024, 1, random_ids[1024])
                run("random_100000", form, 100000 if form == "count" else line_cap - 1, 1, random_ids[100000])
            res["cases"]["%s/%s" % (which, kind)] = case
            mt.free()
            t.close()
            del text, random_ids, d_goff
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
