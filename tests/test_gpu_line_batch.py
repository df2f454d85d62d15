"""GPU: the three entry forms of the text fronts pinned to each other (libfsm_amd/csrc/line_batch.h and its users in tok.hip, match.hip,
replace.hip and span.hip): the host form on NumPy arrays, the _device form on the same arrays uploaded (limit = the text's bytes, and limit = 0)
and the fsm_hip_text_* form on a text of the same bytes give equal arrays, and these are the Python references' (tokens_ref,
matches_ref, replace_ref, span_ref).  One text of 5 lines, one of them empty, the last without a delimiter; then a pick with a
repeat, and, for the text form, the hits of a lines DFA.  Last, what all four host forms refuse about a batch."""
import ctypes as C
import errno

import numpy as np
import pytest

import matches_ref
import replace_ref
import span_ref
import tokens_ref
from tokens_ref import EARLIEST

pytestmark = pytest.mark.gpu

TEXT = b"ab\n\nxab ab\nb\nab"
NL = 0x0A
RAW = [b"ab\n", b"\n", b"xab ab\n", b"b\n", b"ab"]             # the lines with their delimiters
LINES = [x.rstrip(b"\n") for x in RAW]
BASE = np.frombuffer(TEXT, np.uint8)
OFF = np.array([0, 3, 4, 11, 13, 15], np.uint64)
N, NBYTES = 5, len(TEXT)
PICK = np.array([4, 0, 0, 2], np.uint64)
HIT_LINES = np.array([0, 2, 4], np.uint64)                   # the lines that hold ab
LEXER = [b"ab", b"x", b" "]                                  # the tokens' words: line 3, a lone b, has no token
WORD = [b"ab"]                                               # the matches' word
TABLE = [b"<ab>", b"-"]                                      # the replacements of rule 0 and rule 1
ROWS, LENS = span_ref.rows_of(LINES)
RAW_ROWS, RAWS = span_ref.rows_of(RAW)


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()   # raises if the HIP extension is missing: no silent fallback
    return libfsm_amd


@pytest.fixture(scope="module")
def made(hip):
    """the images, the text and its hits, the uploaded arrays and the references over all five lines: made once, left unchanged"""
    import torch
    lexer, lexer_sets = tokens_ref.trie_lexer(LEXER)
    ends, ends_sets = tokens_ref.trie_lexer(WORD)
    starts = span_ref.starts_of(WORD)
    u64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()   # noqa: E731
    text = hip.HipText(TEXT, NL)
    hits = text.hits(hip.LinesDfa(span_ref.line_matcher_of(WORD)[0], NL))
    assert text.lines == N and np.array_equal(hits.lines(), HIT_LINES)
    res = matches_ref.matches(starts, ends, ROWS, LENS, ids=tokens_ref.state_ids(ends, EARLIEST, ends_sets))
    assert int(res["off"][-1]) == 4 and len(set(res["off"])) < N + 1      # some line has no match, some has two
    return dict(td=hip.TokDfa.from_flat(lexer[0]), starts_pd=hip.PosDfa.from_flat(starts[0]), ends_td=hip.TokDfa.from_flat(ends[0]),
                ends_pd=hip.PosDfa.from_flat(ends[0]), repl=hip.HipRepl(TABLE), text=text, hits=hits, starts=starts, ends=ends,
                d_base=torch.from_numpy(BASE.copy()).cuda(), d_off=u64(OFF), d_pick=u64(PICK),
                tokens=tokens_ref.Judge(lexer, ROWS, LENS).run(0, tokens_ref.state_ids(lexer, EARLIEST, lexer_sets)), matches=res)


def same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(np.asarray(g), np.asarray(w)), (what, k, g, w)


@pytest.mark.parametrize("pick", [False, True], ids=["every line", "a pick"])
def test_tokens_by_every_form(hip, made, pick):
    td, r = made["td"], made["tokens"]
    sel = PICK if pick else None
    dp, m = (made["d_pick"].data_ptr(), len(PICK)) if pick else (0, 0)
    want = tokens_ref.select(r, PICK) if pick else (r["off"], r["end"], r["id"], r["err"])
    assert int(want[0][-1]) > 0 and (pick or (want[3] != tokens_ref.NO_POS).any())   # there are tokens, and a line that stops at a bad byte
    runs = [("host", lambda: td.tokens(BASE, OFF, sel, trim_byte=NL))]
    for limit in (NBYTES, 0):
        runs.append(("device, limit = %d" % limit,
                     lambda limit=limit: td.tokens_device(made["d_base"].data_ptr(), made["d_off"].data_ptr(), N, dp, m, trim_byte=NL, limit=limit)))
    for what, run in runs:
        tk = run()
        same(tk.copy(), want, ("tokens", what))
        tk.close()
    hits = made["hits"] if pick else None
    tk = td.text_tokens(made["text"], hits)
    same(tk.copy(), tokens_ref.select(r, HIT_LINES) if pick else want, ("tokens", "text"))
    tk.close()


@pytest.mark.parametrize("pick", [False, True], ids=["every line", "a pick"])
def test_matches_and_replace_by_every_form(hip, made, pick):
    pd, td, rp, res = made["starts_pd"], made["ends_td"], made["repl"], made["matches"]
    sel = PICK if pick else None
    d_base, d_off, dp, m = made["d_base"].data_ptr(), made["d_off"].data_ptr(), (made["d_pick"].data_ptr() if pick else 0), (len(PICK) if pick else 0)

    def wanted(lines):
        mw = matches_ref.select(res, lines)
        idx = np.asarray(lines, np.int64)
        return mw, replace_ref.replace(RAW_ROWS[idx], LENS[idx], RAWS[idx], mw, TABLE)

    mw, rw = wanted(PICK if pick else np.arange(N))
    assert int(mw[0][-1]) > 0 and len(rw[1]) > int(RAWS[np.asarray(PICK if pick else np.arange(N), np.int64)].sum())   # matches, and lines that grow
    runs = [("host", lambda: hip.HipMatches.run(pd, td, BASE, OFF, sel, trim_byte=NL), lambda mt: mt.replace(rp, BASE, OFF, sel, trim_byte=NL))]
    for limit in (NBYTES, 0):
        runs.append(("device, limit = %d" % limit,
                     lambda limit=limit: hip.HipMatches.run_device(pd, td, d_base, d_off, N, dp, m, trim_byte=NL, limit=limit),
                     lambda mt, limit=limit: mt.replace_device(rp, d_base, d_off, N, dp, m, trim_byte=NL, limit=limit)))
    for what, run, replace in runs:
        mt = run()
        same(mt.copy(), mw, ("matches", what))
        rd = replace(mt)
        same(rd.copy(), rw, ("replace", what))
        rd.free()
        mt.free()
    hits = made["hits"] if pick else None
    if pick:
        mw, rw = wanted(HIT_LINES)
    mt = td.text_matches(pd, made["text"], hits)
    same(mt.copy(), mw, ("matches", "text"))
    rd = mt.text_replace(rp, made["text"], hits)
    same(rd.copy(), rw, ("replace", "text"))
    rd.free()
    mt.free()


@pytest.mark.parametrize("pick", [False, True], ids=["every line", "a pick"])
def test_spans_host_against_device(hip, made, pick):
    import torch
    sel = PICK if pick else None
    idx = np.asarray(PICK if pick else np.arange(N), np.int64)
    dp, m = (made["d_pick"].data_ptr(), len(PICK)) if pick else (0, 0)
    for pd, auto, back in ((made["ends_pd"], made["ends"], False), (made["starts_pd"], made["starts"], True)):
        want = span_ref.accept_pos(auto, ROWS[idx], LENS[idx], back=back)
        assert (want[1] != span_ref.NO_POS).any() and (pick or (want[1] == span_ref.NO_POS).any())
        same(pd.accept_pos(BASE, OFF, sel, trim_byte=NL, backward=back), want, ("spans", "host", back))
        for limit in (NBYTES, 0):
            first, last = torch.zeros(len(idx), dtype=torch.int64, device="cuda"), torch.zeros(len(idx), dtype=torch.int64, device="cuda")
            pd.accept_pos_device(made["d_base"].data_ptr(), made["d_off"].data_ptr(), N, first.data_ptr(), last.data_ptr(), dp, m, trim_byte=NL, backward=back,
                                 limit=limit)
            torch.cuda.synchronize()
            same((first.cpu().numpy().view(np.uint64), last.cpu().numpy().view(np.uint64)), want, ("spans", "device", back, limit))


# ---- what every host form refuses about a batch -----------------------------------------------------------------------------

def _decreasing(at):
    off = OFF.copy()
    off[at] = off[at + 1] + np.uint64(1)
    return off


BAD_PICK = np.array([4, 0, 5, 2], np.uint64)                 # pick[2] == n
BAD = {
    "offsets decrease at the first pair": dict(off=_decreasing(0)),
    "offsets decrease at a middle pair": dict(off=_decreasing(2)),
    "offsets decrease at the last pair": dict(off=_decreasing(4)),
    "pick[j] == n": dict(pick=BAD_PICK, m=4),
    "no text, but bytes": dict(base=None),
    "trim_byte -2": dict(trim_byte=-2),
    "trim_byte 256": dict(trim_byte=256),
    "an unknown flag bit": dict(flags=0x80000000),
    "no offsets, but inputs": dict(off=None),
}


@pytest.mark.parametrize("case", list(BAD), ids=list(BAD))
def test_bad_batches_are_refused_by_every_host_form(hip, made, case):
    """EINVAL from fsm_hip_tokens_run, fsm_hip_matches_run, fsm_hip_matches_replace and fsm_hip_exec_accept_pos, nothing written,
    and a good call straight after answers"""
    lib = hip.load_library()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    change = BAD[case]
    fields = dict(base=BASE, off=OFF, n=N, pick=None, m=0, trim_byte=NL, flags=0)
    fields.update(change)
    picked = fields["pick"] is not None
    args = {k: (ptr(v) if k in ("base", "off", "pick") else v) for k, v in fields.items()}
    pd, td, rp = made["starts_pd"], made["ends_td"], made["repl"]
    mt = hip.HipMatches.run(pd, td, BASE, OFF, PICK if picked else None, trim_byte=NL)     # the matches of as many inputs
    first, last = np.full(5, 77, np.uint64), np.full(5, 77, np.uint64)
    H = lambda o: C.c_void_p(o.handle)   # noqa: E731
    tb, mb, pb = hip.TokBatch(**args), hip.MatchBatch(**args), hip.PosBatch(first_out=ptr(first), last_out=ptr(last), **args)
    calls = {"tokens": lambda: lib.fsm_hip_tokens_run(H(made["td"]), C.byref(tb)), "matches": lambda: lib.fsm_hip_matches_run(H(pd), H(td), C.byref(mb)),
             "replace": lambda: lib.fsm_hip_matches_replace(H(mt), C.byref(mb), H(rp)),
             "spans": lambda: None if lib.fsm_hip_exec_accept_pos(H(made["ends_pd"]), C.byref(pb)) == -1 else 0}
    for what, call in calls.items():
        C.set_errno(0)
        assert call() is None and C.get_errno() == errno.EINVAL, (case, what, C.get_errno())
    assert (first == 77).all() and (last == 77).all()
    # ... and the next call answers, in every front
    r, res = made["tokens"], made["matches"]
    tk = made["td"].tokens(BASE, OFF, trim_byte=NL)
    same(tk.copy(), (r["off"], r["end"], r["id"], r["err"]), (case, "tokens after"))
    tk.close()
    sel = PICK if picked else np.arange(N)
    mw = matches_ref.select(res, sel)
    same(mt.copy(), mw, (case, "matches"))
    idx = np.asarray(sel, np.int64)
    rd = mt.replace(rp, BASE, OFF, PICK if picked else None, trim_byte=NL)
    same(rd.copy(), replace_ref.replace(RAW_ROWS[idx], LENS[idx], RAWS[idx], mw, TABLE), (case, "replace after"))
    rd.free()
    mt.free()
    mt = hip.HipMatches.run(pd, td, BASE, OFF, trim_byte=NL)
    same(mt.copy(), matches_ref.select(res, np.arange(N)), (case, "matches after"))
    mt.free()
    same(made["ends_pd"].accept_pos(BASE, OFF, trim_byte=NL), span_ref.accept_pos(made["ends"], ROWS, LENS), (case, "spans after"))


def test_device_forms_refuse_bytes_of_no_text(hip, made):
    """base == NULL with limit != 0: EINVAL from all four device forms, nothing launched"""
    lib = hip.load_library()
    H = lambda o: C.c_void_p(o.handle)   # noqa: E731
    args = dict(base=None, off=made["d_off"].data_ptr(), n=N, trim_byte=NL, limit=NBYTES)
    pd, td = made["starts_pd"], made["ends_td"]
    mt = hip.HipMatches.run(pd, td, BASE, OFF, trim_byte=NL)
    tb, mb, pb = hip.TokBatch(**args), hip.MatchBatch(**args), hip.PosBatch(**args)
    for what, call in (("tokens", lambda: lib.fsm_hip_tokens_run_device(H(made["td"]), C.byref(tb), None)),
                       ("matches", lambda: lib.fsm_hip_matches_run_device(H(pd), H(td), C.byref(mb), None)),
                       ("replace", lambda: lib.fsm_hip_matches_replace_device(H(mt), C.byref(mb), H(made["repl"]), None)),
                       ("spans", lambda: None if lib.fsm_hip_exec_accept_pos_device(H(made["ends_pd"]), C.byref(pb), None) == -1 else 0)):
        C.set_errno(0)
        assert call() is None and C.get_errno() == errno.EINVAL, (what, C.get_errno())
    mt.free()
