"""GPU: tokens (libfsm_amd/csrc/tok.hip: walk_tok<false>, walk_tok<true> and the fronts).

Every answer -- count, tok_off, end, id, err, total -- is compared with tests/tokens_ref.py, the definition of include/fsm_hip.h
("tokens") restated in plain Python over the automaton's own formula, never with anything derived from the code under test.  The
automata are global_ref.affine's, span_ref's variants of them and a word lexer (a trie); the inputs are the 1 500 rows of
tests/line_inputs.py."""
import ctypes as C
import errno
import os
import subprocess
import sys

import numpy as np
import pytest

import span_ref
import tokens_ref
from global_ref import affine
from line_inputs import FILL, LEAD, SIZES, device_u64, device_u8, lead_packed, make_inputs
from tokens_ref import EARLIEST, ERROR, NO_BACKTRACK, NO_MATCH, NO_POS, RET, SKIP_BAD

pytestmark = pytest.mark.gpu

# name -> (S, K, keyword arguments, walked from LDS)
AFFINE = {
    "s15": (15, 4, {}, True),
    "s200_dying": (200, 4, dict(holes=16, sinks=3), True),
    "dying1023": (1023, 16, dict(holes=8, sinks=4), True),          # 1024 * 16 = 16 384 entries: the largest LDS image
    "glob_dying": (1024, 16, dict(holes=4), False),                 # 1025 * 16 = 16 400 entries: the first global image
}
FURTHER = ("s15_start", "s200_everywhere", "words")
WORDS = [w.encode() for w in "a ab abcda b bc bcdab c ca cab d dd ddabc".split()]
COMBOS = (0, NO_BACKTRACK, SKIP_BAD, NO_BACKTRACK | SKIP_BAD)


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()   # raises if the HIP extension is missing: no silent fallback
    return libfsm_amd


def word_inputs():
    """the same 1 500 lengths over abcdx, x rare: lines a word lexer cuts into many tokens"""
    rng = np.random.RandomState(17)
    _, lens = make_inputs()
    rows = np.frombuffer(b"abcdx", np.uint8)[rng.choice(5, (1500, 300), p=[.24, .24, .24, .24, .04])]
    return np.ascontiguousarray(rows), lens


_made = {}


def automaton(name, mode=EARLIEST):
    """(auto, TokDfa, ids by state, rows, lens) of a named automaton; the image's form is asserted from the Plan before anything
    is launched"""
    if (name, mode) not in _made:
        from libfsm_amd import Plan, TokDfa
        sets = None
        if name in AFFINE:
            S, K, kw, in_lds = AFFINE[name]
            auto = affine(S, K, endids=True, **kw)
            shape = (S + 1, K)
        elif name == "s15_start":
            auto, in_lds, shape = span_ref.start_accepting_of(affine(15, 4)), True, (16, 4)
        elif name == "s200_everywhere":
            auto, in_lds, shape = span_ref.everywhere_of(affine(200, 4, holes=16, sinks=3)), True, (201, 4)
        else:
            auto, sets = tokens_ref.trie_lexer(WORDS)
            in_lds, shape = True, (auto[0].nstates + 1, None)
        assert auto[0].start == 0
        plan = Plan(auto[0])
        if name != "words":
            assert (plan.S1, plan.C) == shape
        assert plan.S1 == shape[0] and (plan.S1 * plan.C <= 16384) == in_lds
        td = TokDfa.from_flat(auto[0], mode)
        assert td.in_lds == in_lds
        rows, lens = word_inputs() if name == "words" else make_inputs()
        _made[name, mode] = (auto, td, tokens_ref.state_ids(auto, mode, sets), rows, lens)
    return _made[name, mode]


_judges, _refs = {}, {}


def reference(name, flags, mode=EARLIEST):
    """the judge's answer for all 1 500 inputs, computed once and left unchanged"""
    if (name, flags, mode) not in _refs:
        auto, _, ids, rows, lens = automaton(name, mode)
        if name not in _judges:
            _judges[name] = tokens_ref.Judge(auto, rows, lens)
        res = _judges[name].run(flags, ids)
        for v in res.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _refs[name, flags, mode] = res
    return _refs[name, flags, mode]


def head(res, n):
    """the answer for the first n inputs: (off, end, id, err)"""
    total = int(res["off"][n])
    return res["off"][:n + 1], res["end"][:total], res["id"][:total], res["err"][:n]


def check(tk, want, what, m=None):
    """a tokens object against (off, end, id, err); the copies are pre-filled and two entries too long: nothing behind total or
    behind m was written"""
    w_off, w_end, w_id, w_err = want
    m = len(w_err) if m is None else m
    total = int(w_off[-1])
    assert tk.count == m, (what, "m")
    assert tk.total == total, (what, "total", tk.total, total)
    off, end, ids, err = tk.copy(extra=2, fill=FILL)
    assert (off[m + 1:] == FILL).all() and (end[total:] == FILL).all() and (ids[total:] == FILL & 0xFFFFFFFF).all() and (err[m:] == FILL).all(), what
    assert int(off[m]) == total, (what, "tok_off[m] == total")
    for nm, got, exp in (("tok_off", off[:m + 1], w_off), ("err", err[:m], w_err), ("end", end[:total], w_end), ("id", ids[:total], w_id)):
        bad = np.flatnonzero(got != exp)
        assert len(bad) == 0, (what, nm, bad[:5], got[bad[:5]], exp[bad[:5]])
    assert tk.ms() >= 0.0
    tk.close()


def run_device(td, data, off, flags, pick=None, trim_byte=-1, limit=0):
    """tokens_run_device over a text of exactly len(data) bytes"""
    import torch
    d_data = device_u8(data) if len(data) else None
    d_off = device_u64(off)
    d_pick = device_u64(pick if len(pick) else np.zeros(1, np.uint64)) if pick is not None else None
    tk = td.tokens_device(d_data.data_ptr() if d_data is not None else 0, d_off.data_ptr(), len(off) - 1,
                          d_pick=d_pick.data_ptr() if d_pick is not None else 0, m=len(pick) if pick is not None else 0,
                          trim_byte=trim_byte, flags=flags, limit=limit)
    torch.cuda.synchronize()
    tk._keep = (tk._keep, d_data, d_off, d_pick)
    return tk


# ---- group 1: the judge's own output is not trivial ------------------------------------------------------------------------

def test_conditions_on_the_judges_output(hip):
    """at n = 1 500: shares of the judge's answer alone, so that no test below can pass on trivial lines"""
    n = 1500
    for name in AFFINE:
        S, sinks = AFFINE[name][0], AFFINE[name][2].get("sinks", 0)
        r = reference(name, 0)
        cnt = np.diff(r["off"].astype(np.int64))
        real = r["state"] >= 0
        assert real.all()
        print(name, "default:", (cnt >= 2).mean(), (r["err"] != NO_POS).mean(), (r["length"] > 16).mean(), (r["overrun"] >= 2).mean(),
              (r["overrun"] >= 16).mean())
        assert (cnt >= 2).mean() >= 0.15
        assert (r["err"] != NO_POS).mean() >= 0.55
        assert (r["length"] > 16).mean() >= 0.4
        assert (r["overrun"] >= 2).mean() >= 0.4
        assert (r["overrun"] >= 16).mean() >= 0.015
        if sinks:
            line_of = np.repeat(np.arange(n), cnt)
            in_sink = np.zeros(n, bool)
            in_sink[line_of[r["state"] >= S - sinks]] = True
            print(name, "sink lines:", in_sink.mean())
            assert in_sink.mean() >= 0.15
        k = reference(name, SKIP_BAD)
        kcnt = np.diff(k["off"].astype(np.int64))
        print(name, "skip_bad:", (k["state"] < 0).mean(), (kcnt >= 2).mean(), kcnt.max())
        assert (k["state"] < 0).mean() >= 0.4
        assert (kcnt >= 2).mean() >= 0.65
        assert kcnt.max() >= 12
        kb = reference(name, SKIP_BAD | NO_BACKTRACK)
        ko, kbo = k["off"].astype(np.int64), kb["off"].astype(np.int64)
        differ = np.array([not np.array_equal(k["end"][ko[i]:ko[i + 1]], kb["end"][kbo[i]:kbo[i + 1]]) or
                           not np.array_equal(k["id"][ko[i]:ko[i + 1]], kb["id"][kbo[i]:kbo[i + 1]]) for i in range(n)])
        print(name, "rules differ under skip_bad:", differ.mean())
        assert differ.mean() >= 0.4
    # the empty match at the start state is ignored: no token is empty, anywhere
    for name in list(AFFINE) + list(FURTHER):
        for flags in COMBOS:
            assert (reference(name, flags)["length"] >= 1).all()
    w = reference("words", 0)
    assert (np.diff(w["off"].astype(np.int64)) >= 4).mean() >= 0.3 and set(w["id"].tolist()) == set(range(12))


# ---- group 2: every automaton x every n, both forms, both rules, both modes -------------------------------------------------

@pytest.mark.parametrize("name", list(AFFINE) + list(FURTHER))
def test_every_input_both_rules_both_modes_both_forms(hip, name):
    auto, td, ids, rows, lens = automaton(name)
    for n in SIZES:
        data, off = lead_packed(rows[:n], lens[:n])
        assert len(data) == int(off[n]) and int(off[0]) == LEAD
        for flags in COMBOS:
            want = head(reference(name, flags), n)
            check(run_device(td, data, off, flags), want, (name, n, flags, "device"))
            check(td.tokens(data, off, flags=flags), want, (name, n, flags, "host"))


def test_earliest_against_ret(hip):
    """the same tokens, the ids of the other mode; ERROR is EARLIEST on a conflict-free automaton and EINVAL on the others"""
    from libfsm_amd import TokDfa
    n = 257
    for name in ("s200_dying", "glob_dying"):
        auto, td_r, ids_r, rows, lens = automaton(name, RET)
        data, off = lead_packed(rows[:n], lens[:n])
        e, r = reference(name, 0, EARLIEST), reference(name, 0, RET)
        assert np.array_equal(e["end"], r["end"]) and (e["id"] != r["id"]).mean() > 0.5
        check(run_device(td_r, data, off, 0), head(r, n), (name, "ret"))
        check(run_device(automaton(name, EARLIEST)[1], data, off, 0), head(e, n), (name, "earliest"))
        assert tokens_ref.conflict(auto)
        with pytest.raises(OSError) as ei:
            TokDfa.from_flat(auto[0], ERROR)
        assert ei.value.errno == errno.EINVAL
    auto, td, ids, rows, lens = automaton("words", ERROR)
    assert not tokens_ref.conflict(auto, tokens_ref.trie_lexer(WORDS)[1])
    data, off = lead_packed(rows[:n], lens[:n])
    check(run_device(td, data, off, 0), head(reference("words", 0), n), ("words", "error mode"))
    for bad_mode in (0, 4, -1):
        with pytest.raises(OSError) as ei:
            TokDfa.from_flat(auto[0], bad_mode)
        assert ei.value.errno == errno.EINVAL


# ---- group 3: pick, trim, limit, edges -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["s200_dying", "glob_dying", "words"])
def test_pick(hip, name):
    auto, td, ids, rows, lens = automaton(name)
    n = 700
    data, off = lead_packed(rows[:n], lens[:n])
    rng = np.random.RandomState(12)
    pick = np.concatenate([rng.permutation(n)[:300], [7, 7, 7, 0, n - 1, n - 1], rng.randint(0, n, 100), np.arange(n)[::-1][:50]]).astype(np.uint64)
    for flags in COMBOS:
        res = reference(name, flags)
        want = tokens_ref.select(res, pick)
        check(run_device(td, data, off, flags, pick=pick), want, (name, flags, "device"))
        check(td.tokens(data, off, pick=pick, flags=flags), want, (name, flags, "host"))
        # an empty pick: a valid object, nothing launched that stores
        none = (np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint64))
        check(run_device(td, data, off, flags, pick=np.zeros(0, np.uint64)), none, (name, flags, "m == 0 device"), m=0)
        check(td.tokens(data, off, pick=np.zeros(0, np.uint64), flags=flags), none, (name, flags, "m == 0 host"), m=0)
        # an index at or beyond n: no token and no err on the device form, its neighbours right; EINVAL on the host form
        wild = pick.copy()
        at = [0, 5, 255, 256, len(wild) - 1]
        wild[at] = [n, n + 1, 2 ** 40, NO_POS, n]
        empty = dict(res)
        empty["off"] = np.concatenate([res["off"], res["off"][-1:]])        # line 1500: one without tokens
        empty["err"] = np.concatenate([res["err"], [np.uint64(NO_POS)]])
        as_empty = wild.copy()
        as_empty[at] = 1500
        check(run_device(td, data, off, flags, pick=wild), tokens_ref.select(empty, as_empty), (name, flags, "wild"))
        with pytest.raises(OSError) as ei:
            td.tokens(data, off, pick=wild, flags=flags)
        assert ei.value.errno == errno.EINVAL
    check(td.tokens(data, off, pick=pick), tokens_ref.select(reference(name, 0), pick), (name, "the next call answers"))


@pytest.mark.parametrize("name", ["s200_dying", "glob_dying"])
def test_trim(hip, name):
    auto, td, ids, rows, lens = automaton(name)
    n, trim = 600, 0x0A
    rows = rows[:n].copy()
    lens = lens[:n].copy()
    idx = np.arange(n)
    ends_in = (idx % 3 == 0) & (lens > 0)
    rows[idx[ends_in], lens[ends_in] - 1] = trim                       # lines ending in the byte
    other = ~ends_in & (lens > 0)
    rows[idx[other], lens[other] - 1] = np.where(rows[idx[other], lens[other] - 1] == trim, 0x41, rows[idx[other], lens[other] - 1])
    lens[10], lens[11] = 1, 0                                          # a line of that byte alone, the empty line
    rows[10, 0] = trim
    ends_in[10], ends_in[11] = True, False
    shorter = lens - ends_in
    assert ends_in.sum() > 100 and (lens == 0).sum() > 5 and (~ends_in & (lens > 0)).sum() > 100
    data, off = lead_packed(rows, lens)
    for flags in COMBOS:
        r = tokens_ref.Judge(auto, rows, shorter).run(flags, ids)
        want = (r["off"], r["end"], r["id"], r["err"])
        check(run_device(td, data, off, flags, trim_byte=trim), want, (name, flags, "device"))
        check(td.tokens(data, off, trim_byte=trim, flags=flags), want, (name, flags, "host"))
    r = tokens_ref.Judge(auto, rows, lens).run(0, ids)             # no trim: the byte is walked like any other
    check(run_device(td, data, off, 0), (r["off"], r["end"], r["id"], r["err"]), (name, "untrimmed"))


def test_limit_given_or_read_on_the_device(hip):
    """limit = off[n] given is limit = 0; a limit inside the text clips the lines that cross it"""
    auto, td, ids, rows, lens = automaton("s200_dying")
    n = 257
    data, off = lead_packed(rows[:n], lens[:n])
    for flags in (0, SKIP_BAD):
        check(run_device(td, data, off, flags, limit=int(off[n])), head(reference("s200_dying", flags), n), ("limit = off[n]", flags))
        cut = int(off[200]) + 7
        clipped = np.clip(cut - off[:n].astype(np.int64), 0, lens[:n])
        assert (clipped != lens[:n]).sum() > 10
        r = tokens_ref.Judge(auto, rows[:n], clipped).run(flags, ids)
        check(run_device(td, data, off, flags, limit=cut), (r["off"], r["end"], r["id"], r["err"]), ("limit inside", flags))


@pytest.mark.parametrize("name", ["s15_start", "dying1023", "glob_dying", "words"])
def test_edge_chunks_at_the_head_and_the_tail_of_the_text(hip, name):
    """lines of 1 to 15 bytes at the head and at the very end of a text with leads 0 .. 3, limit set exactly to the text's
    length: the chunk that would end behind the limit is assembled from byte loads"""
    auto, td, ids, rows, _ = automaton(name)
    for lead in (0, 1, 2, 3):
        for L in (1, 2, 7, 11, 15 - lead, 15):
            lens = np.array([L, 20, 33, 16 - L, L], np.int64)
            sub = rows[100:105]
            data, off = lead_packed(sub, lens, lead)
            j = tokens_ref.Judge(auto, sub, lens)
            for flags in COMBOS:
                r = j.run(flags, ids)
                want = (r["off"], r["end"], r["id"], r["err"])
                check(run_device(td, data, off, flags, limit=len(data)), want, (name, lead, L, flags, "device"))
                check(td.tokens(data, off, flags=flags), want, (name, lead, L, flags, "host"))


# ---- group 4: the text front -----------------------------------------------------------------------------------------------

def text_lines(rng):
    """400 lines of 0-60 bytes over abcdx and, every third, over xyz: about a third without any token; the last without a newline"""
    out = []
    for i in range(400):
        alpha = b"abcdx" if i % 3 else b"xyzw"
        out.append(bytes(rng.choice(list(alpha), rng.randint(0, 61)).astype(np.uint8)))
    out[-1] = b"abcdab"
    return out


def test_text_tokens_over_a_text_and_its_hits(hip):
    auto, td, ids, _, _ = automaton("words")
    lines = text_lines(np.random.RandomState(18))
    blob = b"".join(x + b"\n" for x in lines)[:-1]
    text = hip.HipText(blob, 0x0A)
    assert text.lines == len(lines)
    rows, lens = span_ref.rows_of(lines)
    judge = tokens_ref.Judge(auto, rows, lens)
    off = np.zeros(len(lines) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) + 1 for x in lines])
    off[-1] -= 1
    ld = hip.LinesDfa(span_ref.line_matcher_of([b"ab", b"dd"])[0], 0x0A)
    kinds = {"plain": text.hits(ld), "no bytes": text.hits(ld, want_bytes=False), "inverted": text.hits(ld, invert=True)}
    assert 100 < kinds["plain"].count < 300 and kinds["plain"].count + kinds["inverted"].count == len(lines)
    for flags in COMBOS:
        res = judge.run(flags, ids)
        want = (res["off"], res["end"], res["id"], res["err"])
        check(td.text_tokens(text, flags=flags), want, ("text", flags))
        # ... is the primitive over the text's own offsets with the delimiter trimmed
        check(td.tokens(np.frombuffer(blob, np.uint8), off, trim_byte=0x0A, flags=flags), want, ("primitive", flags))
        for what, hits in kinds.items():
            check(td.text_tokens(text, hits, flags=flags), tokens_ref.select(res, hits.lines()), (what, flags))
    assert (judge.run(0, ids)["err"] != NO_POS).mean() > 0.3


def test_empty_text_no_inputs_and_no_tokens(hip):
    auto, td, ids, rows, lens = automaton("words")
    none = (np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint64))
    for flags in COMBOS:
        text = hip.HipText(b"", 0x0A)
        assert text.lines == 0
        tk = td.text_tokens(text, flags=flags)
        assert tk.end_ptr == 0 and tk.id_ptr == 0 and tk.err_ptr == 0 and tk.off_ptr != 0
        check(tk, none, ("empty text", flags), m=0)
        check(td.tokens(np.zeros(0, np.uint8), np.zeros(1, np.uint64), flags=flags), none, ("n == 0 host", flags), m=0)
        check(run_device(td, np.zeros(0, np.uint8), np.zeros(1, np.uint64), flags), none, ("n == 0 device", flags), m=0)
    # a text whose tokens total 0: lines of bytes no word begins with, and empty lines
    lines = [b"xx", b"", b"xyz", b"", b"x" * 40]
    text = hip.HipText(b"".join(x + b"\n" for x in lines), 0x0A)
    zero = (np.zeros(len(lines) + 1, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32),
            np.array([0, NO_POS, 0, NO_POS, 0], np.uint64))
    for flags in (0, NO_BACKTRACK):
        tk = td.text_tokens(text, flags=flags)
        assert tk.total == 0 and tk.end_ptr == 0 and tk.id_ptr == 0
        check(tk, zero, ("total == 0", flags))
    tk = td.text_tokens(text, flags=SKIP_BAD)           # ... and every byte a bad one
    assert tk.total == 45 and (tk.copy()[2] == NO_MATCH).all()


# ---- group 5: refusals -----------------------------------------------------------------------------------------------------

def test_refusals_with_a_device(hip):
    """EINVAL, and the next call answers"""
    from libfsm_amd import TokBatch
    auto, td, ids, rows, lens = automaton("s15")
    lib = hip.load_library()
    n = 64
    data, off = lead_packed(rows[:n], lens[:n])
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    good = dict(base=ptr(data), off=ptr(off), n=n, trim_byte=-1)
    bad_off = off.copy()
    bad_off[10] = bad_off[11] + np.uint64(1)
    for change in (dict(off=None), dict(base=None), dict(flags=4), dict(flags=0x80000000), dict(trim_byte=256), dict(trim_byte=-2), dict(off=ptr(bad_off))):
        b = TokBatch(**dict(good, **change))
        C.set_errno(0)
        assert lib.fsm_hip_tokens_run(C.c_void_p(td.handle), C.byref(b)) is None and C.get_errno() == errno.EINVAL, change
    b = TokBatch(**good)
    C.set_errno(0)
    assert lib.fsm_hip_tokens_run(None, C.byref(b)) is None and C.get_errno() == errno.EINVAL
    C.set_errno(0)
    assert lib.fsm_hip_tokens_run(C.c_void_p(td.handle), None) is None and C.get_errno() == errno.EINVAL
    d_off = device_u64(off)
    b = TokBatch(base=None, off=d_off.data_ptr(), n=n, trim_byte=-1, limit=int(off[n]))    # nothing is launched
    C.set_errno(0)
    assert lib.fsm_hip_tokens_run_device(C.c_void_p(td.handle), C.byref(b), None) is None and C.get_errno() == errno.EINVAL
    text = hip.HipText(b"ab\ncd\n", 0x0A)
    for args in ((None, text.handle, None, 0, None), (td.handle, None, None, 0, None), (td.handle, text.handle, None, 4, None)):
        C.set_errno(0)
        assert lib.fsm_hip_text_tokens(*args) is None and C.get_errno() == errno.EINVAL, args
    check(td.tokens(data, off), head(reference("s15", 0), n), "the next call answers")


def test_errno_table_from_a_child_process():
    """the errno table in a process of its own, which has used the device for nothing else: every refusal is EINVAL there (ENODEV,
    which is checked first, is what tests/test_tokens_abi.py sees where there is no device), and a run after them answers"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import ctypes as C, errno, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import libfsm_amd
import tokens_ref
lib = libfsm_amd.load_library()
auto, sets = tokens_ref.trie_lexer([b"ab", b"abc", b"c"])
td = libfsm_amd.TokDfa.from_flat(auto[0])
data, off = np.frombuffer(b"abcabx", np.uint8), np.array([0, 5, 6], np.uint64)
ptr = lambda a: a.ctypes.data_as(C.c_void_p)
good = dict(base=ptr(data), off=ptr(off), n=2, trim_byte=-1)
table = [(lib.fsm_hip_tok_dfa_create, (None, 1))]
for change in (dict(off=None), dict(base=None), dict(flags=4), dict(trim_byte=256), dict(trim_byte=-2), dict(off=ptr(off[::-1].copy()))):
    table.append((lib.fsm_hip_tokens_run, (C.c_void_p(td.handle), C.byref(libfsm_amd.TokBatch(**dict(good, **change))))))
table += [(lib.fsm_hip_tokens_run, (None, C.byref(libfsm_amd.TokBatch(**good)))), (lib.fsm_hip_tokens_run, (C.c_void_p(td.handle), None)),
          (lib.fsm_hip_tokens_run_device, (None, None, None)), (lib.fsm_hip_text_tokens, (None, None, None, 0, None)),
          (lib.fsm_hip_text_tokens, (C.c_void_p(td.handle), None, None, 0, None))]
for k, (fn, args) in enumerate(table):
    C.set_errno(0)
    assert fn(*args) is None and C.get_errno() == errno.EINVAL, (k, C.get_errno())
tk = td.tokens(data, off)
o, e, i, r = tk.copy()
assert o.tolist() == [0, 2, 2] and e.tolist() == [3, 5] and i.tolist() == [1, 0] and r.tolist() == [2 ** 64 - 1, 0], (o, e, i, r)
print("child ok")
""" % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.stdout + r.stderr)[-2000:]


# ---- group 6: the example --------------------------------------------------------------------------------------------------

def test_example_prints_the_judges_tokens(hip, tmp_path):
    """examples/hiplex.c over a small text against the judge: line:start-end:id per token, -s for SKIP_BAD"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    auto, td, ids, _, _ = automaton("words")
    lines = text_lines(np.random.RandomState(19))[:120]
    table = str(tmp_path / "words.fsmhip")
    auto[0].write_c(table)
    path = tmp_path / "in.txt"
    path.write_bytes(b"".join(x + b"\n" for x in lines)[:-1])
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    exe = str(tmp_path / "hiplex")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "hiplex.c"),
                           "-o", exe, "-L" + os.path.join(root, "libfsm_amd"), "-lfsm_hip", "-Wl,-rpath," + os.path.join(root, "libfsm_amd")])
    judge = tokens_ref.Judge(auto, *span_ref.rows_of(lines))
    for opts, flags in (((), 0), (("-s",), SKIP_BAD)):
        res = judge.run(flags, ids)
        off = res["off"].astype(np.int64)
        want = b""
        for i in range(len(lines)):
            p = 0
            for k in range(off[i], off[i + 1]):
                idv = int(res["id"][k])
                want += b"%d:%d-%d:%s\n" % (i + 1, p, int(res["end"][k]), b"-" if idv == NO_MATCH else b"%d" % idv)
                p = int(res["end"][k])
        r = subprocess.run([exe, *opts, table, str(path)], capture_output=True, env=env, timeout=120)
        assert want.count(b"\n") >= 100 and (r.returncode, r.stdout) == (0, want), r.stderr[-500:]   # (the spans example asks as many)
