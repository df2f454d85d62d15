"""GPU: accept positions (libfsm_amd/csrc/span.hip: walk_pos<false>, walk_pos<true>) and the spans of a text's hits (text.hip:
spans_close, spans_advance).

Every answer is compared with tests/span_ref.py -- the definitions of include/fsm_hip.h ("match positions") stated in numpy over
global_ref.trace() and the description's own is_end -- never with anything derived from the code under test.  The automata are
global_ref.affine's (their transition function is a closed formula) and, for the spans, span_ref's Python Aho-Corasick."""
import errno
import os
import subprocess

import numpy as np
import pytest

import span_ref
from global_ref import affine
from line_inputs import FILL, LEAD, SIZES, device_u64, device_u8, lead_packed, make_inputs
from span_ref import NO_POS

pytestmark = pytest.mark.gpu

# name -> (S, K, keyword arguments, the start state is an end state too, walked from LDS)
AUTOMATA = {
    "s15": (15, 4, {}, False, True),
    "s15_start": (15, 4, {}, True, True),                           # pins k = 0
    "s200_dying": (200, 4, dict(holes=16, sinks=3), False, True),
    "lds_full": (1023, 16, {}, False, True),                        # 1024 * 16 = 16 384 entries: the largest LDS image
    "glob_first": (1024, 16, {}, False, False),                     # 1025 * 16 = 16 400 entries: the first global image
    "dying1023": (1023, 16, dict(holes=8, sinks=4), False, True),
}


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()   # raises if the HIP extension is missing: no silent fallback
    return libfsm_amd


def host_u64(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def inputs():
    """the 1 500 rows of tests/line_inputs.py: 300 random bytes; lengths 0, 1, 15, 16, 17, 31, 32, 33, then odd rows 0-12 and even rows 0-300"""
    return make_inputs()


_made = {}


def automaton(name):
    """(auto, PosDfa) of AUTOMATA[name]; the image's form is asserted from the Plan before anything is launched"""
    if name not in _made:
        from libfsm_amd import Plan, PosDfa
        S, K, kw, start_ends, in_lds = AUTOMATA[name]
        auto = affine(S, K, **kw)
        if start_ends:
            auto = span_ref.start_accepting_of(auto)
        assert auto[0].start == 0
        plan = Plan(auto[0])
        assert (plan.S1, plan.C) == (S + 1, K) and (plan.S1 * plan.C <= 16384) == in_lds
        pd = PosDfa.from_flat(auto[0])
        assert pd.in_lds == in_lds
        _made[name] = (auto, pd)
    return _made[name]


_refs = {}


def reference(name, inputs, back):
    """(first, last, the state every input stopped in) of all 1 500 inputs, computed once and left unchanged"""
    if (name, back) not in _refs:
        rows, lens = inputs
        first, last, stop = span_ref.accept_pos(automaton(name)[0], rows, lens, back=back, detail=True)
        for a in (first, last, stop):
            a.setflags(write=False)
        _refs[name, back] = (first, last, stop)
    return _refs[name, back]


def run_device(pd, data, off, m, back=False, want=(True, True), **kw):
    """accept_pos_device over a text of exactly len(data) bytes, the outputs pre-filled and two entries longer than needed:
    (first, last) of m entries each (None for the one left out); nothing behind them was written"""
    import torch
    d_data = device_u8(data) if len(data) else None
    d_off = device_u64(off)
    outs = [device_u64(np.full(m + 2, FILL, np.uint64)) if w else None for w in want]
    tens = {k: device_u64(v) for k, v in kw.items() if k in ("pick", "frm", "to") and v is not None}
    pd.accept_pos_device(d_data.data_ptr() if d_data is not None else 0, d_off.data_ptr(), len(off) - 1,
                         outs[0].data_ptr() if outs[0] is not None else 0, outs[1].data_ptr() if outs[1] is not None else 0,
                         d_pick=tens["pick"].data_ptr() if "pick" in tens else 0, m=m if "pick" in tens else 0,
                         d_from=tens["frm"].data_ptr() if "frm" in tens else 0, d_to=tens["to"].data_ptr() if "to" in tens else 0,
                         trim_byte=kw.get("trim_byte", -1), backward=back, limit=kw.get("limit", 0))
    torch.cuda.synchronize()
    res = []
    for o in outs:
        if o is None:
            res.append(None)
            continue
        h = host_u64(o)
        assert (h[m:] == FILL).all(), "a store behind the outputs"
        res.append(h[:m])
    return res


def run_host(pd, data, off, m, back=False, want=(True, True), **kw):
    outs = tuple(np.full(m + 2, FILL, np.uint64) if w else None for w in want)
    pd.accept_pos(data, off, pick=kw.get("pick"), frm=kw.get("frm"), to=kw.get("to"), trim_byte=kw.get("trim_byte", -1), backward=back, out=outs)
    for o in outs:
        assert o is None or (o[m:] == FILL).all(), "a store behind the outputs"
    return [None if o is None else o[:m] for o in outs]


def check(got, want_first, want_last, what):
    first, last = got
    if first is not None:
        bad = np.flatnonzero(first != want_first)
        assert len(bad) == 0, (what, "first", bad[:5], first[bad[:5]], want_first[bad[:5]])
    if last is not None:
        bad = np.flatnonzero(last != want_last)
        assert len(bad) == 0, (what, "last", bad[:5], last[bad[:5]], want_last[bad[:5]])


# ---- group 1: all inputs ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(AUTOMATA))
def test_every_input_both_directions_both_forms(hip, inputs, name):
    rows, lens = inputs
    auto, pd = automaton(name)
    S, sinks = AUTOMATA[name][0], AUTOMATA[name][2].get("sinks", 0)
    for back in (False, True):
        first, last, stop = reference(name, inputs, back)
        some = first != NO_POS
        want_len = np.where(back, 0, lens).astype(np.uint64)
        # the inputs exercise what they are meant to, by the reference alone: every share at least 0.1, to two decimals (the
        # smallest: dying1023 backward stops in an accepting sink on 149 of the 1 500 inputs)
        share = lambda mask: round(float(mask.mean()), 2)      # noqa: E731
        assert share(some) >= 0.1 and (name == "s15_start" or share(~some) >= 0.1)
        assert share(some & (first != last)) >= 0.1 and share(some & (last == want_len)) >= 0.1
        if sinks:
            assert share(stop == -1) >= 0.1 and share(stop >= S - sinks) >= 0.1
    assert reference("s15_start", inputs, False)[0].max() == 0          # k = 0 accepts everywhere there
    for n in SIZES:
        data, off = lead_packed(rows[:n], lens[:n])
        assert len(data) == int(off[n]) and int(off[0]) == LEAD
        for back in (False, True):
            first, last, _ = reference(name, inputs, back)
            for want in ((True, True), (True, False), (False, True)):
                check(run_device(pd, data, off, n, back, want), first[:n], last[:n], (name, n, back, want, "device"))
                check(run_host(pd, data, off, n, back, want), first[:n], last[:n], (name, n, back, want, "host"))


def test_limit_given_or_read_on_the_device(hip, inputs):
    """limit = off[n] given is limit = 0; a limit inside the text clips the lines that cross it"""
    rows, lens = inputs
    auto, pd = automaton("s200_dying")
    n = 257
    data, off = lead_packed(rows[:n], lens[:n])
    for back in (False, True):
        first, last, _ = reference("s200_dying", inputs, back)
        check(run_device(pd, data, off, n, back, limit=int(off[n])), first[:n], last[:n], ("limit = off[n]", back))
        cut = int(off[200]) + 7
        clipped = np.clip(cut - off[:n].astype(np.int64), 0, lens[:n])
        f2, l2 = span_ref.accept_pos(auto, rows[:n], clipped, back=back)
        assert (clipped != lens[:n]).sum() > 10
        check(run_device(pd, data, off, n, back, limit=cut), f2, l2, ("limit inside", back))


@pytest.mark.parametrize("name", ["s15_start", "lds_full", "glob_first"])
def test_edge_chunks_at_the_head_and_the_tail_of_the_text(hip, inputs, name):
    """lines inside the first and the last 16 bytes of the text: a backward walk assembles the chunk that would begin before base
    from byte loads, a forward walk the one that would end behind the limit (1 to 15 bytes of it, at every lead 0 .. 3)"""
    rows, _ = inputs
    auto, pd = automaton(name)
    for lead in (0, 1, 2, 3):
        for L in (1, 2, 7, 11, 15 - lead):
            lens = np.array([L, 20, 33, 16 - L, L], np.int64)      # line 1 begins inside the head and ends outside it
            sub = rows[100:105]
            data, off = lead_packed(sub, lens, lead)
            for back in (False, True):
                f, l = span_ref.accept_pos(auto, sub, lens, back=back)
                check(run_device(pd, data, off, 5, back), f, l, (name, lead, L, back, "device"))
                check(run_host(pd, data, off, 5, back), f, l, (name, lead, L, back, "host"))


# ---- group 2: pick ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["s200_dying", "glob_first"])
def test_pick(hip, inputs, name):
    rows, lens = inputs
    auto, pd = automaton(name)
    n = 700
    data, off = lead_packed(rows[:n], lens[:n])
    rng = np.random.RandomState(12)
    pick = np.concatenate([rng.permutation(n)[:300], [7, 7, 7, 0, n - 1, n - 1], rng.randint(0, n, 100)]).astype(np.uint64)
    for back in (False, True):
        first, last, _ = reference(name, inputs, back)
        p = pick.astype(np.int64)
        check(run_device(pd, data, off, len(pick), back, pick=pick), first[p], last[p], (name, back, "device"))
        check(run_host(pd, data, off, len(pick), back, pick=pick), first[p], last[p], (name, back, "host"))
        # m = 0: nothing launched, nothing written
        got = run_device(pd, data, off, 0, back, pick=np.zeros(1, np.uint64))
        assert len(got[0]) == 0 and len(got[1]) == 0
        assert all(len(o) == 0 for o in run_host(pd, data, off, 0, back, pick=np.zeros(0, np.uint64)))
        # an index at or beyond n: NO_POS on the device form, its neighbours right; EINVAL on the host form, before any launch
        wild = pick.copy()
        at = [0, 5, 255, 256, len(wild) - 1]
        wild[at] = [n, n + 1, 2 ** 40, NO_POS, n]
        wf, wl = first[p].copy(), last[p].copy()
        wf[at] = NO_POS
        wl[at] = NO_POS
        check(run_device(pd, data, off, len(wild), back, pick=wild), wf, wl, (name, back, "wild"))
        with pytest.raises(OSError) as ei:
            run_host(pd, data, off, len(wild), back, pick=wild)
        assert ei.value.errno == errno.EINVAL
        check(run_host(pd, data, off, len(pick), back, pick=pick), first[p], last[p], (name, back, "the next call answers"))


# ---- group 3: from / to -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["s15", "dying1023", "glob_first"])
def test_from_to(hip, inputs, name):
    rows, lens = inputs
    auto, pd = automaton(name)
    n = 1500
    data, off = lead_packed(rows, lens)
    rng = np.random.RandomState(13)
    inside = np.array([1, 15, 16, 17], np.int64)
    frm = np.zeros(n, np.uint64)
    to = lens.astype(np.uint64).copy()
    kind = np.arange(n) % 8
    k_in = inside[rng.randint(0, 4, n)]
    mid = (rng.rand(n) * (lens + 1)).astype(np.int64)
    frm[kind == 0] = mid[kind == 0]                                        # from == to
    to[kind == 0] = mid[kind == 0]
    to[kind == 1] = (lens + 1 + rng.randint(0, 5, n))[kind == 1]           # to > len: clipped
    to[(kind == 1) & (np.arange(n) % 16 == 1)] = NO_POS
    frm[kind == 2] = (np.minimum(to.astype(np.int64), lens) + 1)[kind == 2]   # from > to': not walked
    frm[kind == 3] = NO_POS                                                # not walked
    frm[kind == 4] = np.minimum(k_in, lens)[kind == 4]                     # starts 1, 15, 16, 17 bytes inside the line
    to[kind == 5] = np.maximum(lens - k_in, 0)[kind == 5]                  # ends 1, 15, 16, 17 bytes inside
    sel = kind >= 6                                                        # both, wherever they fit
    frm[sel] = np.minimum(k_in, lens)[sel]
    to[sel] = np.maximum(lens - inside[rng.randint(0, 4, n)], 0)[sel]      # (from > to' happens here too: not walked)
    for back in (False, True):
        f, l = span_ref.accept_pos(auto, rows, lens, frm=frm, to=to, back=back)
        assert (f[kind == 2] == NO_POS).all() and (f[kind == 3] == NO_POS).all() and (f != NO_POS).sum() > 300
        check(run_device(pd, data, off, n, back, frm=frm, to=to), f, l, (name, back, "device"))
        check(run_host(pd, data, off, n, back, frm=frm, to=to), f, l, (name, back, "host"))
        f, l = span_ref.accept_pos(auto, rows, lens, frm=frm, back=back)
        check(run_device(pd, data, off, n, back, frm=frm), f, l, (name, back, "from alone"))
        f, l = span_ref.accept_pos(auto, rows, lens, to=to, back=back)
        check(run_device(pd, data, off, n, back, to=to), f, l, (name, back, "to alone"))


# ---- group 4: trim ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["s200_dying", "glob_first"])
def test_trim(hip, inputs, name):
    rows, lens = inputs
    auto, pd = automaton(name)
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
    rng = np.random.RandomState(14)
    to = (rng.rand(n) * (lens + 2)).astype(np.uint64)                  # to is clipped to the SHORTENED length
    for back in (False, True):
        f, l = span_ref.accept_pos(auto, rows, shorter, back=back)
        check(run_device(pd, data, off, n, back, trim_byte=trim), f, l, (name, back, "device"))
        check(run_host(pd, data, off, n, back, trim_byte=trim), f, l, (name, back, "host"))
        f, l = span_ref.accept_pos(auto, rows, shorter, to=to, back=back)
        check(run_device(pd, data, off, n, back, trim_byte=trim, to=to), f, l, (name, back, "with to"))
        f, l = span_ref.accept_pos(auto, rows, lens, back=back)        # no trim: the byte is walked like any other
        check(run_device(pd, data, off, n, back), f, l, (name, back, "untrimmed"))


def test_refusals_with_a_device(hip, inputs):
    """EINVAL with the buffers untouched, and the next call answers"""
    import ctypes as C
    from libfsm_amd import PosBatch
    rows, lens = inputs
    auto, pd = automaton("s15")
    lib = hip.load_library()
    n = 64
    data, off = lead_packed(rows[:n], lens[:n])
    first, last, _ = reference("s15", inputs, False)
    out = np.full(n, FILL, np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    good = dict(base=ptr(data), off=ptr(off), n=n, trim_byte=-1, first_out=ptr(out))
    bad_off = off.copy()
    bad_off[10] = bad_off[11] + np.uint64(1)
    for change in (dict(off=None), dict(base=None), dict(flags=2), dict(trim_byte=256), dict(off=ptr(bad_off))):
        b = PosBatch(**dict(good, **change))
        C.set_errno(0)
        assert lib.fsm_hip_exec_accept_pos(C.c_void_p(pd.handle), C.byref(b)) == -1 and C.get_errno() == errno.EINVAL, change
        assert (out == FILL).all()
    b = PosBatch(**good)
    C.set_errno(0)
    assert lib.fsm_hip_exec_accept_pos(None, C.byref(b)) == -1 and C.get_errno() == errno.EINVAL
    assert lib.fsm_hip_exec_accept_pos(C.c_void_p(pd.handle), None) == -1
    d_off = device_u64(off)
    b = PosBatch(base=None, off=d_off.data_ptr(), n=n, trim_byte=-1, limit=int(off[n]), first_out=ptr(out))    # nothing is launched
    C.set_errno(0)
    assert lib.fsm_hip_exec_accept_pos_device(C.c_void_p(pd.handle), C.byref(b), None) == -1 and C.get_errno() == errno.EINVAL
    b = PosBatch(**dict(good, n=0))                   # no lines: nothing launched, 0
    assert lib.fsm_hip_exec_accept_pos(C.c_void_p(pd.handle), C.byref(b)) == 0 and (out == FILL).all()
    b = PosBatch(**good)
    assert lib.fsm_hip_exec_accept_pos(C.c_void_p(pd.handle), C.byref(b)) == 0
    assert np.array_equal(out, first[:n])


# ---- group 5: spans -----------------------------------------------------------------------------------------------------

WORDS = [b"ab", b"abc", b"ca", b"d", b"bdb"]


def span_files(rng):
    """3 files of lines of 0-24 bytes over abcdxyzw, about half of them without any word; the last line has no delimiter"""
    files = []
    for k in (60, 1, 90):
        ls = []
        for i in range(k):
            alpha = b"abcdxyzw" if i % 2 == 0 else b"xyzwba"
            ls.append(bytes(rng.choice(list(alpha), rng.randint(0, 25)).astype(np.uint8)))
        files.append(ls)
    files[2][-1] = b"xxabcabd"
    return files


@pytest.fixture(scope="module")
def span_text(hip):
    """(HipText of the 3 files, the lines without their delimiters, HipHits with one line of context on both sides)"""
    files = span_files(np.random.RandomState(15))
    datas = [b"".join(x + b"\n" for x in ls) for ls in files]
    datas[2] = datas[2][:-1]
    fo = np.cumsum([0] + [len(d) for d in datas]).astype(np.uint64)
    lines = [x for ls in files for x in ls]
    text = hip.HipText(b"".join(datas), 0x0A, file_off=fo)
    assert text.lines == len(lines) and text.files == 3
    ld = hip.LinesDfa(span_ref.line_matcher_of(WORDS)[0], 0x0A)
    hits = text.hits_context(ld, 1, 1)
    core = hits.core()
    assert 20 <= core.sum() and 20 <= (~core).sum()         # hits that are context: they have no span
    return text, lines, hits


def rounds_of(hip, hits, starts_pd, ends_pd, most=200):
    """every round until count() == 0: [(start, end, count)], the last round (count 0) included"""
    sp = hip.HipSpans(hits, starts_pd, ends_pd)
    out = []
    for _ in range(most):
        st, en = sp.copy()
        out.append((st, en, sp.count))
        assert sp.ms() >= 0.0
        if out[-1][2] == 0:
            sp.close()
            return out
        sp.next()
    raise AssertionError("the rounds do not end")


def test_spans_are_leftmost_longest(hip, span_text):
    text, lines, hits = span_text
    picked = [lines[int(i)] for i in hits.lines()]
    want = [span_ref.leftmost_longest(WORDS, x) for x in picked]
    core = hits.core()
    assert all((len(w) > 0) == bool(c) for w, c in zip(want, core))
    assert want[-1] == [(2, 5), (5, 7), (7, 8)]                   # the last line, without a delimiter: "xxabcabd"
    starts_pd, ends_pd = hip.PosDfa.from_flat(span_ref.starts_of(WORDS)[0]), hip.PosDfa.from_flat(span_ref.ends_of(WORDS)[0])
    rounds = rounds_of(hip, hits, starts_pd, ends_pd)
    got = [[] for _ in picked]
    for st, en, count in rounds:
        assert ((st == NO_POS) == (en == NO_POS)).all() and count == int((st != NO_POS).sum())
        for i in np.flatnonzero(st != NO_POS):
            got[i].append((int(st[i]), int(en[i])))
    assert got == want
    assert len(rounds) == max(len(w) for w in want) + 1 and len(rounds) >= 5
    # hits without bytes and inverted hits: the text is read, and lines without a match have no span
    ld = hip.LinesDfa(span_ref.line_matcher_of(WORDS)[0], 0x0A)
    plain = text.hits(ld, want_bytes=False)
    r2 = rounds_of(hip, plain, starts_pd, ends_pd)
    assert [c for _, _, c in r2] == [sum(len(w) > k for w in want) for k in range(len(rounds))]
    inv = text.hits(ld, invert=True)
    r3 = rounds_of(hip, inv, starts_pd, ends_pd)
    assert inv.count > 20 and len(r3) == 1 and r3[0][2] == 0 and (r3[0][0] == NO_POS).all() and (r3[0][1] == NO_POS).all()


def test_spans_of_no_hits(hip, span_text):
    """m == 0: a valid object, count 0, nothing launched"""
    text, lines, _ = span_text
    ld = hip.LinesDfa(span_ref.line_matcher_of([b"qqqq"])[0], 0x0A)
    hits = text.hits(ld)
    assert hits.count == 0
    pd = hip.PosDfa.from_flat(span_ref.ends_of(WORDS)[0])
    sp = hip.HipSpans(hits, pd, pd)
    assert sp.count == 0 and sp.start_ptr == 0 and sp.end_ptr == 0
    st, en = sp.copy()
    assert len(st) == 0 and len(en) == 0
    sp.next()
    assert sp.count == 0


def test_spans_of_any_pair_follow_the_composed_definition(hip, span_text):
    """the two automata need not belong together (s15 as starts, s200_dying as ends), and one that matches the empty string
    advances by one: the rounds are those of span_ref.spans_rounds"""
    text, lines, hits = span_text
    picked = [lines[int(i)] for i in hits.lines()]
    rows, lens = span_ref.rows_of(picked)
    s15, s200 = automaton("s15"), automaton("s200_dying")
    empty = (span_ref.everywhere_of(span_ref.starts_of(WORDS)), span_ref.ends_of(WORDS, empty=True))
    pairs = {"unrelated": (s15[0], s200[0], s15[1], s200[1]),
             "empty": (empty[0], empty[1], hip.PosDfa.from_flat(empty[0][0]), hip.PosDfa.from_flat(empty[1][0]))}
    for what, (starts, ends, starts_pd, ends_pd) in pairs.items():
        want = span_ref.spans_rounds(starts, ends, rows, lens)
        got = rounds_of(hip, hits, starts_pd, ends_pd)
        assert len(got) == len(want), what
        for k, ((st, en, count), (wst, wen)) in enumerate(zip(got, want)):
            assert np.array_equal(st, wst) and np.array_equal(en, wen) and count == int((wst != NO_POS).sum()), (what, k)
        if what == "empty":                      # every hit: a span at every p up to len, so len + 1 rounds at the least
            assert len(want) >= int(lens.max()) // 3 + 2 and any((st == en)[st != NO_POS].any() for st, en in want)
            assert want[0][0].tolist() == [0] * len(picked)


# ---- group 6: the example -----------------------------------------------------------------------------------------------

def test_example_prints_what_grep_o_prints(hip, tmp_path):
    """examples/hipgrep_only.c over three files (the last line without a newline) against the brute force's -o, -b -o, -n -o"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = span_files(np.random.RandomState(16))
    tables = []
    for nm, auto in (("lines", span_ref.line_matcher_of(WORDS)), ("starts", span_ref.starts_of(WORDS)), ("ends", span_ref.ends_of(WORDS))):
        tables.append(str(tmp_path / (nm + ".fsmhip")))
        auto[0].write_c(tables[-1])
    names = []
    for j, ls in enumerate(files):
        data = b"".join(x + b"\n" for x in ls)
        p = tmp_path / ("f%d.txt" % j)
        p.write_bytes(data[:-1] if j == 2 else data)
        names.append(str(p))
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    exe = str(tmp_path / "hipgrep_only")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "hipgrep_only.c"), "-o", exe,
                           "-L" + os.path.join(root, "libfsm_amd"), "-lfsm_hip", "-Wl,-rpath," + os.path.join(root, "libfsm_amd")])

    def run(*opts, fs=names):
        r = subprocess.run([exe, *opts, *tables, *fs], capture_output=True, env=env, timeout=120)
        return r.returncode, r.stdout

    def compose(byte=False, number=False, name=False):
        out = b""
        for nm, ls in zip(names, files):
            at = 0
            for i, x in enumerate(ls):
                for s, e in span_ref.leftmost_longest(WORDS, x):
                    out += (nm.encode() + b":" if name else b"") + (b"%d:" % (i + 1) if number else b"") + (b"%d:" % (at + s) if byte else b"")
                    out += x[s:e] + b"\n"
                at += len(x) + 1
        return out

    assert compose().count(b"\n") >= 100
    assert run() == (0, compose())
    assert run("-b") == (0, compose(byte=True))
    assert run("-n") == (0, compose(number=True))
    assert run("-H", "-n", "-b") == (0, compose(True, True, True))
    quiet = tmp_path / "none.txt"
    quiet.write_bytes(b"xyz\nwwww\n\n")
    assert run(fs=[str(quiet)]) == (1, b"")                    # nothing matched: grep's 1
