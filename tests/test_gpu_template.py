"""GPU: replacement templates -- the match itself inside its replacement (libfsm_amd/csrc/replace.hip: repl_lengths<true>,
repl_write<LDS / global table, true>; fsm_hip_repl_create_template beside them).

out_off and every output byte are compared with tests/template_ref.py, the definition of include/fsm_hip.h ("replace", the template
table) restated in Python, over the matches of tests/matches_ref.py -- never over matches or offsets that came from the device.  The
inputs are the 1 500 keyword lines of tests/line_inputs.py, as are the automata and the matches' judge: rows of at most 300 bytes with
lengths 0, 1, 15, 16, 17, 31, 32, 33, ..., line 8 = 300 times d, and LEAD = 5 bytes in front of the text that belong to no line."""
import ctypes as C
import errno
import functools
import os
import subprocess

import numpy as np
import pytest

import matches_ref
import replace_ref
import span_ref
import template_ref
from line_inputs import (EMPTY_RULE, FILL, KEYWORDS, SIZES, auto_of, device_u64, device_u8, ends_image, inputs_of, judged, lead_packed, reference,
                         starts_image, state_ids)
from matches_ref import DROP_EMPTY

pytestmark = pytest.mark.gpu

BLOCK = 16384
# one table over the five keyword rules: & alone, <&>, &&, 17 literal bytes + & + 40 literal bytes, a rule without an insert
SEVENTEEN, FORTY = bytes(range(0x30, 0x30 + 17)), bytes(range(0x50, 0x50 + 40))
MIXED = [b"&", b"<&>", b"&&", SEVENTEEN + b"&" + FORTY, b"plain"]
LONG = 40000


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()   # raises if the HIP extension is missing: no silent fallback
    return libfsm_amd


def parsed(seds):
    """sed replacements -> (table, inserts), by the judge's parser"""
    p = [template_ref.parse_sed(x) for x in seds]
    return [x[0] for x in p], [x[1] for x in p]


def check(rd, want, what, m=None):
    """a replaced object against (out_off, bytes); the copies are pre-filled and two entries too long: nothing behind nbytes or
    behind m + 1 was written"""
    w_off, w_data = want
    m = len(w_off) - 1 if m is None else m
    total = int(w_off[-1])
    assert rd.count == m, (what, "m")
    assert rd.nbytes == total, (what, "nbytes", rd.nbytes, total)
    assert rd.off_ptr != 0 and (rd.bytes_ptr != 0) == (total != 0), what
    off, data = rd.copy(extra=2, fill=FILL)
    assert (off[m + 1:] == FILL).all() and (data[total:] == FILL & 0xFF).all(), what
    bad = np.flatnonzero(off[:m + 1] != w_off)
    assert len(bad) == 0, (what, "out_off", bad[:5], off[bad[:5]], w_off[bad[:5]])
    bad = np.flatnonzero(data[:total] != w_data)
    assert len(bad) == 0, (what, "bytes", bad[:8], data[bad[:8]], w_data[bad[:8]], "line", np.searchsorted(w_off, bad[:8], "right") - 1)
    assert rd.ms >= 0.0 and all(rd.pass_ms(k) >= 0.0 for k in range(4))
    rd.free()
    return off[:m + 1], data[:total]


class Batch:
    """a packed text on the device and on the host"""

    def __init__(self, data, off):
        self.data, self.off = data, off
        self.n = len(off) - 1
        self.d_data = device_u8(data) if len(data) else None
        self.d_off = device_u64(off)

    def device_args(self):
        return dict(d_base=self.d_data.data_ptr() if self.d_data is not None else 0, d_off=self.d_off.data_ptr(), n=self.n, limit=len(self.data))


def device_form(hip, pd, td, b, rp, mflags=0):
    """matches_run_device, then matches_replace_device on the same batch"""
    import torch
    mt = hip.HipMatches.run_device(pd, td, flags=mflags, **b.device_args())
    rd = mt.replace_device(rp, **b.device_args())
    torch.cuda.synchronize()
    rd._keep = (rd._keep, b)
    return rd


def host_form(hip, pd, td, b, rp, mflags=0):
    mt = hip.HipMatches.run(pd, td, b.data, b.off, flags=mflags)
    return mt.replace(rp, b.data, b.off)


def both_forms(hip, starts, ends, n, table, inserts, mflags=0, host=True, rp=None):
    rows, lens = inputs_of("kw_ends")
    pd, td = starts_image(starts), ends_image(ends)
    b = Batch(*lead_packed(rows[:n], lens[:n]))
    rp = hip.HipRepl.template(table, inserts) if rp is None else rp
    want = template_ref.replace(rows[:n], lens[:n], lens[:n], matches_ref.head(reference(starts, ends, mflags), n), table, inserts)
    check(device_form(hip, pd, td, b, rp, mflags), want, (starts, ends, n, "device"))
    if host:
        check(host_form(hip, pd, td, b, rp, mflags), want, (starts, ends, n, "host"))
    return want


# ---- group 1: every size, one table of mixed templates -----------------------------------------------------------------------

def test_every_size_with_a_mixed_template(hip):
    table, inserts = parsed(MIXED)
    assert inserts == [[0], [1], [0, 0], [17], []] and [len(x) for x in table] == [0, 2, 0, 57, 5]
    rp = hip.HipRepl.from_sed(MIXED)                                        # the binding's parser: the same table
    assert rp.inserts == 5 and rp.in_lds and rp.nrepl == 5
    _, lens = inputs_of("kw_ends")
    for n in SIZES:
        off, _ = both_forms(hip, "kw_starts", "kw_ends", n, table, inserts, host=n in (1, 257, 1500), rp=rp)
    out = np.diff(off.astype(np.int64))
    print("lines that grow / stay:", (out > lens).mean(), (out == lens).mean(), "output blocks:", int(off[-1]) / BLOCK)
    assert (out > lens).mean() >= 0.2 and (out == lens).mean() >= 0.02 and (out >= lens).all()      # from the judge alone
    assert int(off[-1]) > 2 * BLOCK
    # ids beyond the table stay: the first three rules only, d and bdb are left alone
    res = reference("kw_starts", "kw_ends")
    assert (res["id"] >= 3).mean() >= 0.1
    for n in (257, 1500):
        both_forms(hip, "kw_starts", "kw_ends", n, table[:3], inserts[:3], host=False)


def test_text_replace_over_a_text_and_its_hits(hip):
    pd, td = starts_image("kw_starts"), ends_image("kw_ends")
    rng = np.random.RandomState(18)
    lines = [bytes(rng.choice(list(b"abcdx" if i % 3 else b"xyzw"), rng.randint(0, 61)).astype(np.uint8)) for i in range(400)]
    lines[-1] = b"xxabcabd"
    blob = b"".join(x + b"\n" for x in lines)[:-1]
    text = hip.HipText(blob, 0x0A)
    assert text.lines == len(lines)
    rows, lens = span_ref.rows_of(lines)
    with_nl = [x + b"\n" for x in lines[:-1]] + [lines[-1]]
    raw_rows, raws = span_ref.rows_of(with_nl)
    mt_ref = judged("kw_starts", "kw_ends", rows, lens)
    res = dict(off=mt_ref[0], start=mt_ref[1], end=mt_ref[2], id=mt_ref[3])
    table, inserts = parsed(MIXED)
    rp = hip.HipRepl.template(table, inserts)
    want = template_ref.replace(raw_rows, lens, raws, mt_ref, table, inserts)
    assert bytes(want[1]).count(b"\n") == len(lines) - 1 and bytes(want[1]).endswith(b"xx<abc>ab" + SEVENTEEN + b"d" + FORTY)
    check(td.text_matches(pd, text).text_replace(rp, text), want, "text")
    ld = hip.LinesDfa(span_ref.line_matcher_of(KEYWORDS)[0], 0x0A)
    hits = text.hits(ld)
    assert 100 < hits.count < 300
    picks = hits.lines().astype(np.int64)
    sel = template_ref.replace(raw_rows[picks], lens[picks], raws[picks], matches_ref.select(res, picks), table, inserts)
    check(td.text_matches(pd, text, hits).text_replace(rp, text, hits), sel, "hits")
    none = text.hits(ld, invert=True)                                       # lines without a match: the lines themselves
    picks = none.lines().astype(np.int64)
    sel = template_ref.replace(raw_rows[picks], lens[picks], raws[picks], matches_ref.select(res, picks), table, inserts)
    assert template_ref.lines_of(*sel) == [with_nl[i] for i in picks] and len(picks) > 100
    check(td.text_matches(pd, text, none).text_replace(rp, text, none), sel, "no hits")


# ---- group 2: empty matches ----------------------------------------------------------------------------------------------------

def test_an_empty_match_gives_the_literal(hip):
    """`ends` accepts the empty string as rule EMPTY_RULE and every position is a start: an empty match has no bytes to insert,
    X = R[i] -- <> wherever no word begins; dropped, nothing is inserted"""
    starts, ends = "kw_starts_everywhere", "kw_ends_empty_ids"
    kept, dropped = reference(starts, ends), reference(starts, ends, DROP_EMPTY)
    empty = kept["end"] == kept["start"]
    assert empty.sum() >= 1000 and (kept["id"][empty] == EMPTY_RULE).all() and len(dropped["start"]) == int((~empty).sum())
    table, inserts = parsed(MIXED + [b"<&&>"])
    for n in (65, 1500):
        a, _ = both_forms(hip, starts, ends, n, table, inserts, host=n == 65)
        d, _ = both_forms(hip, starts, ends, n, table, inserts, mflags=DROP_EMPTY, host=False)
        assert int(a[-1]) == int(d[-1]) + 2 * int(empty[:int(kept["off"][n])].sum())
    both_forms(hip, starts, ends, 257, *parsed([b"", b"", b"", b"", b"", b"&-&"]), host=False)   # only the literal is left where words were


# ---- group 3: one match longer than two output blocks; the edges of the text --------------------------------------------------

@functools.lru_cache(maxsize=None)
def long_line_matches():
    """(lines, rows, lens, matches) of three lines whose middle one is LONG times d, ONE match of the pair d_starts / d_plus.
    The matches' judge walks `ends` from every start to the line's end, which is quadratic in the line: for the long line its
    table E (the farthest end from every start) is stated instead, by the law that the judge itself shows on a line of 200: d+ has
    one live state that loops, so from every s < len the farthest end is len, and from len there is none.  M (the starts) is the
    judge's own, and so is the cursor loop over M and E."""
    starts, ends = auto_of("d_starts")[0], auto_of("d_plus")[0]
    ids = state_ids("d_plus")
    r, l = span_ref.rows_of([b"d" * 200])
    E, Q = matches_ref.longest_from(ends, r, l)
    assert (E[0, :200] == 200).all() and E[0, 200] == -1 and (Q[0, :200] == 1).all()
    r, l = span_ref.rows_of([b"d" * LONG])
    E = np.full((1, LONG + 1), LONG, np.int64)
    E[0, LONG] = -1
    Q = np.where(E >= 0, 1, -1)
    big = matches_ref.matches(starts, ends, r, l, ids=ids, tables=(matches_ref.marks(starts, r, l), E, Q))
    assert big["start"].tolist() == [0] and big["end"].tolist() == [LONG] and big["id"].tolist() == [0]
    lines = [b"xddxdxx", b"d" * LONG, b"dxxdd"]
    rows, lens = span_ref.rows_of(lines)
    small = [matches_ref.matches(starts, ends, *span_ref.rows_of([x]), ids=ids) for x in (lines[0], lines[2])]
    parts = [small[0], big, small[1]]
    off = np.r_[0, np.cumsum([len(p["start"]) for p in parts])].astype(np.uint64)
    mt = (off,) + tuple(np.concatenate([p[k] for p in parts]) for k in ("start", "end", "id"))
    assert off.tolist() == [0, 2, 3, 5]
    return lines, rows, lens, mt, (big["off"], big["start"], big["end"], big["id"])


def test_one_match_longer_than_two_blocks(hip):
    """[&|&] around 40 000 bytes: chunks wholly inside the match's copies cross block boundaries, and the seam between the copies"""
    lines, rows, lens, mt, _ = long_line_matches()
    pd, td = starts_image("d_starts"), ends_image("d_plus")
    table, inserts = parsed([b"[&|&]"])
    want = template_ref.replace(rows, lens, lens, mt, table, inserts)
    out = template_ref.lines_of(*want)
    assert out[1] == b"[" + b"d" * LONG + b"|" + b"d" * LONG + b"]" and out[0] == b"x[dd|dd]x[d|d]xx" and int(want[0][-1]) > 4 * BLOCK
    first = int(want[0][1]) + 1                                             # where the first copy begins in the output
    assert first // BLOCK + 2 <= (first + LONG) // BLOCK                    # two block boundaries inside the first copy
    assert (first + LONG) % 16 not in (0, 15)                               # the seam | and bytes of both copies in one chunk
    rp = hip.HipRepl.template(table, inserts)
    b = Batch(*lead_packed(rows, lens))
    check(device_form(hip, pd, td, b, rp), want, "long, device")
    check(host_form(hip, pd, td, b, rp), want, "long, host")
    rg = hip.HipRepl.template(table + [b"u" * (BLOCK + 1)], inserts + [[7]])                   # the same from device memory
    assert not rg.in_lds
    check(device_form(hip, pd, td, b, rg), want, "long, table in device memory")


def test_the_match_is_the_whole_text(hip):
    """the long line alone, LEAD = 0 and no byte behind it: the match begins at the first byte of the text and ends at its last, so
    the windows of the stretches at both ends of each copy would leave the text: the byte loads under `limit`"""
    _, _, _, _, mt = long_line_matches()
    rows, lens = span_ref.rows_of([b"d" * LONG])
    pd, td = starts_image("d_starts"), ends_image("d_plus")
    data, off = lead_packed(rows, lens, lead=0)
    assert len(data) == LONG and off.tolist() == [0, LONG]
    for seds in ([b"[&|&]"], [b"&&"], [b"&<\\&>&"]):
        table, inserts = parsed(seds)
        want = template_ref.replace(rows, lens, lens, mt, table, inserts)
        check(device_form(hip, pd, td, Batch(data, off), hip.HipRepl.template(table, inserts)), want, seds)
    # ... and short texts that are one match: the first chunk holds the text's first byte, the last its last
    for k in (1, 15, 16, 17, 33):
        rows, lens = span_ref.rows_of([b"d" * k])
        data, off = lead_packed(rows, lens, lead=0)
        table, inserts = parsed([b"&-&&"])
        want = template_ref.replace(rows, lens, lens, judged("d_starts", "d_plus", rows, lens), table, inserts)
        assert bytes(want[1]) == b"d" * k + b"-" + b"d" * 2 * k
        check(device_form(hip, pd, td, Batch(data, off), hip.HipRepl.template(table, inserts)), want, ("whole text", k))


def test_three_inserts_in_an_empty_literal(hip):
    """&&& on lines of 8-12 bytes: a chunk of 16 output bytes holds the copies of several matches"""
    rng = np.random.RandomState(23)
    pieces = KEYWORDS + [b"x"]
    lines = [b"".join(pieces[k] for k in rng.randint(0, len(pieces), 12))[:rng.randint(8, 13)] for _ in range(300)]
    rows, lens = span_ref.rows_of(lines)
    mt = judged("kw_starts", "kw_ends", rows, lens)
    assert len(mt[1]) >= 3 * len(lines)
    table, inserts = parsed([b"&&&"] * len(KEYWORDS))
    assert table == [b""] * 5 and inserts == [[0, 0, 0]] * 5
    want = template_ref.replace(rows, lens, lens, mt, table, inserts)
    assert template_ref.lines_of(*want)[:300] and int(want[0][-1]) > 2 * int(lens.sum())
    pd, td = starts_image("kw_starts"), ends_image("kw_ends")
    b = Batch(*lead_packed(rows, lens))
    rp = hip.HipRepl.template(table, inserts)
    check(device_form(hip, pd, td, b, rp), want, "&&&, device")
    check(host_form(hip, pd, td, b, rp), want, "&&&, host")


# ---- group 4: the table from LDS and from device memory ---------------------------------------------------------------------

def test_template_table_in_lds_and_in_device_memory(hip):
    rows, lens = inputs_of("kw_ends")
    n = 600
    table, inserts = parsed(MIXED)
    bound, rules = hip.repl_lds_bytes(), hip.repl_lds_rules()
    assert (bound, rules) == (16384, 1023)
    more = rules + 1 - len(table)
    used = sum((len(x) for x in table))
    tables = {
        "small": (table, inserts, True),
        "more than 1 023 rules": (table + [b"r%d" % i for i in range(more)], inserts + [[i % 3] for i in range(more)], False),
        "above the byte budget": (table + [b"u" * (bound + 1 - used)], inserts + [[0, 9, bound + 1 - used]], False),
        # 16 rules of 255 inserts: 4 080 positions are 8 160 bytes of LDS, next to 9 000 bytes of table
        "no room for the inserts": (table + [b"v" * 560] * 16, inserts + [list(range(255))] * 16, False),
        "room for the inserts": (table + [b"v" * 400] * 16, inserts + [list(range(255))] * 16, True),
    }
    pd, td = starts_image("kw_starts"), ends_image("kw_ends")
    b = Batch(*lead_packed(rows[:n], lens[:n]))
    first = None
    for what, (tb, ins, in_lds) in tables.items():
        rp = hip.HipRepl.template(tb, ins)
        assert rp.in_lds == in_lds, what
        assert rp.inserts == sum(len(a) for a in ins)
        want = template_ref.replace(rows[:n], lens[:n], lens[:n], matches_ref.head(reference("kw_starts", "kw_ends"), n), tb, ins)
        first = want if first is None else first
        assert np.array_equal(want[0], first[0]) and np.array_equal(want[1], first[1])        # the same bytes expected
        check(device_form(hip, pd, td, b, rp), want, what)
    # a rule of 255 inserts read from device memory (1 034 rules), and a position at the end of a literal above the byte budget
    far = [b""] * 3 + [bytes(range(255))] + [b""] * 1030
    far_ins = [[]] * 3 + [list(range(255))] + [[]] * 1030
    rp = hip.HipRepl.template(far, far_ins)
    assert not rp.in_lds and rp.inserts == 255
    want = template_ref.replace(rows[:65], lens[:65], lens[:65], matches_ref.head(reference("kw_starts", "kw_ends"), 65), far, far_ins)
    check(device_form(hip, pd, td, Batch(*lead_packed(rows[:65], lens[:65])), rp), want, "255 inserts, device memory")
    big = [b"p" * 19960, b"", b"", bytes(range(40))]
    big_ins = [[19960], [], [], [0, 40]]
    rp = hip.HipRepl.template(big, big_ins)
    assert not rp.in_lds
    want = template_ref.replace(rows[:16], lens[:16], lens[:16], matches_ref.head(reference("kw_starts", "kw_ends"), 16), big, big_ins)
    check(device_form(hip, pd, td, Batch(*lead_packed(rows[:16], lens[:16])), rp), want, "far end")


def test_a_template_table_without_inserts_is_the_plain_table(hip):
    rows, lens = inputs_of("kw_ends")
    table = [b"<AB>", b"", b"c", bytes(range(0x30, 0x30 + 40)), b"seventeen bytes.."]
    pd, td = starts_image("kw_starts"), ends_image("kw_ends")
    b = Batch(*lead_packed(rows, lens))
    want = replace_ref.replace(rows, lens, lens, matches_ref.head(reference("kw_starts", "kw_ends"), 1500), table)
    got = []
    for what, rp in (("plain", hip.HipRepl(table)), ("ioff NULL", hip.HipRepl.template(table, None)), ("every c = 0", hip.HipRepl.template(table, [[]] * 5))):
        assert rp.inserts == 0 and rp.in_lds, what
        got.append(check(device_form(hip, pd, td, b, rp), want, what))
    for off, data in got[1:]:
        assert np.array_equal(off, got[0][0]) and np.array_equal(data, got[0][1])
    # ... under the plain table's own LDS rule: at the byte bound the inserts' room is not asked for
    at = [b"u" * 16384]
    assert hip.HipRepl.template(at, None).in_lds and hip.HipRepl.template(at, [[]]).in_lds and not hip.HipRepl.template(at, [[0]]).in_lds
    assert hip.HipRepl.template([], None).inserts == 0 and hip.HipRepl.template([], []).in_lds


# ---- group 5: refusals ----------------------------------------------------------------------------------------------------------

def test_refusals_with_a_device(hip):
    """EINVAL before any upload, and the next call answers"""
    rows, lens = inputs_of("kw_ends")
    lib = hip.load_library()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    u64 = lambda *a: np.array(a, np.uint64)           # noqa: E731
    table = [b"<>", b"", b"abc"]
    tb, roff = replace_ref.pack_table(table)
    good_ioff, good_ins = u64(0, 1, 1, 3), u64(1, 0, 3)
    many = np.zeros(256, np.uint64)
    cases = {
        "the MASK flag": (ptr(tb), ptr(roff), 3, ptr(good_ins), ptr(good_ioff), 1),
        "another flag": (ptr(tb), ptr(roff), 3, ptr(good_ins), ptr(good_ioff), 2),
        "MASK without inserts": (ptr(tb), ptr(roff), 3, None, None, 1),
        "ioff descends": (ptr(tb), ptr(roff), 3, ptr(good_ins), ptr(u64(0, 2, 1, 3)), 0),
        "ioff[0] != 0": (ptr(tb), ptr(roff), 3, ptr(good_ins), ptr(u64(1, 1, 1, 3)), 0),
        "a position > |R[i]|": (ptr(tb), ptr(roff), 3, ptr(u64(3, 0, 3)), ptr(good_ioff), 0),
        "a position > |R[i]| = 0": (ptr(tb), ptr(roff), 3, ptr(u64(1, 1, 3)), ptr(u64(0, 1, 2, 3)), 0),
        "positions descend": (ptr(tb), ptr(roff), 3, ptr(u64(1, 2, 1)), ptr(good_ioff), 0),
        "256 inserts in a rule": (ptr(tb), ptr(roff), 3, ptr(many), ptr(u64(0, 0, 0, 256)), 0),
        "ins NULL with inserts": (ptr(tb), ptr(roff), 3, None, ptr(good_ioff), 0),
        "roff NULL": (ptr(tb), None, 3, ptr(good_ins), ptr(good_ioff), 0),
        "bytes NULL": (None, ptr(roff), 3, ptr(good_ins), ptr(good_ioff), 0),
    }
    for what, args in cases.items():
        C.set_errno(0)
        assert lib.fsm_hip_repl_create_template(*args) is None and C.get_errno() == errno.EINVAL, what
    with pytest.raises(OSError) as ei:
        hip.HipRepl.template(table, [[1], [], [0, 3]], flags=hip.REPL_MASK)
    assert ei.value.errno == errno.EINVAL
    with pytest.raises(ValueError):
        hip.HipRepl.template(table, [[1]])
    # the plain entry point still refuses what it refused
    C.set_errno(0)
    assert lib.fsm_hip_repl_create(ptr(tb), ptr(roff), 3, 2) is None and C.get_errno() == errno.EINVAL
    # the good arrays are accepted, and 255 inserts in a rule are: judged on 65 lines
    h = lib.fsm_hip_repl_create_template(ptr(tb), ptr(roff), 3, ptr(good_ins), ptr(good_ioff), 0)
    assert h is not None and lib.fsm_hip_repl_inserts(h) == 3 and lib.fsm_hip_repl_in_lds(h) == 1
    lib.fsm_hip_repl_free(h)
    cap = [b"", b"", b"", b"0123456789", b""]
    cap_ins = [[], [], [], sorted(list(range(11)) * 24)[:255], []]              # d -> 255 times d among ten digits
    assert len(cap_ins[3]) == hip.HipRepl.max_inserts() == 255
    want = both_forms(hip, "kw_starts", "kw_ends", 65, cap, cap_ins, host=False)
    assert int(np.diff(want[0].astype(np.int64))[8]) == 300 * (10 + 255)


# ---- group 6: the example -------------------------------------------------------------------------------------------------------

def test_example_with_templates(hip, tmp_path):
    """examples/hipsed.c -t over three files, the second without a final newline: stdout is the judge's text; without -t an
    argument that holds & is a literal"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.RandomState(17)
    files = [[bytes(rng.choice(list(b"abcdxyzw" if i % 2 == 0 else b"xyzwba"), rng.randint(0, 25)).astype(np.uint8)) for i in range(k)] for k in (70, 40, 25)]
    files[1][-1] = b"xxabcabd"
    tables = []
    for nm, auto in (("lines", span_ref.line_matcher_of(KEYWORDS)), ("starts", auto_of("kw_starts")[0]), ("ends", auto_of("kw_ends")[0])):
        tables.append(str(tmp_path / (nm + ".fsmhip")))
        auto[0].write_c(tables[-1])
    names = []
    for j, ls in enumerate(files):
        data = b"".join(x + b"\n" for x in ls)
        p = tmp_path / ("f%d.txt" % j)
        p.write_bytes(data[:-1] if j == 1 else data)
        names.append(str(p))
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    exe = str(tmp_path / "hipsed")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "hipsed.c"),
                           "-o", exe, "-L" + os.path.join(root, "libfsm_amd"), "-lfsm_hip", "-Wl,-rpath," + os.path.join(root, "libfsm_amd")])

    def run(*args):
        r = subprocess.run([exe, *args, "--", *names], capture_output=True, env=env, timeout=120)
        return r.returncode, r.stdout

    def compose(table, inserts):
        out = b""
        for j, ls in enumerate(files):
            rows, lens = span_ref.rows_of(ls)
            with_nl = [x + b"\n" for x in ls]
            if j == 1:
                with_nl[-1] = ls[-1]
            raw_rows, raws = span_ref.rows_of(with_nl)
            out += bytes(template_ref.replace(raw_rows, lens, raws, judged("kw_starts", "kw_ends", rows, lens), table, inserts)[1])
        return out

    seds = ["<b>&</b>", "(&)", "\\&&\\\\", "&&", "plain"]
    table, inserts = parsed([x.encode() for x in seds])
    assert table == [b"<b></b>", b"()", b"&\\", b"", b"plain"] and inserts == [[3], [1], [1], [0, 0], []]
    want = compose(table, inserts)
    assert want.count(b"\n") == 134 and b"xx(abc)<b>ab</b>dd" in want and b"&ca\\" in want
    assert run("-t", *tables, *seds) == (0, want)
    assert run("-t", *tables, *seds[:2]) == (0, compose(table[:2], inserts[:2]))       # rules without a REPL stay
    literal = compose([x.encode() for x in seds], None)                                # without -t: every byte of REPL as it is
    assert b"<b>&</b>" in literal and literal != want
    assert run(*tables, *seds) == (0, literal)
    for args in (("-t", "-m"), ("-m", "-t")):                                          # a usage error
        code, out = run(*args, *tables, *seds)
        assert (code, out) == (2, b"")
    assert run("-t", *tables, "ends in \\")[0] == 2
