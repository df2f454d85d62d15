"""GPU: the replacement (libfsm_amd/csrc/replace.hip: repl_lengths, repl_offsets, repl_write<LDS / global table> and the fronts;
the scan of the block sums in text.hip).

out_off and every output byte are compared with tests/replace_ref.py, the definition of include/fsm_hip.h ("replace") restated
in Python, over the matches of tests/matches_ref.py -- never over matches or offsets that came from the device.  The inputs, the
automata and the matches' judge are tests/line_inputs.py's: 1 500 rows of at most 300 bytes with lengths 0, 1, 15, 16, 17, 31, 32,
33, ..., line 8 = 300 times d, and LEAD = 5 bytes in front of the text that belong to no line."""
import ctypes as C
import errno
import os
import subprocess

import numpy as np
import pytest

import matches_ref
import replace_ref
import span_ref
from line_inputs import (EMPTY_RULE, FILL, KEYWORDS, SIZES, auto_of, device_u64, device_u8, ends_image, inputs_of, judged, lead_packed, reference,
                         starts_image)
from matches_ref import DROP_EMPTY
from replace_ref import MASK

pytestmark = pytest.mark.gpu

TABLE_LENS = (0, 1, 15, 16, 17, 40)     # per rule, mixed in one table: chunks straddle every kind of boundary, lines grow and shrink


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()   # raises if the HIP extension is missing: no silent fallback
    return libfsm_amd


def mixed_table(nrepl, seed=0, shift=0):
    """nrepl replacements of the lengths TABLE_LENS in turn (from entry `shift` on), their bytes telling rule and position apart"""
    return [bytes((0x80 + 7 * i + t + seed) % 256 for t in range(TABLE_LENS[(i + shift) % len(TABLE_LENS)])) for i in range(nrepl)]


def table_for(res, top=60):
    """a mixed table (40, 0, 1, ... bytes) that covers about half of the ids that occur (the others stay), at most `top` rules"""
    ids = np.unique(res["id"][res["id"] < 0xFFFFFFFE]).astype(np.int64)
    assert len(ids) >= 2
    return mixed_table(int(min(ids[len(ids) // 2] + 1, top)), shift=5)


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


class Batch:
    """a packed text on the device and on the host"""

    def __init__(self, data, off, pick=None):
        self.data, self.off, self.pick = data, off, pick
        self.n = len(off) - 1
        self.d_data = device_u8(data) if len(data) else None
        self.d_off = device_u64(off)
        self.d_pick = device_u64(pick if len(pick) else np.zeros(1, np.uint64)) if pick is not None else None

    def device_args(self, limit=None):
        return dict(d_base=self.d_data.data_ptr() if self.d_data is not None else 0, d_off=self.d_off.data_ptr(), n=self.n,
                    d_pick=self.d_pick.data_ptr() if self.d_pick is not None else 0, m=len(self.pick) if self.pick is not None else 0,
                    limit=len(self.data) if limit is None else limit)


def device_form(hip, pd, td, b, table, flags=0, mflags=0, trim_byte=-1, limit=None):
    """matches_run_device, then matches_replace_device on the same batch"""
    import torch
    mt = hip.HipMatches.run_device(pd, td, trim_byte=trim_byte, flags=mflags, **b.device_args(limit))
    rp = table if isinstance(table, hip.HipRepl) else hip.HipRepl(table, flags)
    rd = mt.replace_device(rp, trim_byte=trim_byte, **b.device_args(limit))
    torch.cuda.synchronize()
    rd._keep = (rd._keep, b)
    return rd


def host_form(hip, pd, td, b, table, flags=0, mflags=0, trim_byte=-1):
    mt = hip.HipMatches.run(pd, td, b.data, b.off, pick=b.pick, trim_byte=trim_byte, flags=mflags)
    return mt.replace(hip.HipRepl(table, flags), b.data, b.off, pick=b.pick, trim_byte=trim_byte)


def both_forms(hip, starts, ends, n, table, flags=0, mflags=0, host=True):
    rows, lens = inputs_of(ends)
    pd, td = starts_image(starts), ends_image(ends)
    data, off = lead_packed(rows[:n], lens[:n])
    b = Batch(data, off)
    want = replace_ref.replace(rows[:n], lens[:n], lens[:n], matches_ref.head(reference(starts, ends, mflags), n), table, flags)
    check(device_form(hip, pd, td, b, table, flags, mflags), want, (starts, ends, n, flags, "device"))
    if host:
        check(host_form(hip, pd, td, b, table, flags, mflags), want, (starts, ends, n, flags, "host"))
    return want


# ---- group 1: every input, every size, a table of mixed lengths ------------------------------------------------------------

@pytest.mark.parametrize("starts,ends", [("lds_full", "glob_first"), ("glob_first", "lds_full"), ("s15_start", "lds_full"), ("kw_starts", "kw_ends")])
def test_every_size_with_a_mixed_table(hip, starts, ends):
    res = reference(starts, ends)
    table = mixed_table(len(KEYWORDS)) if ends == "kw_ends" else table_for(res)
    replaced = (res["id"] < len(table)).mean()
    _, lens = inputs_of(ends)
    for n in SIZES:
        off, _ = both_forms(hip, starts, ends, n, table, host=n in (1, 257, 1500))
    out = np.diff(off.astype(np.int64))
    print(starts, ends, "rules:", len(table), "matches replaced:", replaced, "lines that grow / shrink:", (out > lens).mean(), (out < lens).mean(),
          "output blocks:", int(off[-1]) / 16384)
    assert 0.2 <= replaced <= (1.0 if ends == "kw_ends" else 0.8) and (out > lens).mean() >= 0.02 and (out < lens).mean() >= 0.02
    assert int(off[-1]) > 2 * 16384                                       # several blocks of the write pass
    # the other lengths of TABLE_LENS for the same rules (16, 17, 40, 0, 1 for the keywords; 15, 16, 17 for the others), and the
    # identity: a table without a rule
    other = mixed_table(len(table), seed=1, shift=3 if ends == "kw_ends" else 2)
    assert {len(x) for x in table} | {len(x) for x in other} == set(TABLE_LENS)
    for n in (257, 1500):
        both_forms(hip, starts, ends, n, other, host=False)
    both_forms(hip, starts, ends, 1500, [])


# ---- group 2: lines that vanish --------------------------------------------------------------------------------------------

def test_every_rule_empty_lines_vanish(hip):
    rows, lens = inputs_of("kw_ends")
    table = [b""] * len(KEYWORDS)
    off, data = both_forms(hip, "kw_starts", "kw_ends", 1500, table)
    out = np.diff(off.astype(np.int64))
    gone = (out == 0) & (lens > 0)
    runs = np.diff(np.flatnonzero(np.r_[1, out != 0, 1])) - 1               # runs of empty output lines
    print("lines that vanish:", gone.sum(), "longest run of empty output lines:", runs.max(), "bytes left:", int(off[-1]))
    assert gone.sum() >= 30 and runs.max() >= 2 and (out > 0).sum() >= 500
    assert not (set(bytes(data)) & set(b"d"))                               # no d is left anywhere
    for n in (63, 257):
        both_forms(hip, "kw_starts", "kw_ends", n, table)
    # a text made only of matches, no trim: 0 bytes, a valid object, bytes NULL, nothing stored
    lines = [b"abd", b"dd", b"", b"abcca", b"bdbab"] * 60
    r, l = span_ref.rows_of(lines)
    b = Batch(*lead_packed(r, l))
    want = replace_ref.replace(r, l, l, judged("kw_starts", "kw_ends", r, l), table)
    assert int(want[0][-1]) == 0 and len(want[0]) == 301
    pd, td = starts_image("kw_starts"), ends_image("kw_ends")
    rd = device_form(hip, pd, td, b, table)
    assert rd.nbytes == 0 and rd.bytes_ptr == 0 and rd.off_ptr != 0
    check(rd, want, "nothing left, device")
    check(host_form(hip, pd, td, b, table), want, "nothing left, host")
    # ... and one byte left in the middle of 300 empty output lines
    lines[150] = b"abxd"
    r, l = span_ref.rows_of(lines)
    b = Batch(*lead_packed(r, l))
    want = replace_ref.replace(r, l, l, judged("kw_starts", "kw_ends", r, l), table)
    assert bytes(want[1]) == b"x"
    check(device_form(hip, pd, td, b, table), want, "one byte left")


def test_more_lines_than_a_block_of_the_offsets_pass(hip):
    """m = three blocks of the lengths / offsets pass + 1 (fsm_hip_replaced_block_lines() = 256: 769 inputs), lines of 0-12 bytes of
    which about half are empty after the replacement: the block bases, the block's own scan and runs of empty lines across blocks"""
    B = hip.replaced_block_lines()
    assert B == 256
    m = 3 * B + 1
    rng = np.random.RandomState(41)
    lines = []
    for i in range(m):
        k = rng.randint(0, 13)
        if rng.randint(0, 2):
            lines.append((b"d" * 12)[:k])                                   # matches alone: vanishes
        else:
            lines.append(bytes(rng.choice(list(b"abcdxy"), k).astype(np.uint8)))
    r, l = span_ref.rows_of(lines)
    table = [b""] * len(KEYWORDS)
    mt = judged("kw_starts", "kw_ends", r, l)
    want = replace_ref.replace(r, l, l, mt, table)
    out = np.diff(want[0].astype(np.int64))
    print("empty after the replacement:", (out == 0).mean())
    assert 0.4 <= (out == 0).mean() <= 0.7 and (out[B - 3:B + 3] == 0).any() and out[2 * B:].sum() > 0
    pd, td = starts_image("kw_starts"), ends_image("kw_ends")
    b = Batch(*lead_packed(r, l))
    check(device_form(hip, pd, td, b, table), want, "three blocks + 1, device")
    check(host_form(hip, pd, td, b, table), want, "three blocks + 1, host")
    grow = mixed_table(len(KEYWORDS), 3)
    check(device_form(hip, pd, td, b, grow), replace_ref.replace(r, l, l, mt, grow), "three blocks + 1, mixed table")


# ---- group 3: MASK, empty matches, many matches in a line -------------------------------------------------------------------

def test_mask_keeps_every_length(hip):
    rows, lens = inputs_of("kw_ends")
    table = [b"*", b"#@!", b"", b"xy"]                                      # |R| 1 and 3, |R| = 0 stays, rule 4 is beyond nrepl: stays
    for n in (257, 1500):
        off, data = both_forms(hip, "kw_starts", "kw_ends", n, table, MASK)
        rel = np.r_[0, np.cumsum(lens[:n])].astype(np.uint64)
        assert np.array_equal(off, rel)                                     # out_off == the input's own relative offsets
    text = bytes(data)
    assert b"bdb" in text and b"ca" in text and b"#@" in text and b"*" in text
    # the same table without the flag changes lengths
    off2, _ = both_forms(hip, "kw_starts", "kw_ends", 257, table)
    assert not np.array_equal(off2, np.r_[0, np.cumsum(lens[:257])].astype(np.uint64))


def test_empty_matches_insert_or_are_dropped(hip):
    """`ends` accepts the empty string as rule EMPTY_RULE and every position is a start: kept, the rule's replacement is inserted
    wherever no word begins; dropped, nothing is"""
    starts, ends = "kw_starts_everywhere", "kw_ends_empty_ids"
    kept, dropped = reference(starts, ends), reference(starts, ends, DROP_EMPTY)
    empty = kept["end"] == kept["start"]
    assert empty.sum() >= 1000 and (kept["id"][empty] == EMPTY_RULE).all() and len(dropped["start"]) == int((~empty).sum())
    table = mixed_table(len(KEYWORDS)) + [b"<>"]
    for n in (65, 1500):
        a, _ = both_forms(hip, starts, ends, n, table)
        d, _ = both_forms(hip, starts, ends, n, table, mflags=DROP_EMPTY)
        assert int(a[-1]) >= int(d[-1]) + 2 * int(empty[:int(kept["off"][n])].sum())
    both_forms(hip, starts, ends, 257, table[:len(KEYWORDS)])                  # the empty rule beyond nrepl: nothing is inserted
    both_forms(hip, starts, ends, 257, [b"", b"", b"", b"", b"", b"-"])      # only inserts are left where words were
    both_forms(hip, starts, ends, 257, table, MASK)                         # an empty match has no byte to mask


def test_300_matches_in_one_line(hip):
    rows, lens = inputs_of("kw_ends")
    res = reference("kw_starts", "kw_ends")
    off = res["off"].astype(np.int64)
    assert int(lens[8]) == 300 and off[9] - off[8] == 300
    table = [b"", b"1", b"fifteen bytes..", bytes(range(0x30, 0x30 + 40)), b"seventeen bytes.."]      # d -> 40 bytes
    assert [len(x) for x in table] == [0, 1, 15, 40, 17]
    out, _ = both_forms(hip, "kw_starts", "kw_ends", 16, table)
    assert int(out[9] - out[8]) == 300 * 40                                 # 12 000 bytes out of 300
    both_forms(hip, "kw_starts", "kw_ends", 16, [b"", b"", b"", b""])       # ... and 0 bytes out of 300
    both_forms(hip, "kw_starts", "kw_ends", 16, [b"", b"", b"", b"Z"], MASK)


# ---- group 4: trim, pick, limit --------------------------------------------------------------------------------------------

def test_trim_byte_is_copied(hip):
    rows, lens = inputs_of("kw_ends")
    pd, td = starts_image("kw_starts"), ends_image("kw_ends")
    n, trim = 600, 0x0A
    rows = rows[:n].copy()
    lens = lens[:n].copy()
    idx = np.arange(n)
    ends_in = (idx % 3 == 0) & (lens > 0)
    rows[idx[ends_in], lens[ends_in] - 1] = trim                            # lines ending in the byte; the others never hold it
    lens[10], lens[11] = 1, 0
    rows[10, 0] = trim
    ends_in[10], ends_in[11] = True, False
    shorter = lens - ends_in
    assert ends_in.sum() > 100 and (~ends_in & (lens > 0)).sum() > 100
    b = Batch(*lead_packed(rows, lens))
    table = mixed_table(len(KEYWORDS), 5)
    mt = judged("kw_starts", "kw_ends", rows, shorter)
    want = replace_ref.replace(rows, shorter, lens, mt, table)
    assert bytes(want[1]).count(b"\n") == int(ends_in.sum())
    check(device_form(hip, pd, td, b, table, trim_byte=trim), want, "trim, device")
    check(host_form(hip, pd, td, b, table, trim_byte=trim), want, "trim, host")
    gone = replace_ref.replace(rows, shorter, lens, mt, [b""] * 5)           # a line of words alone keeps its delimiter only
    assert (np.diff(gone[0].astype(np.int64))[ends_in] >= 1).all()
    check(device_form(hip, pd, td, b, [b""] * 5, trim_byte=trim), gone, "trim, every rule empty")


@pytest.mark.parametrize("starts,ends", [("glob_first", "lds_full"), ("kw_starts", "kw_ends")])
def test_pick_and_limit(hip, starts, ends):
    rows, lens = inputs_of(ends)
    pd, td = starts_image(starts), ends_image(ends)
    n = 700
    data, off = lead_packed(rows[:n], lens[:n])
    rng = np.random.RandomState(12)
    pick = np.concatenate([rng.permutation(n)[:300], [7, 7, 7, 0, n - 1, n - 1, 8, 8], rng.randint(0, n, 100), np.arange(n)[::-1][:50]]).astype(np.uint64)
    res = reference(starts, ends)
    table = mixed_table(len(KEYWORDS)) if ends == "kw_ends" else table_for(res)

    def want_of(p, nlines=n):
        ok = p < nlines
        at = np.where(ok, p, 0).astype(np.int64)
        ln = np.where(ok, lens[at], 0)
        return replace_ref.replace(rows[at], ln, ln, matches_ref.select(res, p, nlines), table)

    check(device_form(hip, pd, td, Batch(data, off, pick), table), want_of(pick), (starts, ends, "device"))
    check(host_form(hip, pd, td, Batch(data, off, pick), table), want_of(pick), (starts, ends, "host"))
    # an empty pick: a valid object, nothing launched that stores
    none = (np.zeros(1, np.uint64), np.zeros(0, np.uint8))
    check(device_form(hip, pd, td, Batch(data, off, np.zeros(0, np.uint64)), table), none, "m == 0 device", m=0)
    check(host_form(hip, pd, td, Batch(data, off, np.zeros(0, np.uint64)), table), none, "m == 0 host", m=0)
    # an index at or beyond n: an empty output line on the device form, its neighbours right; EINVAL on the host form
    wild = pick.copy()
    at = [0, 5, 255, 256, len(wild) - 1]
    wild[at] = [n, n + 1, 2 ** 40, 0xFFFFFFFFFFFFFFFF, n]
    want = want_of(wild)
    assert (np.diff(want[0].astype(np.int64))[at] == 0).all()
    check(device_form(hip, pd, td, Batch(data, off, wild), table), want, (starts, ends, "wild"))
    good = hip.HipMatches.run(pd, td, data, off, pick=pick)
    with pytest.raises(OSError) as ei:
        good.replace(hip.HipRepl(table), data, off, pick=wild)
    assert ei.value.errno == errno.EINVAL
    # a limit that cuts the last line (and the lines behind it): the judge on the clipped text; limit = 0 is off[n]
    n2 = 257
    data, off = lead_packed(rows[:n2], lens[:n2])
    b = Batch(data, off)
    check(device_form(hip, pd, td, b, table, limit=0), replace_ref.replace(rows[:n2], lens[:n2], lens[:n2], matches_ref.head(res, n2), table), "limit = 0")
    for cut in (int(off[n2]) - 3, int(off[200]) + 7):
        clipped = np.clip(cut - off[:n2].astype(np.int64), 0, lens[:n2])
        assert (clipped != lens[:n2]).sum() >= 1
        want = replace_ref.replace(rows[:n2], clipped, clipped, judged(starts, ends, rows[:n2], clipped), table)
        check(device_form(hip, pd, td, b, table, limit=cut), want, ("limit", cut))


# ---- group 5: the table from LDS and from device memory --------------------------------------------------------------------

def test_table_under_and_over_the_lds_bound(hip):
    rows, lens = inputs_of("kw_ends")
    n = 600
    words = mixed_table(len(KEYWORDS), 9)
    bound, rules = hip.repl_lds_bytes(), hip.repl_lds_rules()
    assert (bound, rules) == (16384, 1023)
    room = bound - sum(len(x) for x in words)
    tables = {"under": (words + [b"u" * (room - 1)], True), "at": (words + [b"u" * room], True), "one byte over": (words + [b"u" * (room + 1)], False),
              "rules at": (words + [b""] * (rules - len(words)), True), "one rule over": (words + [b""] * (rules + 1 - len(words)), False)}
    wants = None
    for what, (table, in_lds) in tables.items():
        rp = hip.HipRepl(table)
        assert rp.in_lds == in_lds, what
        b = Batch(*lead_packed(rows[:n], lens[:n]))
        want = replace_ref.replace(rows[:n], lens[:n], lens[:n], matches_ref.head(reference("kw_starts", "kw_ends"), n), table)
        if wants is None:
            wants = want
        assert np.array_equal(want[0], wants[0]) and np.array_equal(want[1], wants[1])      # the same bytes expected
        check(device_form(hip, starts_image("kw_starts"), ends_image("kw_ends"), b, rp), want, what)
    # the table's own bytes at its far end, from device memory: rule 3 (d) is the last 40 bytes of a table of 20 000
    big = [b"", b"", b"", bytes(range(40))]
    table = [b"p" * 19960] + big[1:]
    rp = hip.HipRepl(table, 0)
    assert not rp.in_lds
    want = replace_ref.replace(rows[:16], lens[:16], lens[:16], matches_ref.head(reference("kw_starts", "kw_ends"), 16), table)
    check(device_form(hip, starts_image("kw_starts"), ends_image("kw_ends"), Batch(*lead_packed(rows[:16], lens[:16])), rp), want, "far end")
    # one table, many calls
    rp = hip.HipRepl(words, MASK)
    for k in (65, 256):
        want = replace_ref.replace(rows[:k], lens[:k], lens[:k], matches_ref.head(reference("kw_starts", "kw_ends"), k), words, MASK)
        check(device_form(hip, starts_image("kw_starts"), ends_image("kw_ends"), Batch(*lead_packed(rows[:k], lens[:k])), rp), want, ("reused", k))


# ---- group 6: the text front, and the result as a text ---------------------------------------------------------------------

def text_lines(rng):
    """400 lines of 0-60 bytes over abcdx and, every third, over xyzw: a third without any word; the last without a newline"""
    out = []
    for i in range(400):
        alpha = b"abcdx" if i % 3 else b"xyzw"
        out.append(bytes(rng.choice(list(alpha), rng.randint(0, 61)).astype(np.uint8)))
    out[-1] = b"xxabcabd"
    return out


def test_text_replace_over_a_text_and_its_hits_and_the_result_fed_back(hip):
    import torch
    pd, td = starts_image("kw_starts"), ends_image("kw_ends")
    lines = text_lines(np.random.RandomState(18))
    blob = b"".join(x + b"\n" for x in lines)[:-1]
    text = hip.HipText(blob, 0x0A)
    assert text.lines == len(lines)
    rows, lens = span_ref.rows_of(lines)
    with_nl = [x + b"\n" for x in lines[:-1]] + [lines[-1]]
    raw_rows, raws = span_ref.rows_of(with_nl)
    mt_ref = judged("kw_starts", "kw_ends", rows, lens)
    res = dict(off=mt_ref[0], start=mt_ref[1], end=mt_ref[2], id=mt_ref[3])
    table = mixed_table(len(KEYWORDS), 2)
    rp = hip.HipRepl(table)
    want = replace_ref.replace(raw_rows, lens, raws, mt_ref, table)
    assert bytes(want[1]).count(b"\n") == len(lines) - 1 and not bytes(want[1]).endswith(b"\n")
    check(td.text_matches(pd, text).text_replace(rp, text), want, "text")
    # ... is the primitive over the text's own offsets with the delimiter trimmed, host and device form alike
    off = np.zeros(len(lines) + 1, np.uint64)
    off[1:] = np.cumsum(raws)
    b = Batch(np.frombuffer(blob, np.uint8), off)
    check(host_form(hip, pd, td, b, table, trim_byte=0x0A), want, "primitive, host")
    check(device_form(hip, pd, td, b, rp, trim_byte=0x0A), want, "primitive, device")
    ld = hip.LinesDfa(span_ref.line_matcher_of(KEYWORDS)[0], 0x0A)
    kinds = {"plain": text.hits(ld), "no bytes": text.hits(ld, want_bytes=False), "inverted": text.hits(ld, invert=True)}
    assert 100 < kinds["plain"].count < 300
    for what, hits in kinds.items():
        picks = hits.lines().astype(np.int64)
        sel = replace_ref.replace(raw_rows[picks], lens[picks], raws[picks], matches_ref.select(res, picks), table)
        check(td.text_matches(pd, text, hits).text_replace(rp, text, hits), sel, what)
        if what == "inverted":                                              # no match in these lines: the lines themselves
            assert replace_ref.lines_of(*sel) == [with_nl[i] for i in picks]
    # matches of the whole text do not belong to its hits: m differs
    with pytest.raises(OSError) as ei:
        td.text_matches(pd, text).text_replace(rp, text, kinds["plain"])
    assert ei.value.errno == errno.EINVAL
    # the result is a packed text on the device: its matches are the judge's matches of the judge's output
    rd = td.text_matches(pd, text).text_replace(rp, text)
    torch.cuda.synchronize()
    out_lines = replace_ref.lines_of(*want)
    o_rows, o_raws = span_ref.rows_of(out_lines)
    o_lens = o_raws - np.array([x.endswith(b"\n") for x in out_lines], np.int64)
    again = judged("kw_starts", "kw_ends", o_rows, o_lens)
    mt2 = hip.HipMatches.run_device(pd, td, rd.bytes_ptr, rd.off_ptr, rd.count, trim_byte=0x0A, limit=rd.nbytes)
    assert mt2.count == len(lines) and mt2.total == int(again[0][-1])
    got = mt2.copy()
    assert all(np.array_equal(g, w) for g, w in zip(got, again))
    # ... and replacing in it again is the judge's second replacement
    twice = replace_ref.replace(o_rows, o_lens, o_raws, again, table)
    rd2 = mt2.replace_device(rp, rd.bytes_ptr, rd.off_ptr, rd.count, trim_byte=0x0A, limit=rd.nbytes)
    check(rd2, twice, "replaced twice")
    mt2.free()
    rd.free()
    # an empty text
    empty = hip.HipText(b"", 0x0A)
    check(td.text_matches(pd, empty).text_replace(rp, empty), (np.zeros(1, np.uint64), np.zeros(0, np.uint8)), "empty text", m=0)


# ---- group 7: refusals -----------------------------------------------------------------------------------------------------

def test_refusals_with_a_device(hip):
    """EINVAL, and the next call answers"""
    from libfsm_amd import MatchBatch
    rows, lens = inputs_of("kw_ends")
    pd, td = starts_image("kw_starts"), ends_image("kw_ends")
    lib = hip.load_library()
    n = 64
    data, off = lead_packed(rows[:n], lens[:n])
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    table = mixed_table(len(KEYWORDS))
    tb, roff = replace_ref.pack_table(table)
    bad_roff = roff.copy()
    bad_roff[2] = bad_roff[3] + np.uint64(1)
    for args in ((ptr(tb), None, 5, 0), (ptr(tb), ptr(roff), 5, 2), (ptr(tb), ptr(roff), 5, 0x80000000), (ptr(tb), ptr(bad_roff), 5, 0), (None, ptr(roff), 5, 0)):
        C.set_errno(0)
        assert lib.fsm_hip_repl_create(*args) is None and C.get_errno() == errno.EINVAL, args
    rp = hip.HipRepl(table)
    mt = hip.HipMatches.run(pd, td, data, off)
    good = dict(base=ptr(data), off=ptr(off), n=n, trim_byte=-1)
    bad_off = off.copy()
    bad_off[10] = bad_off[11] + np.uint64(1)
    M, R = C.c_void_p(mt.handle), C.c_void_p(rp.handle)
    for change in (dict(off=None), dict(n=n - 1), dict(off=ptr(bad_off)), dict(pick=ptr(np.zeros(3, np.uint64)), m=3)):
        b = MatchBatch(**dict(good, **change))
        C.set_errno(0)
        assert lib.fsm_hip_matches_replace(M, C.byref(b), R) is None and C.get_errno() == errno.EINVAL, change
    b = MatchBatch(**good)
    for args in ((None, C.byref(b), R), (M, None, R), (M, C.byref(b), None)):
        C.set_errno(0)
        assert lib.fsm_hip_matches_replace(*args) is None and C.get_errno() == errno.EINVAL
    d_off = device_u64(off)
    b = MatchBatch(base=None, off=d_off.data_ptr(), n=n, trim_byte=-1, limit=int(off[n]))    # nothing is launched
    C.set_errno(0)
    assert lib.fsm_hip_matches_replace_device(M, C.byref(b), R, None) is None and C.get_errno() == errno.EINVAL
    text = hip.HipText(b"ab\ncd\n", 0x0A)
    tm = td.text_matches(pd, text)
    for args in ((None, text.handle, None, rp.handle, None), (tm.handle, None, None, rp.handle, None), (tm.handle, text.handle, None, None, None),
                 (mt.handle, text.handle, None, rp.handle, None)):        # (the last: 64 inputs against 2 lines)
        C.set_errno(0)
        assert lib.fsm_hip_text_replace(*args) is None and C.get_errno() == errno.EINVAL, args
    want = replace_ref.replace(rows[:n], lens[:n], lens[:n], matches_ref.head(reference("kw_starts", "kw_ends"), n), table)
    check(mt.replace(rp, data, off), want, "the next call answers")
    check(tm.text_replace(rp, text), (np.array([0, 1, 3 + len(table[3])], np.uint64), np.frombuffer(b"\nc" + table[3] + b"\n", np.uint8)), "a text of two lines")


# ---- group 8: the example --------------------------------------------------------------------------------------------------

def test_example_writes_the_judges_text(hip, tmp_path):
    """examples/hipsed.c over two files, the second without a final newline: stdout is the judge's text"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.RandomState(17)
    files = [[bytes(rng.choice(list(b"abcdxyzw" if i % 2 == 0 else b"xyzwba"), rng.randint(0, 25)).astype(np.uint8)) for i in range(k)] for k in (70, 40)]
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

    def run(*args, fs=names):
        r = subprocess.run([exe, *args, "--", *fs], capture_output=True, env=env, timeout=120)
        return r.returncode, r.stdout

    def compose(table, flags=0):
        out = b""
        for j, ls in enumerate(files):
            rows, lens = span_ref.rows_of(ls)
            with_nl = [x + b"\n" for x in ls]
            if j == 1:
                with_nl[-1] = ls[-1]
            raw_rows, raws = span_ref.rows_of(with_nl)
            out += bytes(replace_ref.replace(raw_rows, lens, raws, judged("kw_starts", "kw_ends", rows, lens), table, flags)[1])
        return out

    repl = ["<AB>", "", "c", "a longer replacement", "bdb"]
    table = [x.encode() for x in repl]
    want = compose(table)
    assert want.count(b"\n") == 109 and want.endswith(b"xx<AB>a longer replacement") and b"<AB>" in want and want != compose([])
    assert run(*tables, *repl) == (0, want)
    assert run(*tables, *repl[:2]) == (0, compose(table[:2]))              # rules without a REPL stay
    assert run(*tables) == (0, compose([]))                                # no REPL at all: the files' text
    assert run("-m", *tables, "*", "#@!", "", "xy") == (0, compose([b"*", b"#@!", b"", b"xy"], MASK))
    quiet = tmp_path / "none.txt"
    quiet.write_bytes(b"xyz\nwwww\n\n")
    assert run(*tables, *repl, fs=[str(quiet)]) == (1, b"xyz\nwwww\n\n")   # no line held a match: the text all the same
