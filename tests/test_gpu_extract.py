"""GPU: the extraction (libfsm_amd/csrc/extract.hip: ext_lengths, ext_offsets, ext_write, the fronts and the rule set; the scan
of the block pairs in text.hip).

off, every byte, line and match are compared with tests/extract_ref.py, the definition of include/fsm_hip.h ("extract") restated
in Python, over the matches of tests/matches_ref.py -- never over matches or offsets that came from the device.  The inputs, the
automata and the matches' judge are tests/line_inputs.py's: 1 500 rows of at most 300 bytes with lengths 0, 1, 15, 16, 17, 31, 32,
33, ..., line 8 = 300 times d, and LEAD = 5 bytes in front of the text that belong to no line."""
import ctypes as C
import errno
import os
import subprocess

import numpy as np
import pytest

import extract_ref
import matches_ref
import span_ref
from extract_ref import KEEP_OTHER
from line_inputs import (EMPTY_RULE, FILL, KEYWORDS, LEAD, SIZES, auto_of, device_u64, device_u8, ends_image, inputs_of, judged, lead_packed, reference,
                         starts_image, state_ids)
from matches_ref import DROP_EMPTY

pytestmark = pytest.mark.gpu

NL = 0x0A
SEPS = (-1, NL, 0)
NO_ID = 0xFFFFFFFE


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()   # raises if the HIP extension is missing: no silent fallback
    return libfsm_amd


def rules_of(hip, keep, other=False):
    """the judge's (nrules, ids) or None -> a set on the device, or None"""
    return None if keep is None else hip.HipRules(sorted(keep[1]), keep[0], KEEP_OTHER if other else 0)


def check(ex, want, what):
    """an extracted object against (off, bytes, line, match); the copies are pre-filled and two entries too long: nothing behind
    nbytes or behind R (+ 1) was written"""
    w_off, w_data, w_line, w_match = want
    R, total = len(w_off) - 1, int(w_off[-1])
    assert ex.count == R, (what, "R", ex.count, R)
    assert ex.nbytes == total, (what, "nbytes", ex.nbytes, total)
    assert ex.off_ptr != 0 and (ex.bytes_ptr != 0) == (total != 0) and (ex.line_ptr != 0) == (R != 0) and (ex.match_ptr != 0) == (R != 0), what
    off, data, line, match = ex.copy(extra=2, fill=FILL)
    assert (off[R + 1:] == FILL).all() and (data[total:] == FILL & 0xFF).all() and (line[R:] == FILL).all() and (match[R:] == FILL).all(), what
    bad = np.flatnonzero(off[:R + 1] != w_off)
    assert len(bad) == 0, (what, "off", bad[:5], off[bad[:5]], w_off[bad[:5]])
    bad = np.flatnonzero(data[:total] != w_data)
    assert len(bad) == 0, (what, "bytes", bad[:8], data[bad[:8]], w_data[bad[:8]], "record", np.searchsorted(w_off, bad[:8], "right") - 1)
    assert np.array_equal(line[:R], w_line), (what, "line")
    assert np.array_equal(match[:R], w_match), (what, "match")
    assert ex.ms >= 0.0 and all(ex.pass_ms(k) >= 0.0 for k in range(4))
    ex.free()


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


def device_matches(hip, pd, td, b, mflags=0, trim_byte=-1, limit=None):
    return hip.HipMatches.run_device(pd, td, trim_byte=trim_byte, flags=mflags, **b.device_args(limit))


def device_form(hip, mt, b, keep=None, sep=-1, trim_byte=-1, limit=None):
    """matches_extract_device on the batch the matches were made from"""
    import torch
    ex = mt.extract_device(trim_byte=trim_byte, keep=keep, sep_byte=sep, **b.device_args(limit))
    torch.cuda.synchronize()
    ex._keep = (ex._keep, b)
    return ex


def host_matches(hip, pd, td, b, mflags=0, trim_byte=-1):
    return hip.HipMatches.run(pd, td, b.data, b.off, pick=b.pick, trim_byte=trim_byte, flags=mflags)


def host_form(hip, mt, b, keep=None, sep=-1, trim_byte=-1):
    return mt.extract(b.data, b.off, pick=b.pick, trim_byte=trim_byte, keep=keep, sep_byte=sep)


def kw_sets():
    """(the judge's keep, keep_other) of the keyword pair: no set, each single rule, an empty set, a set with and without
    KEEP_OTHER whose nrules leaves rules 3 and 4 beyond it"""
    sets = [(None, False)] + [((len(KEYWORDS), {i}), False) for i in range(len(KEYWORDS))]
    return sets + [((len(KEYWORDS), set()), False), ((3, {0, 2}), False), ((3, {0, 2}), True), ((0, set()), True)]


# ---- group 1: every size, every separator, every kind of set -----------------------------------------------------------------

def test_every_size_separator_and_set_on_the_keywords(hip):
    starts, ends = "kw_starts", "kw_ends"
    rows, lens = inputs_of(ends)
    pd, td = starts_image(starts), ends_image(ends)
    res = reference(starts, ends)
    sets = kw_sets()
    for n in SIZES:
        b = Batch(*lead_packed(rows[:n], lens[:n]))
        mt_ref = matches_ref.head(res, n)
        mt = device_matches(hip, pd, td, b)
        mh = host_matches(hip, pd, td, b) if n in (1, 257, 1500) else None
        for keep, other in sets:
            for sep in SEPS:
                want = extract_ref.extract(rows[:n], lens[:n], lens[:n], mt_ref, keep, other, sep)
                rs = rules_of(hip, keep, other)
                check(device_form(hip, mt, b, rs, sep), want, (n, keep, other, sep, "device"))
                if mh is not None and (sep == NL or keep is None):
                    check(host_form(hip, mh, b, rs, sep), want, (n, keep, other, sep, "host"))
    R = len(res["start"])
    assert R > 40 * 256 and int(want[0][-1]) > 0


def test_ids_without_a_rule_on_the_random_automata(hip):
    """glob_first as `ends` gives every match an id; s15_start as `ends` -- its start state an end state too, its end states
    without ids -- gives NO_ID alone, empty matches among them: a set keeps those only with KEEP_OTHER"""
    for starts, ends in (("s15_start", "glob_first"), ("glob_first", "s15_start")):
        rows, lens = inputs_of(ends)
        pd, td = starts_image(starts), ends_image(ends)
        res = reference(starts, ends)
        ids = res["id"]
        if ends == "s15_start":
            assert len(ids) >= 1000 and (ids == NO_ID).all() and (res["end"] == res["start"]).sum() >= 100
            top, some = 5, {0, 1, 2, 3, 4}
        else:
            assert len(ids) >= 1000 and (ids < NO_ID).all()
            top = int(np.median(ids)) + 1
            some = set(np.unique(ids[ids < top]).tolist()[::2])
            assert 0 < (ids >= top).sum() < len(ids) and some
        for n in (65, 257, 1500):
            b = Batch(*lead_packed(rows[:n], lens[:n]))
            mt_ref = matches_ref.head(res, n)
            mt = device_matches(hip, pd, td, b)
            for keep, other in ((None, False), ((top, some), False), ((top, some), True), ((top, set()), True), ((0, set()), False)):
                for sep in SEPS:
                    want = extract_ref.extract(rows[:n], lens[:n], lens[:n], mt_ref, keep, other, sep)
                    check(device_form(hip, mt, b, rules_of(hip, keep, other), sep), want, (ends, n, keep and keep[0], other, sep))
            if n == 257:
                check(host_form(hip, host_matches(hip, pd, td, b), b, rules_of(hip, (top, some), True), NL),
                      extract_ref.extract(rows[:n], lens[:n], lens[:n], mt_ref, (top, some), True, NL), (ends, "host"))
        kept_other = extract_ref.extract(rows, lens, lens, matches_ref.head(res, 1500), (top, set()), True, -1)
        assert len(kept_other[2]) == int((ids >= top).sum()) > 0
        without = extract_ref.extract(rows, lens, lens, matches_ref.head(res, 1500), (top, some), False, -1)
        assert (len(without[2]) == 0) == (ends == "s15_start")


def test_kept_records_around_a_block_of_matches(hip):
    """R = 0, 1, 255, 256, 257, 511, 512, 513 kept records (fsm_hip_extracted_block_matches() = 256) out of about three times as many
    matches: lines with one d, one ab or no word, of which the set keeps the d alone; the same without the lines of ab -- fewer
    inputs -- with every match kept"""
    B = hip.extracted_block_matches()
    assert B == 256
    pd, td = starts_image("kw_starts"), ends_image("kw_ends")
    rng = np.random.RandomState(5)
    for R in (0, 1, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1):
        lines = [b"ab", b"xx", b""] * 3
        for _ in range(R):
            lines += [b"x" * rng.randint(0, 20) + b"d" + b"y" * rng.randint(0, 3)] + [[b"ab", b"cab"], [b""], [b"xabx", b"y"]][rng.randint(0, 3)]
        rows, lens = span_ref.rows_of(lines)
        mt_ref = judged("kw_starts", "kw_ends", rows, lens)
        b = Batch(*lead_packed(rows, lens))
        mt = device_matches(hip, pd, td, b)
        for sep in SEPS:
            want = extract_ref.extract(rows, lens, lens, mt_ref, (len(KEYWORDS), {3}), False, sep)
            assert len(want[2]) == R and len(mt_ref[1]) >= R + 3
            assert bytes(want[1]) == (b"d" + bytes([sep]) if sep >= 0 else b"d") * R
            check(device_form(hip, mt, b, rules_of(hip, (len(KEYWORDS), {3})), sep), want, ("set", R, sep))
        # ... and by m: the same lines without those of ab hold exactly R matches, every one kept
        lines = [x for x in lines if b"ab" not in x]
        rows, lens = span_ref.rows_of(lines)
        mt_ref = judged("kw_starts", "kw_ends", rows, lens)
        assert len(mt_ref[1]) == R
        b = Batch(*lead_packed(rows, lens))
        want = extract_ref.extract(rows, lens, lens, mt_ref, None, False, NL)
        check(device_form(hip, device_matches(hip, pd, td, b), b, None, NL), want, ("m", R))


# ---- group 2: picks, trim, limit ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("starts,ends", [("s15_start", "glob_first"), ("kw_starts", "kw_ends")])
def test_pick_and_limit(hip, starts, ends):
    rows, lens = inputs_of(ends)
    pd, td = starts_image(starts), ends_image(ends)
    n = 700
    data, off = lead_packed(rows[:n], lens[:n])
    rng = np.random.RandomState(12)
    pick = np.concatenate([rng.permutation(n)[:300], [7, 7, 7, 0, n - 1, n - 1, 8, 8], rng.randint(0, n, 100), np.arange(n)[::-1][:50]]).astype(np.uint64)
    res = reference(starts, ends)
    keep = (len(KEYWORDS), {0, 3}) if ends == "kw_ends" else (int(np.median(res["id"][res["id"] < NO_ID])) + 1, set(range(0, 4000, 3)))
    keep = (keep[0], {i for i in keep[1] if i < keep[0]})

    def want_of(p, k, other, sep, nlines=n):
        ok = p < nlines
        at = np.where(ok, p, 0).astype(np.int64)
        ln = np.where(ok, lens[at], 0)
        return extract_ref.extract(rows[at], ln, ln, matches_ref.select(res, p, nlines), k, other, sep)

    for p in (pick, np.arange(n)[::-1].astype(np.uint64), np.repeat(np.uint64(8), 40)):
        b = Batch(data, off, p)
        mt, mh = device_matches(hip, pd, td, b), host_matches(hip, pd, td, b)
        for k, other, sep in ((None, False, NL), (keep, False, -1), (keep, True, 0)):
            check(device_form(hip, mt, b, rules_of(hip, k, other), sep), want_of(p, k, other, sep), (starts, ends, len(p), sep, "device"))
            check(host_form(hip, mh, b, rules_of(hip, k, other), sep), want_of(p, k, other, sep), (starts, ends, len(p), sep, "host"))
    # an empty pick: a valid object, nothing launched that stores
    none = (np.zeros(1, np.uint64), np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    b = Batch(data, off, np.zeros(0, np.uint64))
    check(device_form(hip, device_matches(hip, pd, td, b), b, None, NL), none, "m == 0 device")
    check(host_form(hip, host_matches(hip, pd, td, b), b, None, NL), none, "m == 0 host")
    # an index at or beyond n: no match and no record on the device form, its neighbours right; EINVAL on the host form
    wild = pick.copy()
    at = [0, 5, 255, 256, len(wild) - 1]
    wild[at] = [n, n + 1, 2 ** 40, 0xFFFFFFFFFFFFFFFF, n]
    b = Batch(data, off, wild)
    mt = device_matches(hip, pd, td, b)
    for sep in (-1, NL):
        want = want_of(wild, None, False, sep)
        assert not set(want[2].tolist()) & set(at)
        check(device_form(hip, mt, b, None, sep), want, (starts, ends, "wild", sep))
    good = host_matches(hip, pd, td, Batch(data, off, pick))
    with pytest.raises(OSError) as ei:
        good.extract(data, off, pick=wild)
    assert ei.value.errno == errno.EINVAL
    # a limit that cuts the last line (and the lines behind it): the judge on the clipped text; limit = 0 is off[n]
    n2 = 257
    data, off = lead_packed(rows[:n2], lens[:n2])
    b = Batch(data, off)
    mt = device_matches(hip, pd, td, b, limit=0)
    check(device_form(hip, mt, b, None, NL, limit=0), extract_ref.extract(rows[:n2], lens[:n2], lens[:n2], matches_ref.head(res, n2), None, False, NL), "limit = 0")
    for cut in (int(off[n2]) - 3, int(off[200]) + 7):
        clipped = np.clip(cut - off[:n2].astype(np.int64), 0, lens[:n2])
        assert (clipped != lens[:n2]).sum() >= 1
        mt = device_matches(hip, pd, td, b, limit=cut)
        for sep in (-1, NL):
            want = extract_ref.extract(rows[:n2], clipped, clipped, judged(starts, ends, rows[:n2], clipped), None, False, sep)
            check(device_form(hip, mt, b, None, sep, limit=cut), want, ("limit", cut, sep))


def test_trim_byte_set_and_unset(hip):
    rows, lens = inputs_of("kw_ends")
    pd, td = starts_image("kw_starts"), ends_image("kw_ends")
    n, trim = 600, ord("d")                                                # lines that end in d lose it for the matches
    rows, lens = rows[:n], lens[:n]
    idx = np.arange(n)
    ends_in = (lens > 0) & (rows[idx, np.maximum(lens - 1, 0)] == trim)
    shorter = lens - ends_in
    assert ends_in.sum() > 30 and (~ends_in & (lens > 0)).sum() > 100
    b = Batch(*lead_packed(rows, lens))
    trimmed, plain = judged("kw_starts", "kw_ends", rows, shorter), matches_ref.head(reference("kw_starts", "kw_ends"), n)
    assert len(trimmed[1]) < len(plain[1])
    for sep in (-1, NL):
        want = extract_ref.extract(rows, shorter, lens, trimmed, (len(KEYWORDS), {0, 3, 4}), False, sep)
        check(device_form(hip, device_matches(hip, pd, td, b, trim_byte=trim), b, rules_of(hip, (len(KEYWORDS), {0, 3, 4})), sep, trim_byte=trim), want,
              ("trim, device", sep))
        check(host_form(hip, host_matches(hip, pd, td, b, trim_byte=trim), b, rules_of(hip, (len(KEYWORDS), {0, 3, 4})), sep, trim_byte=trim), want,
              ("trim, host", sep))
        want = extract_ref.extract(rows, lens, lens, plain, (len(KEYWORDS), {0, 3, 4}), False, sep)
        check(device_form(hip, device_matches(hip, pd, td, b), b, rules_of(hip, (len(KEYWORDS), {0, 3, 4})), sep), want, ("no trim", sep))


# ---- group 3: one long record, runs of empty records -------------------------------------------------------------------------

def d_tables(L):
    """(M, E, Q) of matches_ref for one line of L times d under d_starts / d_plus: every s < L is marked and ends at L in state 1"""
    M = np.ones((1, L + 1), bool)
    M[0, L] = False
    E = np.full((1, L + 1), L, np.int64)
    E[0, L] = -1
    Q = np.ones((1, L + 1), np.int64)
    Q[0, L] = -1
    return M, E, Q


def test_one_record_across_the_blocks_of_the_write_pass(hip):
    """one line of L times d under d+ as the only input: one record of L bytes -- the fast path, the last chunk, several blocks"""
    BB = hip.extracted_block_bytes()
    assert BB == 16384
    pd, td = starts_image("d_starts"), ends_image("d_plus")
    # the tables of the long lines are the judge's own at a length it walks in full
    rows, lens = span_ref.rows_of([b"d" * 33])
    M, E, Q = matches_ref.marks(auto_of("d_starts")[0], rows, lens), *matches_ref.longest_from(auto_of("d_plus")[0], rows, lens)
    assert all(np.array_equal(a, b) for a, b in zip((M, E, Q), d_tables(33)))
    for L in (15, 16, 17, BB - 1, BB, BB + 1, 50000):
        rows = np.full((1, L), ord("d"), np.uint8)
        lens = np.array([L], np.int64)
        res = matches_ref.matches(auto_of("d_starts")[0], auto_of("d_plus")[0], rows, lens, ids=state_ids("d_plus"), tables=d_tables(L))
        mt_ref = (res["off"], res["start"], res["end"], res["id"])
        assert mt_ref[1].tolist() == [0] and mt_ref[2].tolist() == [L] and mt_ref[3].tolist() == [0]
        for lead in (LEAD, 16):
            b = Batch(*lead_packed(rows, lens, lead))
            mt = device_matches(hip, pd, td, b)
            for sep in (-1, NL):
                want = extract_ref.extract(rows, lens, lens, mt_ref, None, False, sep)
                assert int(want[0][-1]) == L + (sep >= 0)
                check(device_form(hip, mt, b, None, sep), want, (L, lead, sep))
    # the same record out of a line whose bytes differ: a window that is placed wrongly shows.  The match arrays are the caller's
    # word, so a matches object of the d line serves a text of other bytes with the same offsets
    L = BB + 1
    rows = (np.arange(L, dtype=np.int64) * 7 % 251).astype(np.uint8)[None, :]
    lens = np.array([L], np.int64)
    b_d = Batch(*lead_packed(np.full((1, L), ord("d"), np.uint8), lens, 3))
    b_x = Batch(*lead_packed(rows, lens, 3))
    mt = device_matches(hip, pd, td, b_d)
    mt_ref = (np.array([0, 1], np.uint64), np.array([0], np.uint64), np.array([L], np.uint64), np.array([0], np.uint32))
    for sep in (-1, 0):
        check(device_form(hip, mt, b_x, None, sep), extract_ref.extract(rows, lens, lens, mt_ref, None, False, sep), ("other bytes", sep))


@pytest.mark.parametrize("run", [300, 70000])
def test_runs_of_empty_records_with_one_byte_in_the_middle(hip, run):
    """empty matches kept and no separator: `run` records without bytes in a row, one record of one byte in their middle.  The
    runs cross blocks of the offsets pass; with the tail of long records behind them also a 16 KiB boundary's first[]"""
    starts, ends = "kw_starts_everywhere", "kw_ends_empty_ids"
    pd, td = starts_image(starts), ends_image(ends)
    # lines of x alone: an empty match at every position; 9 x a line -> 10 empty matches
    per = 10
    nlines = run // per
    # 4 empty, d, 3 empty + the one at len: 9 matches, one with a byte; then 36 000 bytes of short records and another run
    uniq = [b"x" * (per - 1), b"xxxxdxxx", b"ab" * 20, b"abc" * 100, b"", b"x", b"bdb" * 100]
    order = [1 if i == nlines // 2 else 0 for i in range(nlines)] + [2] + [3] * 120 + [4, 5] + [6] * 30 + [0] * 20
    # the judge's matches, line by line where lines repeat: the same line has the same matches
    one = judged(starts, ends, *span_ref.rows_of(uniq))
    o = one[0].astype(np.int64)
    moff = np.r_[0, np.cumsum([o[i + 1] - o[i] for i in order])].astype(np.uint64)
    mt_ref = (moff,) + tuple(np.concatenate([a[o[i]:o[i + 1]] for i in order]) for a in one[1:])
    rows, lens = span_ref.rows_of([uniq[i] for i in order])
    b = Batch(*lead_packed(rows, lens))
    mt = device_matches(hip, pd, td, b)
    got = mt.copy()
    assert all(np.array_equal(g, w) for g, w in zip(got, mt_ref))          # (the device's matches are the judge's: not what is tested here)
    want = extract_ref.extract(rows, lens, lens, mt_ref)
    size = np.diff(want[0].astype(np.int64))
    first_byte = int(np.flatnonzero(size)[0])
    assert first_byte >= run // 2 - per and (size[:first_byte] == 0).all() and size[first_byte] == 1 and bytes(want[1][:1]) == b"d"
    assert (size[first_byte + 1:first_byte + run // 2 - per] == 0).all() and int(want[0][-1]) > 2 * 16384
    check(device_form(hip, mt, b), want, ("empty records", run))
    # the empty rule alone: records without any byte at all -- R > 0, no bytes, nothing written
    want = extract_ref.extract(rows, lens, lens, mt_ref, (EMPTY_RULE + 1, {EMPTY_RULE}))
    assert len(want[2]) >= run and int(want[0][-1]) == 0
    check(device_form(hip, mt, b, rules_of(hip, (EMPTY_RULE + 1, {EMPTY_RULE}))), want, ("no bytes at all", run))
    if run == 300:                                                         # with a separator every record has its byte
        check(device_form(hip, mt, b, None, NL), extract_ref.extract(rows, lens, lens, mt_ref, None, False, NL), "separator")


def test_matches_made_with_and_without_drop_empty(hip):
    starts, ends = "kw_starts_everywhere", "kw_ends_empty_ids"
    rows, lens = inputs_of(ends)
    pd, td = starts_image(starts), ends_image(ends)
    kept, dropped = reference(starts, ends), reference(starts, ends, DROP_EMPTY)
    empty = kept["end"] == kept["start"]
    assert empty.sum() >= 1000 and len(dropped["start"]) == int((~empty).sum())
    for n in (65, 1500):
        b = Batch(*lead_packed(rows[:n], lens[:n]))
        for res, mflags in ((kept, 0), (dropped, DROP_EMPTY)):
            mt = device_matches(hip, pd, td, b, mflags)
            for keep, other, sep in ((None, False, -1), (None, False, NL), ((EMPTY_RULE, {0, 1, 2, 3, 4}), False, -1), ((EMPTY_RULE, set()), True, 0)):
                want = extract_ref.extract(rows[:n], lens[:n], lens[:n], matches_ref.head(res, n), keep, other, sep)
                check(device_form(hip, mt, b, rules_of(hip, keep, other), sep), want, (n, mflags, keep, other, sep))
    # without the empty ones and without a separator the two are the same bytes
    a = extract_ref.extract(rows, lens, lens, matches_ref.head(kept, 1500))
    d = extract_ref.extract(rows, lens, lens, matches_ref.head(dropped, 1500))
    assert bytes(a[1]) == bytes(d[1]) and len(a[2]) == len(d[2]) + int(empty.sum())


# ---- group 4: the text front, and the result as a text -------------------------------------------------------------------------

def text_lines(rng):
    """400 lines of 0-60 bytes over abcdx and, every third, over xyzw: a third without any word; the last without a newline"""
    out = []
    for i in range(400):
        alpha = b"abcdx" if i % 3 else b"xyzw"
        out.append(bytes(rng.choice(list(alpha), rng.randint(0, 61)).astype(np.uint8)))
    out[-1] = b"xxabcabd"
    return out


def test_text_extract_over_a_text_and_its_hits_and_the_result_fed_back(hip):
    import torch
    pd, td = starts_image("kw_starts"), ends_image("kw_ends")
    lines = text_lines(np.random.RandomState(18))
    blob = b"".join(x + b"\n" for x in lines)[:-1]
    text = hip.HipText(blob, NL)
    assert text.lines == len(lines)
    rows, lens = span_ref.rows_of(lines)
    with_nl = [x + b"\n" for x in lines[:-1]] + [lines[-1]]
    raw_rows, raws = span_ref.rows_of(with_nl)
    mt_ref = judged("kw_starts", "kw_ends", rows, lens)
    res = dict(off=mt_ref[0], start=mt_ref[1], end=mt_ref[2], id=mt_ref[3])
    keep = (len(KEYWORDS), {1, 2, 3})
    rs = rules_of(hip, keep)
    for k, r, sep in ((None, None, NL), (keep, rs, NL), (keep, rs, -1)):
        want = extract_ref.extract(raw_rows, lens, raws, mt_ref, k, False, sep)
        check(td.text_matches(pd, text).text_extract(text, keep=r, sep_byte=sep), want, ("text", k, sep))
    # ... is the primitive over the text's own offsets with the delimiter trimmed, host and device form alike
    off = np.zeros(len(lines) + 1, np.uint64)
    off[1:] = np.cumsum(raws)
    b = Batch(np.frombuffer(blob, np.uint8), off)
    want = extract_ref.extract(raw_rows, lens, raws, mt_ref, keep, False, NL)
    check(host_form(hip, host_matches(hip, pd, td, b, trim_byte=NL), b, rs, NL, trim_byte=NL), want, "primitive, host")
    check(device_form(hip, device_matches(hip, pd, td, b, trim_byte=NL), b, rs, NL, trim_byte=NL), want, "primitive, device")
    ld = hip.LinesDfa(span_ref.line_matcher_of(KEYWORDS)[0], NL)
    kinds = {"plain": text.hits(ld), "no bytes": text.hits(ld, want_bytes=False), "inverted": text.hits(ld, invert=True)}
    assert 100 < kinds["plain"].count < 300
    for what, hits in kinds.items():
        picks = hits.lines().astype(np.int64)
        sel = extract_ref.extract(raw_rows[picks], lens[picks], raws[picks], matches_ref.select(res, picks), keep, False, NL)
        check(td.text_matches(pd, text, hits).text_extract(text, hits, keep=rs, sep_byte=NL), sel, what)
        if what == "inverted":                                              # no match in these lines: no record
            assert len(sel[2]) == 0
    # matches of the whole text do not belong to its hits: m differs
    with pytest.raises(OSError) as ei:
        td.text_matches(pd, text).text_extract(text, kinds["plain"])
    assert ei.value.errno == errno.EINVAL
    # the point of the feature: the result is a packed text on the device, its separator the trimmed byte of a second walk.  Its
    # matches under the same pair are the judge's matches of the judge's extracted text
    for k, r in ((None, None), (keep, rs)):
        ex = td.text_matches(pd, text).text_extract(text, keep=r, sep_byte=NL)
        torch.cuda.synchronize()
        want = extract_ref.extract(raw_rows, lens, raws, mt_ref, k, False, NL)
        recs = extract_ref.records_of(want[0], want[1])
        assert all(x.endswith(b"\n") for x in recs) and len(recs) > 500
        o_rows, o_raws = span_ref.rows_of(recs)
        again = judged("kw_starts", "kw_ends", o_rows, o_raws - 1)
        mt2 = hip.HipMatches.run_device(pd, td, ex.bytes_ptr, ex.off_ptr, ex.count, trim_byte=NL, limit=ex.nbytes)
        assert mt2.count == len(recs) and mt2.total == int(again[0][-1]) >= len(recs)
        assert all(np.array_equal(g, w) for g, w in zip(mt2.copy(), again))
        # ... and extracting from it again is the judge's second extraction
        ex2 = mt2.extract_device(ex.bytes_ptr, ex.off_ptr, ex.count, trim_byte=NL, limit=ex.nbytes, sep_byte=0)
        check(ex2, extract_ref.extract(o_rows, o_raws - 1, o_raws, again, None, False, 0), "extracted twice")
        mt2.free()
        ex.free()
    # an empty text
    empty = hip.HipText(b"", NL)
    check(td.text_matches(pd, empty).text_extract(empty, sep_byte=NL),
          (np.zeros(1, np.uint64), np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint64)), "empty text")


# ---- group 5: refusals -------------------------------------------------------------------------------------------------------

def test_refusals_with_a_device(hip):
    """EINVAL before any launch, and the next call answers"""
    from libfsm_amd import MatchBatch
    rows, lens = inputs_of("kw_ends")
    pd, td = starts_image("kw_starts"), ends_image("kw_ends")
    lib = hip.load_library()
    n = 64
    data, off = lead_packed(rows[:n], lens[:n])
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    bits = extract_ref.pack_rules({0, 3}, len(KEYWORDS))
    for args in ((None, 5, 0), (ptr(bits), 5, 2), (ptr(bits), 5, 0x80000000)):
        C.set_errno(0)
        assert lib.fsm_hip_rules_create(*args) is None and C.get_errno() == errno.EINVAL, args
    rs = hip.HipRules([0, 3], len(KEYWORDS))
    none = hip.HipRules([], 0)                                              # nrules == 0 is valid
    mt = hip.HipMatches.run(pd, td, data, off)
    good = dict(base=ptr(data), off=ptr(off), n=n, trim_byte=-1)
    bad_off = off.copy()
    bad_off[10] = bad_off[11] + np.uint64(1)
    M, R = C.c_void_p(mt.handle), C.c_void_p(rs.handle)
    for change in (dict(off=None), dict(n=n - 1), dict(off=ptr(bad_off)), dict(pick=ptr(np.zeros(3, np.uint64)), m=3), dict(trim_byte=256)):
        b = MatchBatch(**dict(good, **change))
        C.set_errno(0)
        assert lib.fsm_hip_matches_extract(M, C.byref(b), R, NL) is None and C.get_errno() == errno.EINVAL, change
    b = MatchBatch(**good)
    for args in ((None, C.byref(b), R, NL), (M, None, R, NL), (M, C.byref(b), R, -2), (M, C.byref(b), R, 256), (M, C.byref(b), None, 1 << 20)):
        C.set_errno(0)
        assert lib.fsm_hip_matches_extract(*args) is None and C.get_errno() == errno.EINVAL
    d_off = device_u64(off)
    d_data = device_u8(data)
    db = dict(base=d_data.data_ptr(), off=d_off.data_ptr(), n=n, trim_byte=-1, limit=int(off[n]))
    for change, sep in ((dict(base=None), NL), (dict(n=n + 1), NL), ({}, -2), ({}, 256)):      # nothing is launched
        b = MatchBatch(**dict(db, **change))
        C.set_errno(0)
        assert lib.fsm_hip_matches_extract_device(M, C.byref(b), R, sep, None) is None and C.get_errno() == errno.EINVAL, (change, sep)
    C.set_errno(0)
    assert lib.fsm_hip_matches_extract_device(None, C.byref(MatchBatch(**db)), R, NL, None) is None and C.get_errno() == errno.EINVAL
    text = hip.HipText(b"ab\ncd\n", NL)
    tm = td.text_matches(pd, text)
    for args in ((None, text.handle, None, rs.handle, NL, None), (tm.handle, None, None, rs.handle, NL, None), (tm.handle, text.handle, None, None, 256, None),
                 (tm.handle, text.handle, None, None, -2, None), (mt.handle, text.handle, None, rs.handle, NL, None)):   # (the last: 64 inputs against 2 lines)
        C.set_errno(0)
        assert lib.fsm_hip_text_extract(*args) is None and C.get_errno() == errno.EINVAL, args
    mt_ref = matches_ref.head(reference("kw_starts", "kw_ends"), n)
    want = extract_ref.extract(rows[:n], lens[:n], lens[:n], mt_ref, (len(KEYWORDS), {0, 3}), False, NL)
    check(mt.extract(data, off, keep=rs, sep_byte=NL), want, "the next call answers")
    check(mt.extract(data, off, keep=none, sep_byte=NL), extract_ref.extract(rows[:n], lens[:n], lens[:n], mt_ref, (0, set()), False, NL), "an empty set")
    got = tm.text_extract(text, keep=None, sep_byte=NL)
    check(got, (np.array([0, 3, 5], np.uint64), np.frombuffer(b"ab\nd\n", np.uint8), np.array([0, 1], np.uint64), np.array([0, 1], np.uint64)), "a text of two lines")


# ---- group 6: the example ----------------------------------------------------------------------------------------------------

def test_example_prints_what_grep_o_prints(hip, tmp_path):
    """examples/hipextract.c over three files, the last without a final newline: stdout is the judge's text, with -H -n -b
    prefixes and with -r"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.RandomState(17)
    files = [[bytes(rng.choice(list(b"abcdxyzw" if i % 2 == 0 else b"xyzwba"), rng.randint(0, 25)).astype(np.uint8)) for i in range(k)] for k in (70, 40, 25)]
    files[2][-1] = b"xxabcabd"
    tables = []
    for nm, auto in (("lines", span_ref.line_matcher_of(KEYWORDS)), ("starts", auto_of("kw_starts")[0]), ("ends", auto_of("kw_ends")[0])):
        tables.append(str(tmp_path / (nm + ".fsmhip")))
        auto[0].write_c(tables[-1])
    names = []
    for j, ls in enumerate(files):
        data = b"".join(x + b"\n" for x in ls)
        p = tmp_path / ("f%d.txt" % j)
        p.write_bytes(data[:-1] if j == 2 else data)
        names.append(str(p))
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    exe = str(tmp_path / "hipextract")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "hipextract.c"),
                           "-o", exe, "-L" + os.path.join(root, "libfsm_amd"), "-lfsm_hip", "-Wl,-rpath," + os.path.join(root, "libfsm_amd")])

    def run(*args, fs=names):
        r = subprocess.run([exe, *args, *tables, *fs], capture_output=True, env=env, timeout=120)
        return r.returncode, r.stdout

    def compose(keep=None, name=False, number=False, offset=False, fs=(0, 1, 2)):
        out = b""
        for j in fs:
            ls = files[j]
            rows, lens = span_ref.rows_of(ls)
            mt = judged("kw_starts", "kw_ends", rows, lens, DROP_EMPTY)
            off, data, line, match = extract_ref.extract(rows, lens, lens, mt, keep, False, NL)
            starts_at = np.r_[0, np.cumsum(lens + 1)]                       # the line's first byte in its file
            for r, rec in enumerate(extract_ref.records_of(off, data)):
                i = int(line[r])
                pre = (names[j].encode() + b":" if name else b"") + (b"%d:" % (i + 1) if number else b"") + \
                      (b"%d:" % (int(starts_at[i]) + int(mt[1][int(match[r])])) if offset else b"")
                out += pre + rec
        return out

    want = compose()
    assert want.count(b"\n") > 100 and want.endswith(b"abc\nab\nd\n") and {b"ab", b"abc", b"ca", b"d", b""} <= set(want.split(b"\n")) <= set(KEYWORDS) | {b""}
    assert run() == (0, want)
    assert run("-H", "-n", "-b") == (0, compose(None, True, True, True))
    assert run("-n") == (0, compose(None, number=True))
    assert run("-b", "-H") == (0, compose(None, name=True, offset=True))
    only = compose((4, {1, 3}))
    assert set(only.split(b"\n")) == {b"abc", b"d", b""}
    assert run("-r", "1,3") == (0, only)
    assert run("-r", "3,1", "-n", "-H") == (0, compose((4, {1, 3}), name=True, number=True))
    assert run("-r", "7") == (1, b"")                                      # no match of such a rule: nothing, status 1
    quiet = tmp_path / "none.txt"
    quiet.write_bytes(b"xyz\nwwww\n\n")
    assert run(fs=[str(quiet)]) == (1, b"")
    assert run("-H", fs=[names[2], str(quiet), names[0]]) == (0, compose(None, name=True, fs=(2,)) + compose(None, name=True, fs=(0,)))
