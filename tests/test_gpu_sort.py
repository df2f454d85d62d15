"""GPU: the sort of a packed text (libfsm_amd/csrc/sort.hip: srt_init, srt_major, srt_prefix, srt_fetch, srt_digits, srt_tile_hist,
srt_hist_scan, srt_scatter, srt_mark, srt_blocks_scan, srt_assign, srt_ranks, srt_finish and the fronts; the scan of the block
pairs in text.hip, the write pass in extract.hip).

order, rank, groups, soff and every byte of the sorted text are compared with tests/sort_ref.py, the definition of
include/fsm_hip.h ("sort") restated as Python's sorted() over the trimmed keys -- nothing that came from the device is ever used to
judge the device.  The caller's arrays on the device are longer than needed and pre-filled: they and what lies behind them are
unchanged afterwards; the copies out are two entries too long and pre-filled: nothing behind R or the bytes is written."""
import errno
import functools
import os
import subprocess

import numpy as np
import pytest

import distinct_ref
import extract_ref
import matches_ref
import sort_ref
import span_ref
from distinct_ref import pack
from line_inputs import FILL, KEYWORDS, device_u64, device_u8, ends_image, inputs_of, judged, lead_packed, reference, starts_image
from sort_ref import MAJOR_DESC, NO_TEXT, REVERSE

pytestmark = pytest.mark.gpu

NL = 0x0A
GUARD = 64                                   # bytes behind the text that belong to no record


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()   # raises if the HIP extension is missing: no silent fallback
    return libfsm_amd


class Packed:
    """a packed text (and its major keys) on the device: `shift` bytes in front of the first byte, GUARD bytes and two entries of
    FILL behind every array; exact: the bytes' allocation ends with the text"""

    def __init__(self, off, data, major=None, shift=0, exact=False):
        self.off, self.data = np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(data, np.uint8)
        self.major = None if major is None else np.ascontiguousarray(major, np.uint64)
        self.R, self.shift = len(self.off) - 1, shift
        self.h_data = np.concatenate([np.full(shift, 0xEE, np.uint8), self.data, np.full(0 if exact else GUARD, FILL & 0xFF, np.uint8)])
        self.h_off = np.concatenate([self.off, np.full(2, FILL, np.uint64)])
        self.h_major = None if major is None else np.concatenate([self.major, np.full(2, FILL, np.uint64)])
        self.d_data = device_u8(self.h_data if len(self.h_data) else np.zeros(1, np.uint8))
        self.d_off = device_u64(self.h_off)
        self.d_major = None if major is None else device_u64(self.h_major)
        assert shift == 0 or self.d_data.data_ptr() % 256 == 0

    def run(self, hip, trim=-1, sep=-1, flags=0, nbytes=None):
        import torch
        sx = hip.sort_device(self.d_off.data_ptr(), self.d_data.data_ptr() + self.shift, self.R, len(self.data) if nbytes is None else nbytes, trim,
                             self.d_major.data_ptr() if self.d_major is not None else 0, sep, flags, keep=(self,))
        torch.cuda.synchronize()
        return sx

    def unchanged(self):
        assert np.array_equal(self.d_off.cpu().numpy().view(np.uint64), self.h_off)
        assert len(self.h_data) == 0 or np.array_equal(self.d_data.cpu().numpy(), self.h_data)
        assert self.d_major is None or np.array_equal(self.d_major.cpu().numpy().view(np.uint64), self.h_major)


def check(sx, want, what, text=True, free=True):
    """a sorted object against the judge's (order, rank, groups, soff, sbytes), in full, and the properties on their own"""
    w_order, w_rank, w_groups, w_soff, w_data = want
    R, total = len(w_order), int(w_soff[-1]) if text else 0
    assert (sx.records, sx.nbytes) == (R, total), (what, "R, nbytes", sx.records, sx.nbytes, R, total)
    assert (sx.order_ptr != 0) == (R != 0) and (sx.rank_ptr != 0) == (R != 0), what
    assert (sx.off_ptr != 0) == text and (sx.bytes_ptr != 0) == (total != 0), what
    order, rank, soff, data = sx.copy(extra=2, fill=FILL)
    assert (order[R:] == FILL).all() and (rank[R:] == FILL & 0xFFFFFFFF).all(), what
    # the properties on their own: a permutation; ranks from 0, monotone, in steps of 0 or 1
    assert np.array_equal(np.sort(order[:R]), np.arange(R, dtype=np.uint64)), (what, "order is no permutation")
    steps = np.diff(rank[:R].astype(np.int64))
    assert R == 0 or (rank[0] == 0 and ((steps == 0) | (steps == 1)).all()), (what, "rank")
    for name, got, w in (("order", order[:R], w_order), ("rank", rank[:R], w_rank)):
        bad = np.flatnonzero(got != w)
        assert len(bad) == 0, (what, name, bad[:5], got[bad[:5]], w[bad[:5]])
    assert sx.groups == w_groups == (int(rank[R - 1]) + 1 if R else 0), (what, "groups", sx.groups, w_groups)
    if text:
        assert (soff[R + 1:] == FILL).all() and (data[total:] == FILL & 0xFF).all(), what
        bad = np.flatnonzero(soff[:R + 1] != w_soff)
        assert len(bad) == 0, (what, "soff", bad[:5], soff[bad[:5]], w_soff[bad[:5]])
        bad = np.flatnonzero(data[:total] != w_data)
        assert len(bad) == 0, (what, "bytes", bad[:8], data[bad[:8]], w_data[bad[:8]], "record", np.searchsorted(w_soff, bad[:8], "right") - 1)
    else:
        assert soff is None and data is None
    assert sx.ms >= 0.0 and all(sx.pass_ms(k) >= 0.0 for k in range(4))
    rounds = sx.rounds
    if free:
        sx.free()
    return order[:R], rank[:R], None if soff is None else soff[:R + 1], None if data is None else data[:total], rounds


def both(hip, records, what, trim=NL, major=None, flags=0, seps=(NL, -1), shift=0, exact=False, no_text=False):
    """the records through the device form, with every separator (and without the text), against the judge; -> (the judge's
    last answer, the rounds of the last run)"""
    off, data = pack(records)
    p = Packed(off, data, major, shift, exact)
    for sep in seps:
        want = sort_ref.sort(off, data, trim, major, sep, flags)
        rounds = check(p.run(hip, trim, sep, flags), want, (what, sep, flags))[4]
    if no_text:
        check(p.run(hip, trim, NL, flags | NO_TEXT), want, (what, "no text", flags), text=False)
    p.unchanged()
    return want, rounds


def letters(rng, n, lo, hi, alphabet=b"ab"):
    return [bytes(rng.choice(list(alphabet), rng.randint(lo, hi + 1)).astype(np.uint8)) for _ in range(n)]


# ---- sizes and shapes ----------------------------------------------------------------------------------------------------------

def test_no_record_one_and_two(hip):
    want, rounds = both(hip, [], "R = 0", no_text=True)
    assert len(want[0]) == 0 and want[3].tolist() == [0] and rounds == 0
    p = Packed([7], np.zeros(0, np.uint8))                # off[0] alone, and not 0: nothing is read
    check(p.run(hip, NL, NL, NO_TEXT), sort_ref.sort([7], b"", NL, None, NL), "R = 0, no text", text=False)
    for rec in (b"", b"\n", b"x", b"x\n", b"0123456789abcdefg"):
        want, rounds = both(hip, [rec], ("R = 1", rec), no_text=True)
        assert want[0].tolist() == [0] and want[2] == 1 and rounds == 0
    for pair in ((b"b", b"a"), (b"a", b"b"), (b"a\n", b"a"), (b"", b"\n"), (b"ab", b"a")):
        both(hip, list(pair), ("R = 2", pair), no_text=True)


@pytest.mark.parametrize("where", ("256", "tile"))
def test_around_a_block_and_a_tile(hip, where):
    rng = np.random.RandomState(11)
    mid = 256 if where == "256" else hip.sort_tile_records()
    for R in (mid - 1, mid, mid + 1):
        recs = [b"%d\n" % rng.randint(0, 400) for _ in range(R)]
        want, _ = both(hip, recs, ("R", R), no_text=True)
        assert 100 < want[2] <= 400


# ---- key edges ------------------------------------------------------------------------------------------------------------------

def test_prefixes_zero_bytes_and_word_edges(hip):
    recs = [b"ab\x00", b"ab", b"\x00\x00", b"", b"\x00", b"abcdefghi", b"abcdefgh\x00", b"abcdefgh", b"", b"ab"]
    want, _ = both(hip, recs, "prefixes", trim=-1)
    assert want[0].tolist() == [3, 8, 4, 2, 1, 9, 0, 7, 6, 5] and want[2] == 8
    rng = np.random.RandomState(4)
    recs = []
    for at in (7, 8, 15, 16, 23):                         # pairs that first differ at byte `at`, the longer one with a tail
        a = bytes(rng.randint(97, 123, at + 3).astype(np.uint8))
        b = a[:at] + bytes([a[at] ^ 0x01]) + a[at + 1:]
        recs += [b, a, a[:at], b + b"tail", a]
    both(hip, recs, "first difference")
    # bytes >= 0x80 in the first and the last byte of a word: unsigned order
    recs = [b"\x80", b"\x7f", b"\xff", b"\x00", b"abcdefg\x80x", b"abcdefg\x7fx", b"abcdefg\xffx", b"\x80bcdefgh1", b"\x7fbcdefgh2", b"\xffbcdefgh0",
            b"abcdefgh\x80", b"abcdefgh\x7f", b"abcdefghijklmno\xff", b"abcdefghijklmno\x01"]
    want, _ = both(hip, recs, "high bytes", trim=-1)
    assert want[0].tolist()[0] == 3 and want[0].tolist()[-6:] == [1, 8, 0, 7, 2, 9]


def test_the_trim_byte(hip):
    recs = [b"b\n", b"\n", b"a", b"", b"a\n", b"b\n\n", b"\n\n", b"ab\n", b"b"]
    want, _ = both(hip, recs, "trim")
    assert want[0].tolist() == [1, 3, 6, 2, 4, 7, 0, 8, 5] and want[2] == 6
    want, _ = both(hip, recs, "no trim", trim=-1)         # trim_byte = -1 trims nothing
    assert want[2] == 9
    both(hip, [b"\x00", b"", b"\x00\x00", b"\x00", b"a\x00"], "the trim byte 0", trim=0, seps=(0, -1))


# ---- stability, duplicates, long keys --------------------------------------------------------------------------------------------

def test_equal_keys_keep_their_order(hip):
    want, rounds = both(hip, [b"same\n"] * 1000, "1 000 equal", no_text=True)
    assert want[0].tolist() == list(range(1000)) and (want[1] == 0).all() and rounds <= 2
    want, rounds = both(hip, [b"k" * 3000] * 1000, "1 000 equal of 3 000 bytes", seps=(NL,))
    assert want[0].tolist() == list(range(1000)) and (want[1] == 0).all() and rounds <= 2
    recs = [b"a" * i + b"b" for i in range(64)]
    want, rounds = both(hip, recs, "a^i b", seps=(NL,))
    assert want[0].tolist() == list(range(63, -1, -1)) and rounds <= -(-65 // 8) + 1


def test_dense_duplicates_and_prefixes(hip):
    rng = np.random.RandomState(6)
    recs = letters(rng, 5000, 0, 40)
    want, _ = both(hip, recs, "5 000 over {a, b}", no_text=True)
    assert 1000 < want[2] < 5000
    both(hip, recs, "5 000 over {a, b}, reversed", flags=REVERSE, seps=(NL,))


@functools.lru_cache(maxsize=None)
def bucket_case(name):
    """(off, bytes, the judge's answer): 70 000 keys of two random letters behind eight shared bytes -- three bucket digits are
    launched, the heads the round leaves lie above 65 535, and the prefix skip takes the shared word, so ONE round sorts them;
    "split": behind one of two first words, the second of which begins at position 66 000, and a shared second word: every
    position is still active in round 2, which sorts by a third bucket digit (0 against 66 000) and skips the shared word"""
    rng = np.random.RandomState(8)
    tails = rng.randint(97, 123, (70000, 2)).astype(np.uint8)
    if name == "shared":
        recs = [b"prefix__" + bytes(t) + b"\n" for t in tails]
    else:
        first = rng.permutation(70000) < 66000
        recs = [(b"aaaaaaaa" if first[i] else b"bbbbbbbb") + b"12345678" + bytes(t) + b"\n" for i, t in enumerate(tails)]
    off, data = pack(recs)
    want = sort_ref.sort(off, data, NL, None, NL)
    for a in (off, data, want[0], want[1], want[3], want[4]):
        a.setflags(write=False)
    return off, data, want


@pytest.mark.parametrize("name", ("shared", "split"))
def test_a_third_bucket_digit(hip, name):
    off, data, want = bucket_case(name)
    assert want[2] == 676 if name == "shared" else want[2] > 1300
    p = Packed(off, data)
    one = check(p.run(hip, NL, NL), want, name)
    assert one[4] == (1 if name == "shared" else 2)       # rounds
    two = check(p.run(hip, NL, NL), want, (name, "again"))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one[:4], two[:4]))   # the same call twice: identical arrays
    p.unchanged()


# ---- major and reverse ----------------------------------------------------------------------------------------------------------

def test_major(hip):
    rng = np.random.RandomState(12)
    recs = letters(rng, 700, 0, 12)
    major = rng.choice(np.array([0, 1, 5, 2 ** 40, 2 ** 64 - 1], np.uint64), 700)
    assert (major == 0).any() and (major == 2 ** 64 - 1).any()
    for flags in (0, MAJOR_DESC, REVERSE, MAJOR_DESC | REVERSE):
        want, _ = both(hip, recs, "major", major=major, flags=flags, seps=(NL,), no_text=True)
    plain, _ = both(hip, recs, "no major", seps=(NL,))
    same, _ = both(hip, recs, "one major", major=np.full(700, 9, np.uint64), seps=(NL,))      # all equal: the same as none
    assert all(np.array_equal(a, b) for a, b in zip(plain, same))
    both(hip, [b"x", b"x", b"y", b"x"], "ties", major=[3, 1, 3, 3], trim=-1)


def test_reverse(hip):
    recs = [b"ab", b"ab\x00", b"", b"abcdefgh", b"abcdefghi", b"b", b"ab", b"\xff", b"abcdefgh\x00"]
    want, _ = both(hip, recs, "reverse", trim=-1, flags=REVERSE, no_text=True)
    assert want[0].tolist() == [7, 5, 4, 8, 3, 1, 0, 6, 2]


# ---- placement ------------------------------------------------------------------------------------------------------------------

def test_every_placement_of_the_bytes(hip):
    rng = np.random.RandomState(5)
    recs = letters(rng, 300, 0, 35, b"abc") + [b"tail-of-the-buffer-17"]
    for shift in (1, 7, 15):
        both(hip, recs, ("shift", shift), seps=(NL,), shift=shift)
    for shift in (0, 3):
        both(hip, recs, ("exact", shift), seps=(NL,), shift=shift, exact=True)
    # nbytes below off[R], and an off that decreases: clamped to the limit and to the predecessor; the last records are empty
    data = np.frombuffer(b"zyxwvutsrqponmlkjihgfedcba0123456789", np.uint8)
    off = np.array([0, 4, 2, 9, 20, 30, 36, 36, 500], np.uint64)
    p = Packed(off, data)
    for nbytes in (36, 33, 19, 3, 0):
        check(p.run(hip, -1, NL, 0, nbytes=nbytes), sort_ref.sort(off, data, -1, None, NL, nbytes=nbytes), ("clamp", nbytes))
    p.unchanged()


# ---- fronts ---------------------------------------------------------------------------------------------------------------------

def test_the_extracted_records_and_the_order_as_a_pick(hip):
    import torch
    starts, ends, n = "kw_starts", "kw_ends", 300
    rows, lens = inputs_of(ends)
    pd, td = starts_image(starts), ends_image(ends)
    mt_ref = matches_ref.head(reference(starts, ends), n)
    data, off = lead_packed(rows[:n], lens[:n])
    d_data, d_off = device_u8(data), device_u64(off)
    mt = hip.HipMatches.run_device(pd, td, d_data.data_ptr(), d_off.data_ptr(), n, limit=len(data))
    for xsep in (NL, -1):
        x_off, x_data, _, _ = extract_ref.extract(rows[:n], lens[:n], lens[:n], mt_ref, None, False, xsep)
        ex = mt.extract_device(d_data.data_ptr(), d_off.data_ptr(), n, limit=len(data), sep_byte=xsep)
        for sep, flags in ((NL, 0), (-1, REVERSE)):
            sx = ex.sort(sep, flags)
            torch.cuda.synchronize()
            check(sx, sort_ref.sort(x_off, x_data, xsep, None, sep, flags), ("extracted", xsep, sep, flags))
        assert len(x_off) - 1 > 300
        ex.free()
    mt.free()
    # the lines themselves sorted, and the order as the pick of the matches front: the judge's matches of the reordered lines
    want = sort_ref.sort(off, data, -1, None, -1)
    sx = hip.sort_device(d_off.data_ptr(), d_data.data_ptr(), n, len(data), flags=NO_TEXT)
    torch.cuda.synchronize()
    check(sx, want, "lines", text=False, free=False)
    ordered = want[0].astype(np.int64)
    picked = hip.HipMatches.run_device(pd, td, d_data.data_ptr(), d_off.data_ptr(), n, d_pick=sx.order_ptr, m=n, limit=len(data))
    torch.cuda.synchronize()
    w_off, w_start, w_end, w_id = judged(starts, ends, rows[:n][ordered], lens[:n][ordered])
    g_off, g_start, g_end, g_id = picked.copy()
    assert np.array_equal(g_off, w_off) and np.array_equal(g_start, w_start) and np.array_equal(g_end, w_end) and np.array_equal(g_id, w_id)
    assert len(w_start) > 300
    picked.free()
    sx.free()


def test_the_lines_of_hits_and_the_keys_of_a_distinct_object(hip):
    import torch
    rng = np.random.RandomState(13)
    pool = [b"xx ab yy", b"d", b"nothing here", b"", b"cab", b"www", b"bdb bdb", b"xx ab yy ", b"abc"]
    lines = [pool[k] for k in rng.permutation(np.repeat(np.arange(len(pool)), (40, 25, 30, 20, 25, 10, 8, 8, 3)))]   # two pairs of equal counts
    lines.append(b"the last line has a d")
    blob = b"".join(x + b"\n" for x in lines)[:-1]
    text = hip.HipText(blob, NL)
    hits = text.hits(hip.LinesDfa(span_ref.line_matcher_of(KEYWORDS)[0], NL))
    recs = [x + b"\n" for x in lines if any(k in x for k in KEYWORDS)]
    recs[-1] = recs[-1][:-1]                              # the text's last line has no delimiter: the same key without it
    assert hits.count == len(recs) and 60 < len(recs) < 200
    off, data = pack(recs)
    for sep, flags in ((NL, 0), (-1, 0), (NL, REVERSE)):
        sx = hits.sort(sep, flags)
        torch.cuda.synchronize()
        check(sx, sort_ref.sort(off, data, NL, None, sep, flags), ("hits", sep, flags))
    bare = text.hits(hip.LinesDfa(span_ref.line_matcher_of(KEYWORDS)[0], NL), want_bytes=False)   # FSM_HIP_HITS_NO_BYTES
    with pytest.raises(OSError) as ei:
        bare.sort(NL)
    assert ei.value.errno == errno.EINVAL
    # the distinct lines: their keys in byte order, and by count -- the judge applied to the distinct judge's output
    for dsep in (NL, -1):
        _, d_count, _, d_off, d_data = distinct_ref.distinct(off, data, NL, None, dsep)
        dx = hits.distinct(dsep)
        plain = dx.sort(sep_byte=NL)
        by_count = dx.sort(by_count=True, sep_byte=NL)
        no_text = dx.sort(by_count=True, sep_byte=NL, flags=NO_TEXT | REVERSE)
        torch.cuda.synchronize()
        D = len(d_count)
        assert D == 7 and len(set(d_count.tolist())) < D  # (ties among the counts)
        check(plain, sort_ref.sort(d_off, d_data, dsep, None, NL), ("keys", dsep))
        check(by_count, sort_ref.sort(d_off, d_data, dsep, d_count, NL, MAJOR_DESC), ("keys by count", dsep))
        check(no_text, sort_ref.sort(d_off, d_data, dsep, d_count, NL, MAJOR_DESC | REVERSE), ("keys by count, reversed", dsep), text=False)
        lib = hip.load_library()
        import ctypes as C
        C.set_errno(0)
        assert not lib.fsm_hip_keys_sort(dx.handle, NL, MAJOR_DESC, None) and C.get_errno() == errno.EINVAL   # MAJOR_DESC without BY_COUNT
        dx.free()
        sx = hits.sort(NL)                                # a plain sort of the same records: as many groups as distinct keys
        assert sx.groups == D
        sx.free()
    nt = hits.distinct(NL, hip.DISTINCT_NO_TEXT)
    with pytest.raises(OSError) as ei:
        nt.sort()
    assert ei.value.errno == errno.EINVAL


def test_the_host_form_and_misuse(hip):
    rng = np.random.RandomState(3)
    recs = letters(rng, 900, 0, 20, b"abc\n")
    off, data = pack(recs)
    major = rng.randint(0, 3, 900).astype(np.uint64)
    check(hip.sort(off, data, NL, None, NL), sort_ref.sort(off, data, NL, None, NL), "host")
    check(hip.sort(off, data, NL, major, -1, MAJOR_DESC), sort_ref.sort(off, data, NL, major, -1, MAJOR_DESC), "host, major")
    check(hip.sort([0], b"", NL, None, NL), sort_ref.sort([0], b""), "host, R = 0")
    p = Packed(off, data, major)
    o, b, m = p.d_off.data_ptr(), p.d_data.data_ptr(), p.d_major.data_ptr()
    for args, want in (((0, b, 2, 2), errno.EINVAL), ((o, 0, 2, 2), errno.EINVAL), ((o, b, 2, 2, 256), errno.EINVAL), ((o, b, 2, 2, -2), errno.EINVAL),
                       ((o, b, 2, 2, -1, 0, 256), errno.EINVAL), ((o, b, 2, 2, -1, 0, -2), errno.EINVAL), ((o, b, 2, 2, -1, 0, -1, 16), errno.EINVAL),
                       ((o, b, 2, 2, -1, 0, -1, MAJOR_DESC), errno.EINVAL), ((o, b, 2, 2, -1, m, -1, sort_ref.BY_COUNT), errno.EINVAL),
                       ((o, b, 2 ** 32 - 1, 2), errno.EOVERFLOW)):
        with pytest.raises(OSError) as ei:
            hip.sort_device(*args)
        assert ei.value.errno == want, args
    with pytest.raises(OSError) as ei:
        hip.sort([0, 3, 2], b"abc")                       # a decreasing off: before any launch
    assert ei.value.errno == errno.EINVAL
    sx = p.run(hip, NL, NL, NO_TEXT)
    with pytest.raises(OSError) as ei:
        hip.capi._call("fsm_hip_sorted_copy", sx.handle, None, None, np.zeros(901, np.uint64).ctypes.data_as(hip.capi.P), None)
    assert ei.value.errno == errno.EINVAL
    sx.free()
    check(p.run(hip, NL, NL), sort_ref.sort(off, data, NL, major, NL), "after misuse")
    p.unchanged()


# ---- the example ----------------------------------------------------------------------------------------------------------------

def test_example_prints_the_keys_in_byte_order(hip, tmp_path):
    """examples/hipuniq.c -s over two small files: count<TAB>value per distinct match in byte order, with -c by count first"""
    from line_inputs import auto_of
    from matches_ref import DROP_EMPTY
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.RandomState(17)
    pool = [b"xx ab yy", b"d", b"nothing here", b"", b"cab", b"bdb bdb", b"abc d"]
    files = [[pool[k] for k in rng.randint(0, len(pool), m)] for m in (70, 30)]
    tables = []
    for nm, auto in (("lines", span_ref.line_matcher_of(KEYWORDS)), ("starts", auto_of("kw_starts")[0]), ("ends", auto_of("kw_ends")[0])):
        tables.append(str(tmp_path / (nm + ".fsmhip")))
        auto[0].write_c(tables[-1])
    names = []
    for j, ls in enumerate(files):
        blob = b"".join(x + b"\n" for x in ls)
        (tmp_path / ("f%d.txt" % j)).write_bytes(blob[:-1] if j == 1 else blob)
        names.append(str(tmp_path / ("f%d.txt" % j)))
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    exe = str(tmp_path / "hipuniq")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "hipuniq.c"),
                           "-o", exe, "-L" + os.path.join(root, "libfsm_amd"), "-lfsm_hip", "-Wl,-rpath," + os.path.join(root, "libfsm_amd")])
    lines = [x for ls in files for x in ls]
    rows, lens = span_ref.rows_of(lines)
    x_off, x_data, _, _ = extract_ref.extract(rows, lens, lens, judged("kw_starts", "kw_ends", rows, lens, DROP_EMPTY), None, False, NL)
    _, count, _, doff, data = distinct_ref.distinct(x_off, x_data, NL, None, NL)
    keys = extract_ref.records_of(doff, data)
    assert len(keys) >= 4
    for args, major, flags in ((("-s",), None, 0), (("-s", "-c"), count, MAJOR_DESC), (("-c", "-s", ), count, MAJOR_DESC)):
        order = sort_ref.sort(doff, data, NL, major, NL, flags)[0]
        want = b"".join(b"%d\t%s" % (count[int(d)], keys[int(d)]) for d in order)
        r = subprocess.run([exe, *args, *tables, *names], capture_output=True, env=env, timeout=120)
        assert (r.returncode, r.stdout) == (0, want), (args, r.stderr)
