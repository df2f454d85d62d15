"""GPU: the distinct records of a packed text (libfsm_amd/csrc/distinct.hip: dst_hash, dst_hash_long, dst_insert, dst_mark,
dst_number, dst_class and the fronts; the scan of the block pairs in text.hip, the write pass in extract.hip).

first, count, class, doff and every byte of the keys are compared with tests/distinct_ref.py, the definition of include/fsm_hip.h
("distinct") restated as a Python dict over the trimmed keys in record order -- nothing that came from the device is ever used to
judge the device.  Every case runs with and without FSM_HIP_DISTINCT_WEAK_HASH, which puts every probe chain's start into the last
four slots of the table.  The caller's arrays on the device are longer than needed and pre-filled: they and what lies behind them
are unchanged afterwards; the copies out are two entries too long and pre-filled: nothing behind D, R or the bytes is written."""
import ctypes as C
import errno
import functools
import os
import subprocess

import numpy as np
import pytest

import distinct_ref
import extract_ref
import matches_ref
import span_ref
from distinct_ref import NO_TEXT, WEAK_HASH, pack
from line_inputs import FILL, KEYWORDS, auto_of, device_u64, device_u8, ends_image, inputs_of, judged, lead_packed, reference, starts_image
from matches_ref import DROP_EMPTY

pytestmark = pytest.mark.gpu

NL = 0x0A
GUARD = 64                                   # bytes behind the text that belong to no record
HASHES = pytest.mark.parametrize("weak", (0, WEAK_HASH), ids=("hash", "weak"))


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()   # raises if the HIP extension is missing: no silent fallback
    return libfsm_amd


def device_u32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).cuda()


class Packed:
    """a packed text (and its tags) on the device: `shift` bytes in front of the first byte, GUARD bytes and two entries of FILL
    behind every array; exact: the bytes' allocation ends with the text"""

    def __init__(self, off, data, tag=None, shift=0, exact=False):
        self.off, self.data = np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(data, np.uint8)
        self.tag = None if tag is None else np.ascontiguousarray(tag, np.uint32)
        self.R, self.shift = len(self.off) - 1, shift
        self.h_data = np.concatenate([np.full(shift, 0xEE, np.uint8), self.data, np.full(0 if exact else GUARD, FILL & 0xFF, np.uint8)])
        self.h_off = np.concatenate([self.off, np.full(2, FILL, np.uint64)])
        self.h_tag = None if tag is None else np.concatenate([self.tag, np.full(2, FILL & 0xFFFFFFFF, np.uint32)])
        self.d_data = device_u8(self.h_data if len(self.h_data) else np.zeros(1, np.uint8))
        self.d_off = device_u64(self.h_off)
        self.d_tag = None if tag is None else device_u32(self.h_tag)
        assert shift == 0 or self.d_data.data_ptr() % 256 == 0

    def run(self, hip, trim=-1, sep=-1, flags=0, nbytes=None):
        import torch
        dx = hip.distinct_device(self.d_off.data_ptr(), self.d_data.data_ptr() + self.shift, self.R, len(self.data) if nbytes is None else nbytes, trim,
                                 self.d_tag.data_ptr() if self.d_tag is not None else 0, sep, flags, keep=(self,))
        torch.cuda.synchronize()
        return dx

    def unchanged(self):
        assert np.array_equal(self.d_off.cpu().numpy().view(np.uint64), self.h_off)
        assert len(self.h_data) == 0 or np.array_equal(self.d_data.cpu().numpy(), self.h_data)
        assert self.d_tag is None or np.array_equal(self.d_tag.cpu().numpy().view(np.uint32), self.h_tag)


def check(dx, want, what, text=True, free=True):
    """a distinct object against the judge's (first, count, class, doff, dbytes), in full, and the properties on their own"""
    w_first, w_count, w_cls, w_doff, w_data = want
    D, R, total = len(w_first), len(w_cls), int(w_doff[-1]) if text else 0
    assert (dx.count, dx.records, dx.nbytes) == (D, R, total), (what, "D, R, nbytes", dx.count, dx.records, dx.nbytes, D, R, total)
    assert (dx.first_ptr != 0) == (D != 0) and (dx.count_ptr != 0) == (D != 0) and (dx.class_ptr != 0) == (R != 0), what
    assert (dx.off_ptr != 0) == text and (dx.bytes_ptr != 0) == (total != 0), what
    first, count, cls, doff, data = dx.copy(extra=2, fill=FILL)
    assert (first[D:] == FILL).all() and (count[D:] == FILL).all() and (cls[R:] == FILL & 0xFFFFFFFF).all(), what
    for name, got, w in (("first", first[:D], w_first), ("count", count[:D], w_count), ("class", cls[:R], w_cls)):
        bad = np.flatnonzero(got != w)
        assert len(bad) == 0, (what, name, bad[:5], got[bad[:5]], w[bad[:5]])
    assert (np.diff(first[:D].astype(np.int64)) > 0).all() and int(count[:D].sum()) == R, what
    assert R == 0 or ((first[:D][cls[:R]] <= np.arange(R)).all() and (first[:D][cls[first[:D].astype(np.int64)]] == first[:D]).all()), what
    if text:
        assert (doff[D + 1:] == FILL).all() and (data[total:] == FILL & 0xFF).all(), what
        bad = np.flatnonzero(doff[:D + 1] != w_doff)
        assert len(bad) == 0, (what, "doff", bad[:5], doff[bad[:5]], w_doff[bad[:5]])
        bad = np.flatnonzero(data[:total] != w_data)
        assert len(bad) == 0, (what, "bytes", bad[:8], data[bad[:8]], w_data[bad[:8]], "key", np.searchsorted(w_doff, bad[:8], "right") - 1)
    else:
        assert doff is None and data is None
    assert dx.ms >= 0.0 and all(dx.pass_ms(k) >= 0.0 for k in range(4))
    if free:
        dx.free()
    return first[:D], count[:D], cls[:R], None if doff is None else doff[:D + 1], None if data is None else data[:total]


def both(hip, records, what, weak, trim=NL, tag=None, seps=(NL, -1), shift=0, exact=False):
    """the records through the device form, with every separator, against the judge; -> the judge's last answer"""
    off, data = pack(records)
    p = Packed(off, data, tag, shift, exact)
    for sep in seps:
        want = distinct_ref.distinct(off, data, trim, tag, sep)
        check(p.run(hip, trim, sep, weak), want, (what, sep, weak))
    p.unchanged()
    return want


# ---- sizes and shapes ----------------------------------------------------------------------------------------------------------

@HASHES
def test_no_record_and_one(hip, weak):
    want = both(hip, [], "R = 0", weak)
    assert len(want[0]) == 0 and want[3].tolist() == [0]
    p = Packed([7], np.zeros(0, np.uint8))                # off[0] alone, and not 0: nothing is read
    check(p.run(hip, NL, NL, weak | NO_TEXT), distinct_ref.distinct([7], b"", NL, None, NL), "R = 0, no text", text=False)
    for rec in (b"", b"\n", b"x", b"x\n", b"0123456789abcdefg"):
        want = both(hip, [rec], ("R = 1", rec), weak)
        assert len(want[0]) == 1 and want[1].tolist() == [1]


@HASHES
def test_more_equal_records_than_a_workgroup(hip, weak):
    want = both(hip, [b"same\n"] * 300, "300 equal", weak)
    assert want[0].tolist() == [0] and want[1].tolist() == [300] and bytes(want[4]) == b"same"
    want = both(hip, [b"x"] + [b"same\n"] * 299 + [b"x\n"], "300 equal between two others", weak)
    assert want[0].tolist() == [0, 1] and want[1].tolist() == [2, 299]


@HASHES
def test_a_thousand_different_records(hip, weak):
    recs = [b"%d\n" % (i * 7919) for i in range(1000)]
    want = both(hip, recs, "1 000 different", weak)
    assert len(want[0]) == 1000 and (want[1] == 1).all() and want[2].tolist() == list(range(1000))


def test_five_records_in_sixteen_slots_wrap(hip):
    """under the weak hash the chains of five one-byte keys start in slot 13 of 16: the fourth key wraps to slot 0"""
    assert hip.distinct_table_slots(5) == 16
    want = both(hip, [b"a", b"b", b"c", b"a", b"e", ], "five in sixteen", WEAK_HASH, trim=-1)
    assert want[0].tolist() == [0, 1, 2, 4] and want[1].tolist() == [2, 1, 1, 1]
    both(hip, [b"e", b"d", b"c", b"b", b"a", b"e", b"d", b"c"], "eight in sixteen", WEAK_HASH, trim=-1)


# ---- key edges ------------------------------------------------------------------------------------------------------------------

def edge_pairs():
    """pairs that differ in their last byte only, at the chunk edges, each twice, with and without the trim byte"""
    rng = np.random.RandomState(5)
    recs = []
    for n in (15, 16, 17, 31, 32, 33):
        a = bytes(rng.randint(97, 123, n).astype(np.uint8))
        b = a[:-1] + bytes([a[-1] ^ 0x01])
        recs += [a, b + b"\n", a + b"\n", b, a[:-1]]
    return recs


@HASHES
def test_the_trim_byte_and_the_chunk_edges(hip, weak):
    recs = [b"", b"\n", b"a\n", b"a", b"b\n\n", b"b\n", b"b", b"ab", b"abc", b"ab\n", b"", b"\n\n"]
    want = both(hip, recs, "trim", weak)
    assert want[2].tolist() == [0, 0, 1, 1, 2, 3, 3, 4, 5, 4, 0, 6] and bytes(want[4]) == b"ab\nbababc\n"
    want = both(hip, recs, "no trim", weak, trim=-1)     # trim_byte = -1 trims nothing
    assert len(want[0]) == 11 and want[1].tolist() == [2] + [1] * 10
    want = both(hip, edge_pairs(), "pairs", weak)
    assert len(want[0]) == 6 * 3 and sorted(want[1].tolist()) == [1] * 6 + [2] * 12
    both(hip, [b"\x00", b"", b"\x00\x00", b"\x00"], "the trim byte 0", weak, trim=0, seps=(0, -1))


@HASHES
def test_every_alignment_of_the_bytes(hip, weak):
    recs = edge_pairs()
    for shift in range(1, 16):
        both(hip, recs, ("shift", shift), weak, seps=(NL,), shift=shift)


@HASHES
def test_the_last_record_ends_the_buffer_and_offsets_are_clamped(hip, weak):
    recs = edge_pairs() + [b"tail-of-the-buffer-17"]
    for shift in (0, 3):
        both(hip, recs, ("exact", shift), weak, seps=(NL,), shift=shift, exact=True)
    # nbytes below off[R], and an off that decreases: clamped to the limit and to the predecessor; bytes behind the limit are not keys
    data = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789", np.uint8)
    off = np.array([0, 4, 2, 9, 20, 30, 36, 36, 500], np.uint64)
    p = Packed(off, data)
    for nbytes in (36, 33, 19, 3, 0):
        want = distinct_ref.distinct(off, data, -1, None, NL, nbytes=nbytes)
        check(p.run(hip, -1, NL, weak, nbytes=nbytes), want, ("clamp", nbytes))
    # off[R] below nbytes: the limit is off[R]
    off = np.array([0, 4, 8, 2], np.uint64)
    want = distinct_ref.distinct(off, data, -1, None, NL)
    assert [bytes(k) for k in distinct_ref.keys_of(off, data)] == [b"ab", b"", b""]
    check(Packed(off, data).run(hip, -1, NL, weak), want, "limit off[R]")
    p.unchanged()


# ---- long records ---------------------------------------------------------------------------------------------------------------

@HASHES
def test_long_records(hip, weak):
    L = hip.distinct_long_bytes()
    rng = np.random.RandomState(9)
    body = bytes(rng.randint(0, 256, 70000).astype(np.uint8))
    recs = []
    for n in (L - 1, L, L + 1):
        recs += [body[:n], body[:n] + b"\n", body[:n - 1] + bytes([body[n - 1] ^ 0x80])]
    recs += [body, body[:-1] + bytes([body[-1] ^ 1]), body]            # two of 70 000 bytes that differ in the last, a third equal to the first
    recs += [body[:L], body[:2 * L + 5], body[:2 * L + 5] + b"\n"]      # a long one equal in its first L bytes to a short one
    want = both(hip, recs, "long", weak, seps=(NL,))
    assert want[1].tolist() == [2, 1, 3, 1, 2, 1, 2, 1, 2] and int(want[3][-1]) > 140000


# ---- tags -----------------------------------------------------------------------------------------------------------------------

@HASHES
def test_tags(hip, weak):
    recs = [b"x\n", b"x", b"y", b"x", b"y\n", b"", b"\n", b"x"]
    tag = [1, 2, 1, 1, 1, 0, 0xFFFFFFFF, 2]
    want = both(hip, recs, "tags", weak, tag=tag)
    assert want[2].tolist() == [0, 1, 2, 0, 2, 3, 4, 1]                 # equal bytes under different tags stay apart, equal tags merge
    want = both(hip, recs, "one tag", weak, tag=[9] * 8)
    none = both(hip, recs, "no tags", weak)                             # d_tag = NULL
    assert all(np.array_equal(a, b) for a, b in zip(want, none)) and want[2].tolist() == [0, 0, 1, 0, 1, 2, 2, 0]
    rng = np.random.RandomState(3)
    recs = [bytes(rng.choice(list(b"ab"), rng.randint(0, 4)).astype(np.uint8)) for _ in range(3000)]
    both(hip, recs, "random tags", weak, tag=rng.randint(0, 3, 3000), seps=(NL,))


# ---- properties -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def property_case(name):
    """(off, bytes, the judge's answer with '\\n' between the keys): computed once, left unchanged"""
    rng = np.random.RandomState(21)
    if name == "few keys":
        recs = [bytes(rng.choice(list(b"ab"), rng.randint(0, 6)).astype(np.uint8)) + (b"\n" if rng.randint(2) else b"") for _ in range(20000)]
    elif name == "all different":
        rows = rng.randint(0, 256, (20000, 24)).astype(np.uint8)
        rows[:, 23] = 0x41
        recs = [bytes(r) for r in rows]
    else:
        which = rng.choice(3, 100000, p=(0.98, 0.01, 0.01))
        recs = [(b"GET /index.html", b"POST /login", b"x")[k] + b"\n" for k in which]
    off, data = pack(recs)
    want = distinct_ref.distinct(off, data, NL, None, NL)
    for a in (off, data) + want:
        a.setflags(write=False)
    return off, data, want


@HASHES
@pytest.mark.parametrize("name", ("few keys", "all different", "three keys"))
def test_properties_and_two_runs_alike(hip, weak, name):
    off, data, want = property_case(name)
    D = len(want[0])
    assert {"few keys": D < 70, "all different": D == 20000, "three keys": D == 3}[name]
    p = Packed(off, data)
    one = check(p.run(hip, NL, NL, weak), want, (name, weak))
    two = check(p.run(hip, NL, NL, weak), want, (name, weak, "again"))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, two))
    p.unchanged()
    if name == "three keys":
        assert sorted(want[1].tolist())[2] > 97000


@HASHES
def test_the_keys_fed_back_are_all_distinct(hip, weak):
    """idempotence: doff / dbytes, as they lie on the device, with trim_byte = sep_byte give D again, every count 1"""
    import torch
    off, data, want = property_case("few keys")
    D = len(want[0])
    p = Packed(off, data)
    for sep in (NL, -1):
        w1 = distinct_ref.distinct(off, data, NL, None, sep)
        dx = p.run(hip, NL, sep, weak)
        check(dx, w1, ("first", sep), free=False)
        back = hip.distinct_device(dx.off_ptr, dx.bytes_ptr, dx.count, dx.nbytes, sep, 0, sep, weak, keep=(dx,))
        torch.cuda.synchronize()
        w2 = distinct_ref.distinct(w1[3], w1[4], sep, None, sep)
        got = check(back, w2, ("back", sep))
        assert got[0].tolist() == list(range(D)) and (got[1] == 1).all() and np.array_equal(got[4], w1[4])
        dx.free()


# ---- fronts ---------------------------------------------------------------------------------------------------------------------

@HASHES
def test_the_extracted_records_of_the_keyword_lines(hip, weak):
    import torch
    starts, ends, n = "kw_starts", "kw_ends", 1500
    rows, lens = inputs_of(ends)
    pd, td = starts_image(starts), ends_image(ends)
    mt_ref = matches_ref.head(reference(starts, ends), n)
    data, off = lead_packed(rows[:n], lens[:n])
    d_data, d_off = device_u8(data), device_u64(off)
    mt = hip.HipMatches.run_device(pd, td, d_data.data_ptr(), d_off.data_ptr(), n, limit=len(data))
    for keep in (None, (len(KEYWORDS), {0, 2})):
        rs = None if keep is None else hip.HipRules(sorted(keep[1]), keep[0])
        for xsep in (NL, -1):
            x_off, x_data, _, _ = extract_ref.extract(rows[:n], lens[:n], lens[:n], mt_ref, keep, False, xsep)
            ex = mt.extract_device(d_data.data_ptr(), d_off.data_ptr(), n, limit=len(data), keep=rs, sep_byte=xsep)
            for sep in (NL, -1):
                want = distinct_ref.distinct(x_off, x_data, xsep, None, sep)
                dx = ex.distinct(sep, weak)
                torch.cuda.synchronize()
                check(dx, want, ("extracted", keep, xsep, sep))
            assert len(want[0]) == (5 if keep is None else 2) and len(x_off) - 1 > 2000
            ex.free()


def three_files():
    """three files of keyword and other lines with repeats, the last without a final delimiter -> (the lines per file, blob, file_off)"""
    rng = np.random.RandomState(13)
    pool = [b"xx ab yy", b"d", b"nothing here", b"", b"cab", b"www", b"bdb bdb", b"xx ab yy "]
    files = [[pool[k] for k in rng.randint(0, len(pool), m)] for m in (90, 40, 25)]
    files[2][-1] = b"the last line has a d"
    blobs = [b"".join(x + b"\n" for x in ls) for ls in files]
    blobs[2] = blobs[2][:-1]
    return files, b"".join(blobs), np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)


@HASHES
def test_the_lines_of_the_hits_of_three_files(hip, weak):
    import torch
    files, blob, fo = three_files()
    text = hip.HipText(blob, NL, file_off=fo)
    ld = hip.LinesDfa(span_ref.line_matcher_of(KEYWORDS)[0], NL)
    hits = text.hits(ld)
    lines = [x for ls in files for x in ls]
    picked = [x for x in lines if any(k in x for k in KEYWORDS)]
    assert hits.count == len(picked) and 40 < len(picked) < len(lines)
    recs = [x + b"\n" for x in picked]
    recs[-1] = recs[-1][:-1]                                           # the text's last line has no delimiter: the same key without it
    for sep in (NL, -1):
        want = distinct_ref.distinct(*pack(recs), NL, None, sep)
        dx = hits.distinct(sep, weak)
        torch.cuda.synchronize()
        check(dx, want, ("hits", sep))
    assert len(want[0]) == 6
    bare = text.hits(ld, want_bytes=False)                             # FSM_HIP_HITS_NO_BYTES: no lines on the device
    with pytest.raises(OSError) as ei:
        bare.distinct(NL, weak)
    assert ei.value.errno == errno.EINVAL


@HASHES
def test_the_host_form_no_text_and_the_tally_over_class(hip, weak):
    import torch
    off, data, want = property_case("few keys")
    rng = np.random.RandomState(2)
    tag = rng.randint(0, 2, len(off) - 1).astype(np.uint32)
    check(hip.distinct(off, data, NL, None, NL, weak), want, "host")
    check(hip.distinct(off, data, NL, tag, -1, weak), distinct_ref.distinct(off, data, NL, tag, -1), "host, tags")
    check(hip.distinct([0], b"", NL, None, NL, weak), distinct_ref.distinct([0], b""), "host, R = 0")
    with pytest.raises(OSError) as ei:
        hip.distinct([0, 3, 2], b"abc", NL, None, NL, weak)              # a decreasing off: before any launch
    assert ei.value.errno == errno.EINVAL
    # NO_TEXT: first, count and class alone
    p = Packed(off, data)
    dx = p.run(hip, NL, NL, weak | NO_TEXT)
    check(dx, want, "no text", text=False, free=False)
    # class as the tally's id array, one input per record: the count row is count[D] and nothing in "other"
    R, D = len(off) - 1, len(want[0])
    d_one = device_u64(np.arange(R + 1, dtype=np.uint64))
    tab = device_u64(np.full(D + 3, FILL, np.uint64))
    hip.tally_ids_device(d_one.data_ptr(), dx.class_ptr, R, R, 0, 0, D, tab.data_ptr(), 0)
    torch.cuda.synchronize()
    got = tab.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[:D], want[1]) and got[D] == 0 and (got[D + 1:] == FILL).all()
    dx.free()


# ---- misuse ---------------------------------------------------------------------------------------------------------------------

def test_misuse_is_refused_before_any_launch(hip):
    p = Packed(*pack([b"a", b"b"]))
    o, b = p.d_off.data_ptr(), p.d_data.data_ptr()
    for args, want in (((0, b, 2, 2), errno.EINVAL),                                   # d_off NULL
                       ((o, 0, 2, 2), errno.EINVAL),                                   # d_bytes NULL with nbytes > 0
                       ((o, b, 2, 2, 256), errno.EINVAL), ((o, b, 2, 2, -2), errno.EINVAL),
                       ((o, b, 2, 2, -1, 0, 256), errno.EINVAL), ((o, b, 2, 2, -1, 0, -2), errno.EINVAL),
                       ((o, b, 2, 2, -1, 0, -1, 4), errno.EINVAL), ((o, b, 2, 2, -1, 0, -1, 0x80000000), errno.EINVAL),
                       ((o, b, 2 ** 32 - 1, 2), errno.EOVERFLOW), ((o, b, 2 ** 40, 2), errno.EOVERFLOW)):
        with pytest.raises(OSError) as ei:
            hip.distinct_device(*args)
        assert ei.value.errno == want, args
    lib = hip.load_library()
    for fn in (lib.fsm_hip_extracted_distinct, lib.fsm_hip_text_hits_distinct):
        C.set_errno(0)
        assert not fn(None, -1, 0, None) and C.get_errno() == errno.EINVAL
    dx = p.run(hip, -1, -1, NO_TEXT)
    assert dx.count == 2 and dx.off_ptr == 0
    doff = np.zeros(3, np.uint64)
    C.set_errno(0)
    assert lib.fsm_hip_distinct_copy(dx.handle, None, None, None, doff.ctypes.data_as(C.c_void_p), None) == -1 and C.get_errno() == errno.EINVAL
    C.set_errno(0)
    assert lib.fsm_hip_distinct_pass_ms(dx.handle, 4) == -1.0 and C.get_errno() == errno.EINVAL
    dx.free()
    check(Packed(*pack([b"a", b"b"])).run(hip, -1, NL, 0, nbytes=2), distinct_ref.distinct(*pack([b"a", b"b"]), -1, None, NL), "after misuse")
    p.unchanged()


# ---- the example ----------------------------------------------------------------------------------------------------------------

def test_example_prints_the_judges_text(hip, tmp_path):
    """examples/hipuniq.c over three small files, the last without a final newline: count<TAB>value per distinct match in the
    order of first appearance, -c by count, -l the matching lines instead of the matches"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files, _, _ = three_files()
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
    exe = str(tmp_path / "hipuniq")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "hipuniq.c"),
                           "-o", exe, "-L" + os.path.join(root, "libfsm_amd"), "-lfsm_hip", "-Wl,-rpath," + os.path.join(root, "libfsm_amd")])

    def run(*args, fs=names):
        r = subprocess.run([exe, *args, *tables, *fs], capture_output=True, env=env, timeout=120)
        return r.returncode, r.stdout

    def compose(by_lines=False, by_count=False, keep=None):
        lines = [x for ls in files for x in ls]
        if by_lines:
            recs = [x + b"\n" for x in lines if any(k in x for k in KEYWORDS)]
        else:
            rows, lens = span_ref.rows_of(lines)
            x_off, x_data, _, _ = extract_ref.extract(rows, lens, lens, judged("kw_starts", "kw_ends", rows, lens, DROP_EMPTY), keep, False, NL)
            recs = extract_ref.records_of(x_off, x_data)
        _, count, _, doff, data = distinct_ref.distinct(*pack(recs), NL, None, NL)
        keys = extract_ref.records_of(doff, data)
        order = sorted(range(len(keys)), key=lambda d: (-int(count[d]), d)) if by_count else range(len(keys))
        return b"".join(b"%d\t%s" % (count[d], keys[d]) for d in order)

    want = compose()
    assert want.count(b"\n") >= 3 and b"\tab\n" in want and b"\td\n" in want
    assert run() == (0, want)
    assert run("-c") == (0, compose(by_count=True)) and compose(by_count=True) != want
    assert run("-l") == (0, compose(by_lines=True)) and compose(by_lines=True).count(b"\n") == 6
    assert run("-l", "-c") == (0, compose(by_lines=True, by_count=True))
    assert run("-r", "0,2") == (0, compose(keep=(5, {0, 2}))) and 1 <= compose(keep=(5, {0, 2})).count(b"\n") < want.count(b"\n")
    quiet = tmp_path / "none.txt"
    quiet.write_bytes(b"xyz\nwwww\n\n")
    assert run(fs=[str(quiet)]) == (1, b"")
