"""GPU: the records of a packed text looked up among the keys of a distinct object (libfsm_amd/csrc/distinct.hip: dst_hash and
dst_hash_long over the probe, fnd_probe, fnd_probe_long, fnd_mark, fnd_pick and the fronts; the scan of the block pairs in text.hip).

class, the bitmap, pick and present are compared in full with tests/find_ref.py, the definition of include/fsm_hip.h ("find")
restated as a Python dict over distinct_ref.keys_of -- nothing that came from the device is ever used to judge the device.  Every
case runs against a dictionary built with and without FSM_HIP_DISTINCT_WEAK_HASH, which puts every probe chain's start into the last
four slots of the table.  The caller's arrays on the device are longer than needed and pre-filled: they and what lies behind them are
unchanged afterwards, and so is the dictionary; the copies out are two entries too long and pre-filled: nothing behind R or the
bitmap's words is written."""
import ctypes as C
import errno
import functools
import os
import subprocess

import numpy as np
import pytest

import distinct_ref
import extract_ref
import find_ref
import hits_ref
import matches_ref
import span_ref
from distinct_ref import WEAK_HASH, pack
from find_ref import NO_PICK, NONE
from line_inputs import FILL, KEYWORDS, device_u64, device_u8, ends_image, inputs_of, lead_packed, reference, starts_image
from test_gpu_distinct import Packed, three_files

pytestmark = pytest.mark.gpu

NL = 0x0A
HASHES = pytest.mark.parametrize("weak", (0, WEAK_HASH), ids=("hash", "weak"))


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()   # raises if the HIP extension is missing: no silent fallback
    return libfsm_amd


class Dictionary:
    """a distinct object over a Packed source, and the judge's numbers of its keys"""

    def __init__(self, hip, records, weak, trim=NL, tag=None, shift=0, exact=False, nbytes=None, packed=None):
        off, data = pack(records) if packed is None else packed
        self.src = Packed(off, data, tag, shift, exact)
        self.dx = self.src.run(hip, trim, NL, weak, nbytes=nbytes)
        self.number = find_ref.numbers_of(off, data, trim, tag, nbytes)
        assert self.dx.count == len(self.number)
        self.before = self.dx.copy()

    def unchanged(self):
        """the dictionary is const: its source and every array of the object are bit for bit what they were"""
        self.src.unchanged()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(self.before, self.dx.copy()))


def find_device(hip, d, p, trim, flags=0, nbytes=None, stream=0):
    return d.dx.find_device(p.d_off.data_ptr(), p.d_data.data_ptr() + p.shift, p.R, len(p.data) if nbytes is None else nbytes, trim,
                            p.d_tag.data_ptr() if p.d_tag is not None else 0, flags, stream, keep=(p,))


def check(fx, want, what, pick=True, free=True):
    """a found object against the judge's (class, bitmap, pick, present), in full, and the properties on their own"""
    w_cls, w_bitmap, w_pick, P = want
    R, W = len(w_cls), len(w_bitmap)
    assert (fx.records, fx.present) == (R, P), (what, "R, P", fx.records, fx.present, R, P)
    assert (fx.class_ptr != 0) == (R != 0) and (fx.bitmap_ptr != 0) == (R != 0) and (fx.pick_ptr != 0) == (R != 0 and pick), what
    cls, bitmap, got_pick = fx.copy(extra=2, fill=FILL)
    assert (cls[R:] == FILL & 0xFFFFFFFF).all() and (bitmap[W:] == FILL).all(), what
    for name, got, w in (("class", cls[:R], w_cls), ("bitmap", bitmap[:W], w_bitmap)):
        bad = np.flatnonzero(got != w)
        assert len(bad) == 0, (what, name, bad[:5], got[bad[:5]], w[bad[:5]])
    assert R % 64 == 0 or int(bitmap[W - 1]) >> (R % 64) == 0, what                       # the zero tail
    assert int(np.unpackbits(bitmap[:W].view(np.uint8)).sum()) == P, what
    if pick or R == 0:
        assert (got_pick[R:] == FILL).all(), what
        bad = np.flatnonzero(got_pick[:R] != w_pick)
        assert len(bad) == 0, (what, "pick", bad[:5], got_pick[bad[:5]], w_pick[bad[:5]])
        for half in (got_pick[:P], got_pick[P:R]):
            assert (np.diff(half.astype(np.int64)) > 0).all(), what
        assert (cls[got_pick[:P].astype(np.int64)] != NONE).all() and (cls[got_pick[P:R].astype(np.int64)] == NONE).all(), what
    else:
        assert got_pick is None, what
    assert fx.ms >= 0.0 and all(fx.pass_ms(k) >= 0.0 for k in range(4)), what
    if free:
        fx.free()
    return cls[:R], bitmap[:W], None if got_pick is None else got_pick[:R]


def lookup(hip, d, records, what, trim=NL, tag=None, shift=0, exact=False, nbytes=None, flags=(0, NO_PICK), packed=None):
    """the probe records through the device form, with and without pick, against the judge; -> the judge's answer"""
    import torch
    off, data = pack(records) if packed is None else packed
    p = Packed(off, data, tag, shift, exact)
    want = find_ref.find(d.number, off, data, trim, tag, nbytes)
    for fl in flags:
        fx = find_device(hip, d, p, trim, fl, nbytes)
        torch.cuda.synchronize()
        check(fx, want, (what, fl), pick=fl == 0)
    p.unchanged()
    d.unchanged()
    return want


# ---- sizes and shapes ----------------------------------------------------------------------------------------------------------

@HASHES
def test_no_record_no_key_and_one(hip, weak):
    d = Dictionary(hip, [b"a\n", b"b\n", b"a"], weak)
    want = lookup(hip, d, [], "R = 0")
    assert len(want[0]) == len(want[1]) == len(want[2]) == 0 and want[3] == 0
    lookup(hip, d, None, "R = 0, off[0] = 7", packed=(np.array([7], np.uint64), np.zeros(0, np.uint8)))
    none = Dictionary(hip, [], weak)                        # a dictionary of no record: D = 0, no table at all
    assert none.dx.count == 0 and none.dx.records == 0
    want = lookup(hip, none, [b"a\n", b"", b"b"] * 30, "D = 0")
    assert (want[0] == NONE).all() and want[3] == 0 and want[2].tolist() == list(range(90)) and want[1].tolist() == [0, 0]
    lookup(hip, none, [], "D = 0, R = 0")
    for key in (b"", b"x", b"0123456789abcdefg"):
        one = Dictionary(hip, [key + b"\n"], weak)
        assert lookup(hip, one, [key], ("one, present", key))[0].tolist() == [0]
        assert lookup(hip, one, [key + b"y"], ("one, absent", key))[0].tolist() == [NONE]


@HASHES
def test_around_the_wavefront_and_the_block(hip, weak):
    d = Dictionary(hip, [b"no such\n", b"yes\n", b"yes", b"y"], weak)
    for R in (63, 64, 65, 255, 256, 257, 513):
        for name, there in (("alternating", np.arange(R) % 2 == 0), ("all", np.ones(R, bool)), ("none", np.zeros(R, bool))):
            want = lookup(hip, d, [b"yes\n" if t else b"no\n" for t in there], (R, name))
            assert want[3] == int(there.sum()) and np.array_equal(want[0] != NONE, there) and set(want[0].tolist()) <= {1, NONE}
            assert len(want[1]) == (R + 63) // 64


@functools.lru_cache(maxsize=None)
def many_blocks():
    """4 096 * 256 + 257 records of 0 - 2 bytes, more block pairs than one round of the scan takes, about half of them keys of the
    dictionary: (the dictionary's records, off, bytes, the judge's answer), computed once, left unchanged"""
    rng = np.random.RandomState(33)
    R = 4096 * 256 + 257
    lens = rng.randint(0, 3, R)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    data = rng.choice(np.frombuffer(b"abc", np.uint8), int(off[-1]))
    keys = [b"", b"a", b"c", b"ab", b"bb", b"ca", b"zz"]
    want = find_ref.find(find_ref.numbers_of(*pack(keys)), off, data)
    for a in (off, data) + want[:3]:
        a.setflags(write=False)
    return keys, off, data, want


@HASHES
def test_more_block_pairs_than_one_round_of_the_scan(hip, weak):
    import torch
    keys, off, data, want = many_blocks()
    assert 0.3 < want[3] / len(want[0]) < 0.7 and len(off) - 1 == 4096 * 256 + 257
    d = Dictionary(hip, keys, weak, trim=-1)
    p = Packed(off, data)
    fx = find_device(hip, d, p, -1)
    torch.cuda.synchronize()
    check(fx, want, "4 097 block pairs")
    p.unchanged()
    d.unchanged()


def test_weak_chains_wrap_and_near_misses(hip):
    """forty keys of five bytes under the weak hash: one tag, every chain starts in slot 125 of 128 and the run goes on over the wrap
    to slot 36.  Every key is probed, the one at the run's end among them; the absent probes of that length and tag differ in the
    first or in the last byte alone; absent probes of 1 and 9 bytes share tag and start, walk the whole run and end at the first
    empty slot behind the wrap; one of 6 bytes starts inside the run with another tag and ends there too"""
    rng = np.random.RandomState(44)
    keys = sorted({bytes(rng.randint(97, 123, 5).astype(np.uint8)) for _ in range(60)})[:40]
    assert len(keys) == 40 and hip.distinct_table_slots(40) == 128
    d = Dictionary(hip, keys, WEAK_HASH, trim=-1)
    probes = list(keys[::-1])
    probes += [bytes([k[0] ^ 0x01]) + k[1:] for k in keys[:8]] + [k[:4] + bytes([k[4] ^ 0x01]) for k in keys[:8]]
    probes += [b"q", b"qqqqqqqqq", b"qqqqqq", b"", keys[7], keys[7][:4]]
    want = lookup(hip, d, probes, "weak chains", trim=-1)
    assert want[0][:40].tolist() == list(range(39, -1, -1)) and want[0][-2] == 7
    assert int((want[0] == NONE).sum()) == len([pr for pr in probes if pr not in set(keys)]) >= 20


# ---- key lengths ---------------------------------------------------------------------------------------------------------------

LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 70000)


@functools.lru_cache(maxsize=None)
def length_case():
    """a key of every length, and per length the probes: the key itself, one that differs in the last byte alone, and above 256
    bytes one that differs in chunk 0 alone, in chunk 63, in chunk 64 and in the last chunk alone, where the key has them (lane 0,
    lane 63, the second stride and the masked tail of the wavefront's comparison)"""
    rng = np.random.RandomState(55)
    keys = [bytes(rng.randint(0, 256, n).astype(np.uint8)) for n in LENGTHS]
    probes, expect = [], []

    def flipped(k, at):
        return k[:at] + bytes([k[at] ^ 0x20]) + k[at + 1:]

    for d, k in enumerate(keys):
        n = len(k)
        probes.append(k)
        expect.append(d)
        if n == 0:
            continue
        ats = [n - 1]
        if n > 256:
            nch = (n + 15) // 16
            ats += [0, 15] + [16 * c for c in (63, 64) if c < nch] + [16 * (nch - 1)]
        for at in ats:
            probes.append(flipped(k, at))
            expect.append(NONE)
    return keys, probes, expect


@HASHES
def test_key_lengths_and_where_long_keys_differ(hip, weak):
    keys, probes, expect = length_case()
    assert hip.distinct_long_bytes() == 256
    d = Dictionary(hip, keys, weak, trim=-1)
    want = lookup(hip, d, probes, "lengths", trim=-1)
    assert want[0].tolist() == expect and want[3] == len(LENGTHS)
    # the probe text in another order and at another alignment: the same classes
    order = np.random.RandomState(56).permutation(len(probes))
    want = lookup(hip, d, [probes[i] for i in order], "lengths, shuffled", trim=-1, shift=5, flags=(0,))
    assert want[0].tolist() == [expect[i] for i in order]


# ---- trim, tags ----------------------------------------------------------------------------------------------------------------

@HASHES
def test_each_side_trims_for_itself(hip, weak):
    d = Dictionary(hip, [b"a", b"bb\n", b"\n"], weak)
    assert lookup(hip, d, [b"a\n", b"a", b"bb", b"bb\n\n", b"", b"\n", b"c\n"], "trim")[0].tolist() == [0, 0, 1, NONE, 2, 2, NONE]
    assert lookup(hip, d, [b"a\n", b"a", b"bb\n", b"bb", b"\n", b""], "no trim", trim=-1)[0].tolist() == [NONE, 0, NONE, 1, NONE, 2]
    d = Dictionary(hip, [b"a;", b"b\n", b"c;;"], weak, trim=ord(";"))
    assert lookup(hip, d, [b"a\n", b"a;", b"b\n\n", b"b\n", b"c;\n", b"c;"], "two trim bytes")[0].tolist() == [0, NONE, 1, NONE, 2, 2]
    d = Dictionary(hip, [b"\x00", b"x\x00\x00"], weak, trim=0)
    assert lookup(hip, d, [b"", b"\x00", b"x\x00", b"x\x00\x00"], "the trim byte 0", trim=0)[0].tolist() == [0, 0, NONE, 1]


@HASHES
def test_tags(hip, weak):
    d = Dictionary(hip, [b"x\n", b"x", b"y", b"x", b""], weak, tag=[1, 2, 0, 1, 0xFFFFFFFF])
    want = lookup(hip, d, [b"x", b"x\n", b"x", b"y", b"y\n", b"", b"\n", b"x"], "tags", tag=[2, 1, 3, 0, 1, 0xFFFFFFFF, 0, 0])
    assert want[0].tolist() == [1, 0, NONE, 2, NONE, 3, NONE, NONE]          # equal bytes under another tag are absent
    assert lookup(hip, d, [b"x", b"y", b""], "no probe tags")[0].tolist() == [NONE, 2, NONE]   # a NULL tag array finds only keys of tag 0
    d = Dictionary(hip, [b"x", b"y"], weak)                                  # ... on either side
    assert lookup(hip, d, [b"x", b"y\n", b"x"], "no dictionary tags", tag=[0, 0, 5])[0].tolist() == [0, 1, NONE]
    rng = np.random.RandomState(3)
    recs = [bytes(rng.choice(list(b"ab"), rng.randint(0, 4)).astype(np.uint8)) for _ in range(3000)]
    d = Dictionary(hip, recs[:40], weak, tag=rng.randint(0, 3, 40))
    lookup(hip, d, recs, "random tags", tag=rng.randint(0, 3, 3000), flags=(0,))


# ---- the ends of the buffers ---------------------------------------------------------------------------------------------------

def edge_records():
    rng = np.random.RandomState(5)
    recs = []
    for n in (15, 16, 17, 31, 32, 33):
        a = bytes(rng.randint(97, 123, n).astype(np.uint8))
        recs += [a, a[:-1] + bytes([a[-1] ^ 0x01]) + b"\n", a + b"\n", a[:-1]]
    return recs + [b"tail-of-the-buffer-17"]


@HASHES
def test_both_texts_end_with_their_allocation_and_offsets_are_clamped(hip, weak):
    recs = edge_records()
    keys = recs[0:24:4] + [recs[-1]]
    for shift in (0, 1, 15):
        d = Dictionary(hip, keys, weak, shift=shift, exact=True)
        want = lookup(hip, d, recs, ("exact", shift), shift=shift, exact=True)
        assert want[3] == 13 and want[0][-1] == len(keys) - 1
    # nbytes below off[R], on either side: the last records are clipped, and the bytes behind the limit are no key's
    off, data = pack(recs)
    total = int(off[-1])
    for shift in (0, 1, 15):
        for cut in (1, 17, 40):
            d = Dictionary(hip, None, weak, shift=shift, exact=True, nbytes=total - cut, packed=(off, data[:total - cut]))
            lookup(hip, d, None, ("clipped", shift, cut), shift=shift, exact=True, nbytes=total - cut, packed=(off, data[:total - cut]), flags=(0,))
            want = lookup(hip, d, recs, ("clipped dictionary", shift, cut), flags=(0,))
            assert want[3] < len(recs)
    # an off that decreases, and an off[R] below nbytes
    data = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789", np.uint8)
    d = Dictionary(hip, [b"ab", b"cdefghi", b"", b"abcd"], weak, trim=-1)
    off = np.array([0, 4, 2, 9, 20, 30, 36, 36, 500], np.uint64)
    for nbytes in (36, 33, 3, 0):
        lookup(hip, d, None, ("clamp", nbytes), trim=-1, nbytes=nbytes, packed=(off, data), flags=(0,))
    assert lookup(hip, d, None, "limit off[R]", trim=-1, packed=(np.array([0, 4, 8, 2], np.uint64), data), flags=(0,))[0].tolist() == [0, 2, 2]


# ---- properties -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def property_case():
    rng = np.random.RandomState(21)
    recs = [bytes(rng.choice(list(b"abc"), rng.randint(0, 7)).astype(np.uint8)) + (b"\n" if rng.randint(2) else b"") for _ in range(20000)]
    off, data = pack(recs)
    want = distinct_ref.distinct(off, data, NL, None, NL)
    for a in (off, data) + want:
        a.setflags(write=False)
    return off, data, want


@HASHES
def test_the_dictionary_finds_its_own_source_and_its_own_keys(hip, weak):
    off, data, dw = property_case()
    R, D = len(off) - 1, len(dw[0])
    d = Dictionary(hip, None, weak, packed=(off, data))
    want = lookup(hip, d, None, "self", packed=(off, data), flags=(0,))
    assert np.array_equal(want[0], dw[2]) and want[3] == R and want[2].tolist() == list(range(R))
    want = lookup(hip, d, None, "keys", packed=(dw[3], dw[4]), flags=(0,))
    assert want[0].tolist() == list(range(D)) and want[3] == D
    # ... as they lie on the device
    import torch
    fx = d.dx.find_device(d.dx.off_ptr, d.dx.bytes_ptr, D, d.dx.nbytes, NL)
    torch.cuda.synchronize()
    check(fx, want, "keys on the device")
    d.unchanged()


@HASHES
def test_two_streams_and_two_runs_alike(hip, weak):
    import torch
    off, data, _ = property_case()
    d = Dictionary(hip, None, weak, packed=(off[:3001], data))
    rng = np.random.RandomState(8)
    recs = [bytes(rng.choice(list(b"abcd"), rng.randint(0, 7)).astype(np.uint8)) + b"\n" for _ in range(5000)]
    poff, pdata = pack(recs)
    p = Packed(poff, pdata)
    want = find_ref.find(d.number, poff, pdata, NL)
    assert 0.2 < want[3] / 5000 < 0.95
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    one = find_device(hip, d, p, NL, stream=s1.cuda_stream)
    two = find_device(hip, d, p, NL, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    got = [check(fx, want, ("stream", k)) for k, fx in enumerate((one, two))]
    again = find_device(hip, d, p, NL)
    torch.cuda.synchronize()
    got.append(check(again, want, "again"))
    assert all(a.tobytes() == b.tobytes() for g in got[1:] for a, b in zip(got[0], g))
    p.unchanged()
    d.unchanged()


# ---- forms ----------------------------------------------------------------------------------------------------------------------

@HASHES
def test_the_records_of_an_extraction(hip, weak):
    import torch
    starts, ends, n = "kw_starts", "kw_ends", 1500
    rows, lens = inputs_of(ends)
    pd, td = starts_image(starts), ends_image(ends)
    mt_ref = matches_ref.head(reference(starts, ends), n)
    data, off = lead_packed(rows[:n], lens[:n])
    d_data, d_off = device_u8(data), device_u64(off)
    mt = hip.HipMatches.run_device(pd, td, d_data.data_ptr(), d_off.data_ptr(), n, limit=len(data))
    d = Dictionary(hip, [b"ab\n", b"bdb\n", b"zzz\n", b"d"], weak)
    for xsep in (NL, -1):
        x_off, x_data, _, _ = extract_ref.extract(rows[:n], lens[:n], lens[:n], mt_ref, None, False, xsep)
        want = find_ref.find(d.number, x_off, x_data, xsep)
        assert len(want[0]) > 2000 and 0 < want[3] < len(want[0])
        ex = mt.extract_device(d_data.data_ptr(), d_off.data_ptr(), n, limit=len(data), sep_byte=xsep)
        for fl in (0, NO_PICK):
            fx = d.dx.find_extracted(ex, fl)
            torch.cuda.synchronize()
            check(fx, want, ("extracted", xsep, fl), pick=fl == 0)
        ex.free()
    d.unchanged()


def lines_of_three_files():
    files, blob, fo = three_files()
    recs = [x + b"\n" for ls in files for x in ls]
    recs[-1] = recs[-1][:-1]                                            # the text's last line has no delimiter
    return blob, fo, recs


@HASHES
def test_the_lines_of_hits(hip, weak):
    import torch
    blob, fo, recs = lines_of_three_files()
    text = hip.HipText(blob, NL, file_off=fo)
    ld = hip.LinesDfa(span_ref.line_matcher_of(KEYWORDS)[0], NL)
    hits = text.hits(ld)
    picked = [x for x in recs if any(k in x for k in KEYWORDS)]
    assert hits.count == len(picked) > 40
    d = Dictionary(hip, [b"d", b"cab\n", b"the last line has a d\n", b"www"], weak)
    want = find_ref.find(d.number, *pack(picked), NL)
    assert 0 < want[3] < len(picked) and want[0][-1] == 2
    fx = d.dx.find_hits(hits)
    torch.cuda.synchronize()
    check(fx, want, "hits")
    bare = text.hits(ld, want_bytes=False)                              # FSM_HIP_HITS_NO_BYTES: no lines on the device
    with pytest.raises(OSError) as ei:
        d.dx.find_hits(bare)
    assert ei.value.errno == errno.EINVAL
    d.unchanged()


@HASHES
def test_the_lines_of_a_text_select_its_hits(hip, weak):
    """grep -F -x -f on the device: the bitmap of find_text handed to fsm_hip_text_hits_device, plain and inverted"""
    import torch
    blob, fo, recs = lines_of_three_files()
    text = hip.HipText(blob, NL, file_off=fo)
    assert text.lines == len(recs)
    d = Dictionary(hip, [b"d", b"cab", b"the last line has a d", b"www", b"", b"absent"], weak)
    want = find_ref.find(d.number, *pack(recs), NL)
    assert 20 < want[3] < len(recs) - 20 and want[0][-1] == 2
    fx = d.dx.find_text(text, NO_PICK)
    bits = np.unpackbits(want[1].view(np.uint8), bitorder="little")[:len(recs)].astype(bool)
    for invert in (False, True):
        hits = text.hits_device(fx.bitmap_ptr, invert=invert)
        torch.cuda.synchronize()
        w_lines, w_off, w_out = hits_ref.hits_ref(blob, NL, bits, invert)
        assert hits.count == len(w_lines) == (len(recs) - want[3] if invert else want[3])
        assert np.array_equal(hits.lines(), w_lines) and np.array_equal(hits.offsets(), w_off) and np.array_equal(hits.bytes(), w_out)
        hits.close()
    check(fx, want, "text", pick=False)
    d.unchanged()


@HASHES
def test_class_into_the_tally_and_pick_into_a_front(hip, weak):
    import torch
    rng = np.random.RandomState(17)
    pool = [b"xx ab yy", b"d", b"nothing here", b"", b"cab", b"www", b"bdb bdb", b"xx ab yy "]
    recs = [pool[k] for k in rng.randint(0, len(pool), 700)]
    d = Dictionary(hip, [b"cab", b"nothing here", b"xx ab yy", b"unseen", b""], weak, trim=-1)
    off, data = pack(recs)
    p = Packed(off, data)
    want = find_ref.find(d.number, off, data)
    R, D, P = len(recs), 5, want[3]
    assert 100 < P < R - 100
    fx = find_device(hip, d, p, -1)
    # class as the tally's id array, one input per record, nrules = D: the absent records fall into the last column
    d_one = device_u64(np.arange(R + 1, dtype=np.uint64))
    tab = device_u64(np.full(D + 3, FILL, np.uint64))
    hip.tally_ids_device(d_one.data_ptr(), fx.class_ptr, R, R, 0, 0, D, tab.data_ptr(), 0)
    torch.cuda.synchronize()
    got = tab.cpu().numpy().view(np.uint64)
    w_count = np.bincount(np.where(want[0] == NONE, D, want[0]).astype(np.int64), minlength=D + 1)
    assert np.array_equal(got[:D + 1], w_count.astype(np.uint64)) and (got[D + 1:] == FILL).all() and w_count[3] == 0 and w_count[D] == R - P
    # pick[0 .. P) as the pick of the accept-position walk: what the judge's list gives
    auto = span_ref.line_matcher_of(KEYWORDS)
    pd = hip.PosDfa.from_flat(auto[0])
    rows, lens = span_ref.rows_of(recs)
    w_first, w_last = span_ref.accept_pos(auto, rows, lens)
    sel = want[2][:P].astype(np.int64)
    first, last = device_u64(np.full(P + 2, FILL, np.uint64)), device_u64(np.full(P + 2, FILL, np.uint64))
    pd.accept_pos_device(p.d_data.data_ptr(), p.d_off.data_ptr(), R, first.data_ptr(), last.data_ptr(), d_pick=fx.pick_ptr, m=P, limit=len(data))
    torch.cuda.synchronize()
    g_first, g_last = first.cpu().numpy().view(np.uint64), last.cpu().numpy().view(np.uint64)
    assert np.array_equal(g_first[:P], w_first[sel]) and np.array_equal(g_last[:P], w_last[sel]) and (g_first[P:] == FILL).all() and (g_last[P:] == FILL).all()
    assert (w_first[sel] != span_ref.NO_POS).any() and (w_first[sel] == span_ref.NO_POS).any()
    check(fx, want, "tally and pick")
    p.unchanged()
    d.unchanged()


@HASHES
def test_the_host_form(hip, weak):
    off, data, _ = property_case()
    d = Dictionary(hip, None, weak, packed=(off[:501], data))
    rng = np.random.RandomState(2)
    o, b = off[:4001], data
    check(d.dx.find(o, b, NL), find_ref.find(d.number, o, b, NL), "host")
    check(d.dx.find(o, b, -1, None, NO_PICK), find_ref.find(d.number, o, b, -1), "host, no trim, no pick", pick=False)
    tag = rng.randint(0, 2, 4000).astype(np.uint32)
    check(d.dx.find(o, b, NL, tag), find_ref.find(d.number, o, b, NL, tag), "host, tags")
    check(d.dx.find([0], b"", NL), find_ref.find(d.number, [0], b""), "host, R = 0")
    with pytest.raises(OSError) as ei:
        d.dx.find([0, 3, 2], b"abc", NL)                                 # a decreasing off: before any launch
    assert ei.value.errno == errno.EINVAL
    d.unchanged()


# ---- misuse ---------------------------------------------------------------------------------------------------------------------

def test_misuse_is_refused_before_any_launch(hip):
    import torch
    d = Dictionary(hip, [b"a", b"b"], 0, trim=-1)
    p = Packed(*pack([b"a", b"c"]))
    o, b = p.d_off.data_ptr(), p.d_data.data_ptr()
    for args, want in (((0, b, 2, 2), errno.EINVAL),                                   # d_off NULL
                       ((o, 0, 2, 2), errno.EINVAL),                                   # d_bytes NULL with nbytes > 0
                       ((o, b, 2, 2, 256), errno.EINVAL), ((o, b, 2, 2, -2), errno.EINVAL),
                       ((o, b, 2, 2, -1, 0, 2), errno.EINVAL), ((o, b, 2, 2, -1, 0, 0x80000000), errno.EINVAL),
                       ((o, b, 2 ** 32 - 1, 2), errno.EOVERFLOW), ((o, b, 2 ** 40, 2), errno.EOVERFLOW)):
        with pytest.raises(OSError) as ei:
            d.dx.find_device(*args)
        assert ei.value.errno == want, args
    lib = hip.load_library()
    H = C.c_void_p(d.dx.handle)
    for fn in (lib.fsm_hip_keys_find_extracted, lib.fsm_hip_keys_find_hits, lib.fsm_hip_keys_find_text):
        C.set_errno(0)
        assert not fn(H, None, 0, None) and C.get_errno() == errno.EINVAL
    C.set_errno(0)
    assert not lib.fsm_hip_keys_find_device(None, C.c_void_p(o), C.c_void_p(b), 2, 2, -1, None, 0, None) and C.get_errno() == errno.EINVAL
    fx = find_device(hip, d, p, -1, NO_PICK)
    torch.cuda.synchronize()
    assert fx.pick_ptr == 0 and fx.present == 1
    pick = np.zeros(4, np.uint64)
    C.set_errno(0)
    assert lib.fsm_hip_found_copy(C.c_void_p(fx.handle), None, None, pick.ctypes.data_as(C.c_void_p)) == -1 and C.get_errno() == errno.EINVAL
    C.set_errno(0)
    assert lib.fsm_hip_found_pass_ms(C.c_void_p(fx.handle), 4) == -1.0 and C.get_errno() == errno.EINVAL
    fx.free()
    assert lookup(hip, d, [b"a", b"c", b"b"], "after misuse", trim=-1)[0].tolist() == [0, NONE, 1]


# ---- the example ----------------------------------------------------------------------------------------------------------------

def test_example_prints_what_grep_fxf_prints(hip, tmp_path):
    """examples/hipfgrep.c over three small files, the last without a final newline: the lines that equal a line of LIST; -v the
    others, -c their number per file, -n with their line numbers"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files, _, _ = three_files()
    names = []
    for j, ls in enumerate(files):
        data = b"".join(x + b"\n" for x in ls)
        path = tmp_path / ("f%d.txt" % j)
        path.write_bytes(data[:-1] if j == 2 else data)
        names.append(str(path))
    wanted = [b"d", b"cab", b"the last line has a d", b"", b"absent"]
    lst = tmp_path / "list.txt"
    lst.write_bytes(b"".join(x + b"\n" for x in wanted))
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    exe = str(tmp_path / "hipfgrep")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "hipfgrep.c"),
                           "-o", exe, "-L" + os.path.join(root, "libfsm_amd"), "-lfsm_hip", "-Wl,-rpath," + os.path.join(root, "libfsm_amd")])

    def run(*args, fs=names, lst=str(lst)):
        r = subprocess.run([exe, "-f", lst, *args, *fs], capture_output=True, env=env, timeout=120)
        return r.returncode, r.stdout

    def grep(invert=False, count=False, number=False):
        """grep -Fxf LIST: a line is printed iff (it is in LIST) != invert, behind its file's name"""
        sel = [[(i, x) for i, x in enumerate(ls) if (x in wanted) != invert] for ls in files]
        if count:
            return b"".join(b"%s:%d\n" % (nm.encode(), len(s)) for nm, s in zip(names, sel))
        return b"".join(b"%s:%s%s\n" % (nm.encode(), b"%d:" % (i + 1) if number else b"", x) for nm, s in zip(names, sel) for i, x in s)

    want = grep()
    assert want.count(b"\n") > 20 and want.endswith(b":the last line has a d\n")
    assert run() == (0, want)
    assert run("-v") == (0, grep(invert=True)) and grep(invert=True).count(b"\n") > 20
    assert run("-c") == (0, grep(count=True)) and run("-v", "-c") == (0, grep(invert=True, count=True))
    assert run("-n") == (0, grep(number=True)) and run("-n", "-v") == (0, grep(invert=True, number=True))
    quiet = tmp_path / "none.txt"
    quiet.write_bytes(b"xyz\nwwww\n")
    assert run(fs=[str(quiet)]) == (1, b"")
