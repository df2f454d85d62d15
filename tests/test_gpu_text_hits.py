"""GPU: the hits of the text front (libfsm_amd/csrc/text.hip: hits_count, hits_scan, hits_emit, hits_gather): the lines a
bitmap selects -- numbers, output offsets and bytes, packed on the device.

Everything is compared with hits_ref.hits_ref (the selection rule stated in numpy over text_ref.split_ref), never with
anything derived from the code under test; the end-to-end cases with the oracle walking every line WITHOUT its delimiter over
the ORIGINAL description."""
import errno
import os
import subprocess

import numpy as np
import pytest

from common import GOLDEN, Golden
from hits_ref import hits_ref, pack_bits
from text_ref import lines_of, newline_dfa, oracle_answers, split_ref

pytestmark = pytest.mark.gpu

SCAN_ROUND = 4096     # blocks of lines the pair scan takes per round (text.hip: 1 024 threads x HITS_SCAN_PER)


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()   # raises if the HIP extension is missing: no silent fallback
    return libfsm_amd


def to_device(buf, lead=0, pad=0, fill=0):
    """a device copy of buf at `lead` bytes into an allocation, `pad` bytes of `fill` on both sides: (tensor, address of the text)"""
    import torch
    host = np.full(lead + pad + len(buf) + pad + 1, fill, np.uint8)
    host[lead + pad:lead + pad + len(buf)] = buf
    t = torch.from_numpy(host).cuda()
    return t, t.data_ptr() + lead + pad


def build_text(tl, delim, rng, trailing=True):
    """a text whose line k has tl[k] >= 1 bytes, its delimiter included; without `trailing` the last line (tl[-1] >= 2) loses it"""
    tl = np.asarray(tl, np.int64)
    assert (tl >= 1).all()
    alphabet = np.array([b for b in range(1, 256) if b != delim and b != 0x0A], np.uint8) if delim else np.arange(1, 256, dtype=np.uint8)
    text = alphabet[rng.randint(0, len(alphabet), int(tl.sum()))]
    if len(tl):
        text[np.cumsum(tl) - 1] = delim
        if not trailing:
            assert tl[-1] >= 2
            text = text[:-1]
    return np.ascontiguousarray(text)


def device_bitmap(bits, garbage=0):
    import torch
    words = pack_bits(bits, garbage)
    return torch.from_numpy(words.view(np.int64).copy()).cuda() if len(words) else torch.zeros(1, dtype=torch.int64, device="cuda")


def check(h, want, want_bytes=True, what=None):
    lines, out_off, out = want
    assert h.count == len(lines), what
    assert np.array_equal(h.lines(), lines), what
    if want_bytes:
        assert h.nbytes == len(out), what
        assert np.array_equal(h.offsets(), out_off), what
        assert np.array_equal(h.bytes(), out), what
    else:
        assert h.nbytes == 0 and h.offsets_device == 0 and h.bytes_device == 0, what
    h.close()


def select_sizes(hip):
    L, W = hip.text_hits_block_lines(), hip.text_max_workgroups()
    assert L >= 64 and W >= 1
    return [0, 1, 63, 64, 65, L - 1, L, L + 1, 2 * L + 5, (W + 1) * L + 17]


SELECT_IDS = ["0", "1", "63", "64", "65", "L-1", "L", "L+1", "2L+5", "(W+1)L+17"]


def patterns(n, rng):
    first, last = np.zeros(n, bool), np.zeros(n, bool)
    first[:1] = True
    last[-1:] = True
    return [("none", np.zeros(n, bool)), ("all", np.ones(n, bool)), ("first", first), ("last", last), ("alternating", np.arange(n) % 2 == 0),
            ("rand8", rng.randint(0, 8, n) == 0), ("rand200", rng.randint(0, 200, n) == 0)]


def short_lines_text(n, delim, trailing, rng):
    """n lines of 0..2 bytes; without `trailing` the last one has a byte, so that cutting its delimiter keeps the line"""
    tl = rng.randint(1, 4, n)
    if n and not trailing:
        tl[-1] = max(int(tl[-1]), 2)
    return build_text(tl, delim, rng, trailing)


@pytest.mark.parametrize("trailing", [True, False], ids=["trailing", "no_trailing"])
@pytest.mark.parametrize("delim", [0x0A, 0x00], ids=["0x0a", "0x00"])
@pytest.mark.parametrize("si", range(len(SELECT_IDS)), ids=SELECT_IDS)
def test_select_matches_reference(hip, si, delim, trailing):
    n = select_sizes(hip)[si]
    rng = np.random.RandomState(100 * si + delim + 7 * trailing)
    text = short_lines_text(n, delim, trailing, rng)
    ht = hip.HipText(text, delim)
    assert ht.lines == n == len(split_ref(text, delim)) - 1
    for name, bits in patterns(n, rng):
        for invert in (False, True):
            want = hits_ref(text, delim, bits, invert)
            for garbage in (0, 1):
                bm = device_bitmap(bits, garbage)
                for want_bytes in (True, False):
                    h = ht.hits_device(bm.data_ptr(), invert=invert, want_bytes=want_bytes)
                    check(h, want, want_bytes, (name, invert, garbage, want_bytes))
    ht.close()


def test_select_pair_scan_takes_a_third_round(hip):
    """more blocks of lines than two rounds of the pair scan hold: the carry from round to round"""
    L = hip.text_hits_block_lines()
    n = 2 * SCAN_ROUND * L + 3
    rng = np.random.RandomState(5)
    tl = rng.randint(1, 3, n)
    text = build_text(tl, 0x0A, rng)
    bits = rng.randint(0, 8, n) == 0
    bits[-1] = True
    ht = hip.HipText(text, 0x0A)
    assert ht.lines == n
    bm = device_bitmap(bits, 1)
    check(ht.hits_device(bm.data_ptr()), hits_ref(text, 0x0A, bits))
    ht.close()


@pytest.mark.parametrize("lo,hi,n", [(0, 3, 20000), (8, 64, 20000), (0, 1024, 4000)], ids=["0-3", "8-64", "0-1024"])
def test_gather_line_lengths(hip, lo, hi, n):
    """one line in 3 selected: chunks that cross 0, 1 and several boundaries, sources on every alignment mod 16"""
    rng = np.random.RandomState(hi)
    for trailing in (True, False):
        tl = rng.randint(lo, hi + 1, n) + 1
        tl[-1] = max(int(tl[-1]), 2)
        text = build_text(tl, 0x0A, rng, trailing)
        bits = rng.randint(0, 3, n) == 0
        bits[-1] = True
        want = hits_ref(text, 0x0A, bits)
        assert len(set((split_ref(text, 0x0A)[:-1][bits] % 16).tolist())) == 16
        ht = hip.HipText(text, 0x0A)
        bm = device_bitmap(bits)
        check(ht.hits_device(bm.data_ptr()), want, what=trailing)
        check(ht.hits_device(bm.data_ptr(), invert=True), hits_ref(text, 0x0A, bits, True), what=trailing)
        ht.close()


def test_gather_one_long_line_spans_blocks(hip):
    GB = hip.text_hits_block_bytes()
    rng = np.random.RandomState(11)
    tl = np.concatenate([rng.randint(1, 40, 300), [100000], rng.randint(1, 40, 300)])
    assert 100000 > 5 * GB
    text = build_text(tl, 0x0A, rng)
    bits = np.zeros(len(tl), bool)
    bits[300] = True
    ht = hip.HipText(text, 0x0A)
    bm = device_bitmap(bits)
    want = hits_ref(text, 0x0A, bits)
    assert len(want[2]) == 100000
    check(ht.hits_device(bm.data_ptr()), want)
    bits[[3, 299, 301, 599]] = True      # short selected neighbours on both sides of it
    bm = device_bitmap(bits)
    check(ht.hits_device(bm.data_ptr()), hits_ref(text, 0x0A, bits))
    ht.close()


def exact_output_sizes(hip):
    GB, W = hip.text_hits_block_bytes(), hip.text_max_workgroups()
    return [GB - 1, GB, GB + 1, (W + 1) * GB + 17]


@pytest.mark.parametrize("ti", range(4), ids=["GB-1", "GB", "GB+1", "(W+1)GB+17"])
def test_gather_exact_output_sizes(hip, ti):
    """selected lines of 997 bytes and one that fills the rest, unselected 5-byte lines between them: the output is exactly T bytes"""
    T = exact_output_sizes(hip)[ti]
    rng = np.random.RandomState(ti)
    sel_len = [997] * (T // 997) + ([T % 997] if T % 997 else [])
    tl = np.full(2 * len(sel_len) + 1, 5, np.int64)
    tl[1::2] = sel_len
    bits = np.zeros(len(tl), bool)
    bits[1::2] = True
    text = build_text(tl, 0x0A, rng)
    want = hits_ref(text, 0x0A, bits)
    assert len(want[2]) == T
    ht = hip.HipText(text, 0x0A)
    bm = device_bitmap(bits)
    check(ht.hits_device(bm.data_ptr()), want)
    ht.close()


@pytest.mark.parametrize("lead", [1, 3, 13])
def test_gather_reads_no_neighbour(hip, lead):
    """a text 1, 3, 13 bytes into an allocation with 64 delimiter bytes before and after it: the output holds none of them"""
    rng = np.random.RandomState(lead)
    for trailing in (True, False):
        tl = rng.randint(1, 50, 3000)
        tl[-1] = max(int(tl[-1]), 2)
        text = build_text(tl, 0x0A, rng, trailing)
        dev, addr = to_device(text, lead=lead, pad=64, fill=0x0A)
        ht = hip.HipText(d_text=addr, nbytes=len(text), delim=0x0A)
        assert ht.lines == len(tl)
        for bits in (np.ones(len(tl), bool), rng.randint(0, 3, len(tl)) == 0):
            bits[[0, -1]] = True
            bm = device_bitmap(bits)
            check(ht.hits_device(bm.data_ptr()), hits_ref(text, 0x0A, bits), what=trailing)
        ht.close()
        del dev


def test_gather_only_the_last_line_without_delimiter(hip):
    rng = np.random.RandomState(3)
    for last in (2, 17, 5001):       # the line's bytes + the delimiter it loses
        tl = np.concatenate([rng.randint(1, 30, 500), [last]])
        text = build_text(tl, 0x0A, rng, trailing=False)
        bits = np.zeros(len(tl), bool)
        bits[-1] = True
        want = hits_ref(text, 0x0A, bits)
        assert len(want[2]) == last - 1 and want[2][-1] != 0x0A
        ht = hip.HipText(text, 0x0A)
        bm = device_bitmap(bits, 1)
        check(ht.hits_device(bm.data_ptr()), want)
        ht.close()


# ---- end to end: the walk's bitmap selects -------------------------------------------------------------------

NLINES = 20000


def make_text(hip, flat, seeds, alphabet, plant, trailing, delim=0x0A):
    """about NLINES lines of 0..300 bytes from the project's generator (alphabet without the delimiter), a tenth of them empty,
    every fifth one of `seeds` (strings the automaton has answers of its own for); joined by the delimiter"""
    rng = np.random.RandomState(len(seeds) + flat.nstates)
    rows = hip.gen_inputs_host(NLINES, 304, 0, 99, alphabet, plant, 3)
    lens = rng.randint(0, 301, NLINES).astype(np.int64)
    lens[rng.randint(0, 10, NLINES) == 0] = 0
    lens[-1] = max(int(lens[-1]), 7)                       # the last line has bytes: cutting its delimiter keeps the line
    if seeds:
        for i in range(0, NLINES, 5):
            s = seeds[(i // 5) % len(seeds)]
            rows[i, :len(s)] = np.frombuffer(s, np.uint8)
            lens[i] = len(s)
    assert not (rows[np.arange(304)[None, :] < lens[:, None]] == delim).any()
    ext = np.concatenate([rows, np.zeros((NLINES, 1), np.uint8)], axis=1)
    ext[np.arange(NLINES), lens] = delim
    text = ext[np.arange(305)[None, :] <= lens[:, None]]
    if not trailing:
        text = text[:-1]                                   # the last line loses its delimiter
    return np.ascontiguousarray(text)


def automata(hip):
    from libfsm_amd import FlatDfa
    c1 = Golden(os.path.join(GOLDEN, "c1.npz"))
    det = Golden(os.path.join(GOLDEN, "endids_union_det.npz"))
    z = np.load(os.path.join(GOLDEN, "bench", "eager40.npz"))
    words = bytes(z["patterns"]).split(b"\n")
    lower = b"abcdefghijklmnopqrstuvwxyz"
    return {
        "c1": (c1.flat, [b"Libfsm", b"libffsmsm", b"xLibf"], b"Libfsm xyz", b"Libfsm"),
        "endids_union_det": (det.flat, det.strings(), b"abcdefox_XYZ", b"abc_def"),
        "eager40": (FlatDfa.load(z), words[:12], lower, words[0]),
        "newline": (newline_dfa(), [b"a", b"aa", b"ab", b"b", b"aaa"], b"ab", b"a"),
    }


@pytest.mark.parametrize("trailing", [True, False], ids=["trailing", "no_trailing"])
@pytest.mark.parametrize("name", ["c1", "endids_union_det", "eager40", "newline"])
def test_hits_of_the_walk(hip, name, trailing):
    import torch
    flat, seeds, alphabet, plant = automata(hip)[name]
    text = make_text(hip, flat, seeds, alphabet, plant, trailing)
    lines = lines_of(text, 0x0A)
    ret = oracle_answers(flat, lines)[0]
    n = len(lines)
    bits = ret == 1
    assert n == NLINES and (text[-1] == 0x0A) == trailing
    ld, ht = hip.LinesDfa(flat, 0x0A), hip.HipText(text, 0x0A)
    assert ht.lines == n
    for invert in (False, True):
        want = hits_ref(text, 0x0A, bits, invert)
        h = ht.hits(ld, invert=invert)
        assert 0 < h.count < n
        check(h, want, what=invert)
        check(ht.hits(ld, invert=invert, want_bytes=False), want, False, what=invert)
    # the device form on a caller's stream, over the bitmap of exec_device on the same stream: what the host form gives
    host = ht.hits(ld)
    want = (host.lines(), host.offsets(), host.bytes())
    host.close()
    s = torch.cuda.Stream()
    d_bm = torch.full(((n + 63) // 64,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ht.exec_device(ld, d_bitmap=d_bm.data_ptr(), stream=s.cuda_stream)
    h = ht.hits_device(d_bm.data_ptr(), stream=s.cuda_stream)
    assert h.lines_device and h.offsets_device and h.bytes_device
    check(h, want)
    # a text opened over the caller's bytes on that stream, its hits on the same stream
    dev, addr = to_device(text, lead=5, pad=64, fill=0x0A)
    ht2 = hip.HipText(d_text=addr, nbytes=len(text), delim=0x0A, stream=s.cuda_stream)
    ht2.exec_device(ld, d_bitmap=d_bm.data_ptr(), stream=s.cuda_stream)
    check(ht2.hits_device(d_bm.data_ptr(), stream=s.cuda_stream), want)
    ht2.close()
    ht.close()


def test_misuse_and_edge_cases(hip):
    flat = newline_dfa()
    ld = hip.LinesDfa(flat, 0x0A)
    # n == 0: a handle with out_off == [0], both forms, with and without the bytes
    for empty in (hip.HipText(b"", 0x0A), hip.HipText(d_text=0, nbytes=0, delim=0x0A)):
        for h in (empty.hits(ld), empty.hits(ld, invert=True), empty.hits_device(0), empty.hits_device(0, invert=True)):
            assert h.count == 0 and h.nbytes == 0 and h.lines().tolist() == [] and h.offsets().tolist() == [0] and h.bytes().tolist() == []
            h.close()
        h = empty.hits_device(0, want_bytes=False)
        assert h.count == 0 and h.nbytes == 0 and h.offsets_device == 0
        h.close()
    # m == 0 with n > 0
    text = b"a\naa\nab\n\nb\na"
    ht = hip.HipText(text, 0x0A)
    n = ht.lines
    assert n == 6
    for bits, invert in ((np.zeros(n, bool), False), (np.ones(n, bool), True)):
        for garbage in (0, 1):
            bm = device_bitmap(bits, garbage)
            h = ht.hits_device(bm.data_ptr(), invert=invert)
            assert h.count == 0 and h.nbytes == 0 and h.offsets().tolist() == [0] and h.lines().tolist() == [] and h.bytes().tolist() == []
            h.close()
    # the host form on it: the oracle's lines
    ret = oracle_answers(flat, lines_of(np.frombuffer(text, np.uint8), 0x0A))[0]
    assert 0 < int((ret == 1).sum()) < n
    check(ht.hits(ld), hits_ref(text, 0x0A, ret == 1))
    # NO_BYTES: the numbers alone, and no offsets to copy
    h = ht.hits(ld, want_bytes=False)
    assert h.count == int((ret == 1).sum()) and h.nbytes == 0 and h.offsets_device == 0 and h.bytes_device == 0
    with pytest.raises(OSError) as ei:
        h.offsets()
    assert ei.value.errno == errno.EINVAL
    h.close()
    # an unknown flag bit, a NULL bitmap with lines, a matcher for another delimiter: EINVAL
    bm = device_bitmap(np.ones(n, bool))
    for flags in (4, 0x80000000, 1 | 8):
        with pytest.raises(OSError) as ei:
            ht.hits_device(bm.data_ptr(), flags=flags)
        assert ei.value.errno == errno.EINVAL
    with pytest.raises(OSError) as ei:
        ht.hits_device(0)
    assert ei.value.errno == errno.EINVAL
    with pytest.raises(OSError) as ei:
        ht.hits(hip.LinesDfa(flat, 0x00))
    assert ei.value.errno == errno.EINVAL
    ht.close()


def test_example_prints_the_matching_lines(hip, tmp_path):
    """examples/hipgrep_print.c on the table and the data of test_gpu_text.py's example test (empty lines, no final newline)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    det = Golden(os.path.join(GOLDEN, "endids_union_det.npz"))
    table = str(tmp_path / "t.fsmhip")
    det.flat.write_c(table)
    rng = np.random.RandomState(8)
    lines = list(det.strings()) + [b"", b"", b"abc", b"zzz", b"foo", b""]
    lines += [bytes(rng.choice(list(b"abcdefor_X"), rng.randint(0, 12)).astype(np.uint8)) for _ in range(400)] + [b"bar"]
    data = b"\n".join(lines)
    assert b"\n\n" in data and not data.endswith(b"\n")
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    exe = str(tmp_path / "hipgrep_print")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "hipgrep_print.c"), "-o", exe,
                           "-L" + os.path.join(root, "libfsm_amd"), "-lfsm_hip", "-Wl,-rpath," + os.path.join(root, "libfsm_amd")])
    ret = oracle_answers(det.flat, lines)[0]
    ranges = [l + b"\n" for l in lines[:-1]] + [lines[-1]]     # every line with its delimiter; the last one has none
    acc = [i for i in range(len(lines)) if ret[i] == 1]
    rej = [i for i in range(len(lines)) if ret[i] != 1]
    assert len(acc) >= 10 and len(rej) >= 10

    def run(*opts, stdin=data):
        r = subprocess.run([exe, *opts, table], input=stdin, capture_output=True, env=env, timeout=120)
        return r.returncode, r.stdout

    assert run() == (0, b"".join(ranges[i] for i in acc))
    assert run("-v") == (0, b"".join(ranges[i] for i in rej))
    assert run("-c") == (0, b"%d\n" % len(acc))
    assert run("-v", "-c") == (0, b"%d\n" % len(rej))
    assert run("-n") == (0, b"".join(b"%d:" % (i + 1) + ranges[i] for i in acc))
    assert run("-n", "-v") == (0, b"".join(b"%d:" % (i + 1) + ranges[i] for i in rej))
    assert run("-c", stdin=b"") == (1, b"0\n")                 # nothing selected: grep's 1
    assert run(stdin=ranges[rej[0]]) == (1, b"")
    assert run("-x")[0] == 2                                   # an error: grep's 2
