"""GPU: files of a text (libfsm_amd/csrc/text.hip: files_mark, files_scan, files_merge, hits_file_first): many files back to
back in one text, lines cut at every file end as well, hits per file.

The offsets and file_lines are compared bit for bit with files_ref.files_ref (the rule stated in numpy), never with anything
derived from the code under test; the walk with the per-file texts of fsm_hip_text_open (the existing code as the yardstick) and
with the oracle walking every line WITHOUT its delimiter; the hits with files_ref.hits_ref_off over the union offsets."""
import errno
import os
import subprocess

import numpy as np
import pytest

from common import GOLDEN, Golden
from files_ref import files_ref, hits_ref_off, join_files
from hits_ref import pack_bits
from line_inputs import device_u64
from text_ref import lines_of, newline_dfa, oracle_answers, split_ref

pytestmark = pytest.mark.gpu

NO, NO_ID = 0xFFFFFFFF, 0xFFFFFFFE


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


def random_text(nbytes, delim, density, rng):
    """one byte in `density` is the delimiter (0: none at all); the others are anything else"""
    other = np.array([b for b in range(256) if b != delim], np.uint8)
    text = other[rng.randint(0, 255, nbytes)]
    if density:
        text[rng.randint(0, density, nbytes) == 0] = delim
    return text


def random_ends(text, delim, nfiles, B, rng):
    """nfiles + 1 ends: 0 and nbytes repeated, ends at every scan-block edge - 1 / 0 / + 1, ends exactly on a delimiter and just
    after one, random ends with repeats -- as many of each kind as nfiles has room for"""
    nbytes = len(text)
    if nfiles == 1:
        return np.array([0, nbytes], np.uint64)
    edges = np.concatenate([k * B + np.array([-1, 0, 1]) for k in range(1, nbytes // B + 1)])
    at = np.flatnonzero(text == delim)
    on = np.concatenate([at[:8], at[-8:], at[:8] + 1, at[-8:] + 1]) if len(at) else np.zeros(0, np.int64)
    special = np.concatenate([[0, nbytes], edges, on]).astype(np.int64)
    special = special[(special >= 0) & (special <= nbytes)]
    inner = nfiles - 1
    take = special if len(special) <= inner // 2 else rng.choice(special, max(inner // 2, 1), replace=False)
    rest = inner - len(take)
    rand = rng.randint(0, nbytes + 1, rest - rest // 4)
    mid = np.concatenate([take, rand, rng.choice(np.concatenate([take, rand]), rest // 4)])   # repeats of what is there
    assert len(mid) == inner
    return np.sort(np.concatenate([[0], mid, [nbytes]])).astype(np.uint64)


def check_text(ht, text, delim, fo, what=None):
    off, fl = files_ref(text, delim, fo)
    assert ht.files == len(fo) - 1, what
    assert ht.lines == len(off) - 1, what
    assert np.array_equal(ht.offsets(), off), what
    assert np.array_equal(ht.file_lines(), fl), what
    assert ht.file_lines_ptr != 0, what
    return off, fl


@pytest.mark.parametrize("nfiles", [1, 2, 7, 500])
@pytest.mark.parametrize("density", [2, 40, 0])
@pytest.mark.parametrize("delim", [0x0A, 0x00], ids=["0x0a", "0x00"])
def test_random_texts(hip, delim, density, nfiles):
    B = hip.text_block_bytes()
    nbytes = 3 * B + 5
    for seed in range(3):
        rng = np.random.RandomState(1000 * seed + 10 * nfiles + density + delim)
        text = random_text(nbytes, delim, density, rng)
        fo = random_ends(text, delim, nfiles, B, rng)
        ht = hip.HipText(text, delim, file_off=fo)
        off, fl = check_text(ht, text, delim, fo, (seed, fo))
        if density == 0:     # no delimiter at all: every non-empty file is one line
            assert len(off) - 1 == len(np.unique(fo)) - 1
        ht.close()
    if nfiles == 500:
        assert (np.diff(fo.astype(np.int64)) == 0).any() and {B - 1, B, B + 1, 3 * B - 1, 3 * B, 3 * B + 1} <= set(fo.tolist())
        if density:
            at = np.flatnonzero(text == delim)
            assert at[0] in fo and at[0] + 1 in fo


def test_files_scan_takes_a_third_round(hip):
    """more file ends than two rounds of files_scan hold: the carry from round to round"""
    FB = hip.text_files_block()
    nfiles = 2 * FB + 3
    rng = np.random.RandomState(9)
    fo = np.concatenate([[0], np.cumsum(rng.randint(0, 3, nfiles))]).astype(np.uint64)
    text = random_text(int(fo[-1]), 0x0A, 3, rng)
    ht = hip.HipText(text, 0x0A, file_off=fo)
    off, fl = check_text(ht, text, 0x0A, fo)
    assert len(off) - 1 > len(split_ref(text, 0x0A)) - 1 + FB // 8      # added ends in every round
    ht.close()


def test_one_file_equals_a_plain_text(hip):
    rng = np.random.RandomState(2)
    for trailing in (True, False):
        text = random_text(40000, 0x0A, 30, rng)
        text[-1] = 0x0A if trailing else 0x41
        plain = hip.HipText(text, 0x0A)
        ht = hip.HipText(text, 0x0A, file_off=[0, len(text)])
        assert np.array_equal(ht.offsets(), plain.offsets()) and np.array_equal(plain.offsets(), split_ref(text, 0x0A))
        assert ht.files == 1 and ht.file_lines().tolist() == [0, plain.lines]
        # on a plain text: no files, NULL from the device accessors, EINVAL from the copies
        assert plain.files == 0 and plain.file_lines_ptr == 0
        with pytest.raises(OSError) as ei:
            plain.file_lines()
        assert ei.value.errno == errno.EINVAL
        bm = device_u64(pack_bits(np.ones(plain.lines, bool)))
        h = plain.hits_device(bm.data_ptr())
        assert h.file_first_ptr == 0
        with pytest.raises(OSError) as ei:
            h.file_first()
        assert ei.value.errno == errno.EINVAL
        h.close()
        plain.close()
        ht.close()
    # no byte at all: files that are all empty
    for fo in ([0, 0], [0, 0, 0, 0]):
        ht = hip.HipText(b"", 0x0A, file_off=fo)
        assert ht.lines == 0 and ht.offsets().tolist() == [0] and ht.file_lines().tolist() == [0] * len(fo)
        h = ht.hits_device(0)
        assert h.count == 0 and h.file_first().tolist() == [0] * len(fo)
        h.close()
        ht.close()


# ---- the walk ------------------------------------------------------------------------------------------------

def parity_files(name):
    """(flat, five files): two lack their final delimiter, one is empty, each of the two is followed by a file with bytes"""
    rng = np.random.RandomState(4)
    if name == "newline":
        flat, seeds, alphabet = newline_dfa(), [b"a", b"aa", b"ab", b"b", b"aaa", b""], b"ab"
    else:
        det = Golden(os.path.join(GOLDEN, "endids_union_det.npz"))
        flat, seeds, alphabet = det.flat, list(det.strings()) + [b""], b"abcdefox_XYZ"

    def some_lines(k):
        out = []
        for i in range(k):
            out.append(seeds[rng.randint(len(seeds))] if i % 2 == 0 else bytes(rng.choice(list(alphabet), rng.randint(0, 9)).astype(np.uint8)))
        return out

    files = []
    for j, k in enumerate((300, 0, 257, 64, 129)):
        ls = some_lines(k)
        data = b"".join(l + b"\n" for l in ls)
        if j in (0, 3):
            data += seeds[0]                    # a last line with bytes and no delimiter
        files.append(data)
    return flat, files


def answers(ht, ld):
    out = ht.exec(ld, ids_mode=1, want_bitmap=True, want_eager=True)
    n = ht.lines
    bits = np.unpackbits(out["bitmap"].view(np.uint8), bitorder="little")[:n].astype(bool)
    return out["end"], bits, out["ids"], out["eager"]


@pytest.mark.parametrize("name", ["newline", "endids_union_det"])
def test_walk_parity(hip, name):
    flat, files = parity_files(name)
    assert [len(f) == 0 for f in files] == [False, True, False, False, False]
    assert [f.endswith(b"\n") for f in files] == [False, False, True, False, True]
    text, fo = join_files(files)
    ld = hip.LinesDfa(flat, 0x0A)
    ht = hip.HipText(text, 0x0A, file_off=fo)
    off, fl = check_text(ht, text, 0x0A, fo)
    got = answers(ht, ld)
    # the existing code as the yardstick: every file opened alone
    each = []
    for f in files:
        one = hip.HipText(f, 0x0A)
        each.append(answers(one, ld))
        one.close()
    assert fl.tolist() == np.concatenate([[0], np.cumsum([len(e[0]) for e in each])]).tolist()
    for k, what in enumerate(("end", "bitmap", "ids", "eager")):
        assert np.array_equal(got[k], np.concatenate([e[k] for e in each])), what
    # the oracle on the lines, without their delimiters, over the original description
    lines = [l for f in files for l in lines_of(np.frombuffer(f, np.uint8), 0x0A)]
    assert len(lines) == ht.lines
    ret, end, ids, sets = oracle_answers(flat, lines)
    assert 0 < int((ret == 1).sum()) < len(lines)
    assert np.array_equal(got[0], end) and np.array_equal(got[1], ret == 1)
    assert np.array_equal(got[2], np.array([NO if t is None else (min(t) if t else NO_ID) for t in ids], np.uint32))
    assert [frozenset(int(x) for x in s) for s in ld.inner.decode_eager(got[3])] == sets
    # the only workaround there was: the plain text over the same bytes glues two pairs of lines and answers otherwise
    plain = hip.HipText(text, 0x0A)
    assert plain.lines == ht.lines - 2
    wrong = answers(plain, ld)
    assert not np.array_equal(wrong[0], got[0]) and not np.array_equal(wrong[1], got[1])
    plain.close()
    ht.close()


# ---- the hits ------------------------------------------------------------------------------------------------

def check_hits(h, text, off, fl, bits, invert, want_bytes, what):
    lines, out_off, out = hits_ref_off(text, off, bits, invert)
    assert h.count == len(lines), what
    assert np.array_equal(h.lines(), lines), what
    if want_bytes:
        assert h.nbytes == len(out), what
        assert np.array_equal(h.offsets(), out_off), what
        assert np.array_equal(h.bytes(), out), what
    else:
        assert h.nbytes == 0 and h.offsets_device == 0 and h.bytes_device == 0, what
    assert h.file_first_ptr != 0, what
    assert np.array_equal(h.file_first(), np.searchsorted(lines, fl).astype(np.uint64)), what
    h.close()


def test_hits_per_file(hip):
    import torch
    L = hip.text_hits_block_lines()
    rng = np.random.RandomState(6)
    nfiles, n0 = 40, 3 * L + 200
    tl = rng.randint(1, 30, n0)
    text = np.arange(1, 256, dtype=np.uint8)[rng.randint(0, 255, int(tl.sum()))]
    text[text == 0x0A] = 0x41
    text[np.cumsum(tl) - 1] = 0x0A
    inner = np.sort(np.concatenate([rng.randint(0, len(text) + 1, nfiles - 5), [0, 0, len(text), len(text)]]))
    fo = np.concatenate([[0], inner, [len(text)]]).astype(np.uint64)
    assert len(fo) == nfiles + 1
    ht = hip.HipText(text, 0x0A, file_off=fo)
    off, fl = check_text(ht, text, 0x0A, fo)
    n = ht.lines
    assert n > 3 * L and n > n0 + 10
    s = torch.cuda.Stream()
    cases = [("rand3", rng.randint(0, 3, n) == 0), ("rand50", rng.randint(0, 50, n) == 0), ("none", np.zeros(n, bool)), ("all", np.ones(n, bool))]
    for name, bits in cases:
        for invert in (False, True):
            for want_bytes in (True, False):
                bm = device_u64(pack_bits(bits, 1))      # spare bits set
                what = (name, invert, want_bytes)
                check_hits(ht.hits_device(bm.data_ptr(), invert=invert, want_bytes=want_bytes), text, off, fl, bits, invert, want_bytes, what)
                torch.cuda.synchronize()
                check_hits(ht.hits_device(bm.data_ptr(), invert=invert, want_bytes=want_bytes, stream=s.cuda_stream), text, off, fl, bits,
                           invert, want_bytes, what)
    # the host form (the walk's own bitmap) and the device form on a caller's stream over exec_device's bitmap agree
    ld = hip.LinesDfa(newline_dfa(), 0x0A)
    txt2, fo2 = join_files([b"a\nb\naa", b"", b"ab\n\na\n", b"\naaa", b"b"])
    ht2 = hip.HipText(txt2, 0x0A, file_off=fo2)
    off2, fl2 = check_text(ht2, txt2, 0x0A, fo2)
    lines2 = [bytes(txt2[int(a):int(b)]).rstrip(b"\n") for a, b in zip(off2[:-1], off2[1:])]
    bits2 = oracle_answers(newline_dfa(), lines2)[0] == 1
    assert lines2 == [b"a", b"b", b"aa", b"ab", b"", b"a", b"", b"aaa", b"b"] and 0 < bits2.sum() < len(bits2)
    for invert in (False, True):
        for want_bytes in (True, False):
            host = ht2.hits(ld, invert=invert, want_bytes=want_bytes)
            d_bm = torch.full(((ht2.lines + 63) // 64,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ht2.exec_device(ld, d_bitmap=d_bm.data_ptr(), stream=s.cuda_stream)
            dev = ht2.hits_device(d_bm.data_ptr(), invert=invert, want_bytes=want_bytes, stream=s.cuda_stream)
            assert np.array_equal(host.file_first(), dev.file_first()) and np.array_equal(host.lines(), dev.lines())
            dev.close()
            check_hits(host, txt2, off2, fl2, bits2, invert, want_bytes, (invert, want_bytes))
    ht2.close()
    ht.close()


# ---- the device form -----------------------------------------------------------------------------------------

def test_device_form_and_invalid_arrays(hip):
    import torch
    B = hip.text_block_bytes()
    rng = np.random.RandomState(12)
    text = random_text(2 * B + 77, 0x0A, 20, rng)
    fo = random_ends(text, 0x0A, 300, B, rng)
    dev, addr = to_device(text, lead=3, pad=64, fill=0x0A)
    assert addr % 2 == 1
    s = torch.cuda.Stream()
    want = files_ref(text, 0x0A, fo)

    def open_with(arr):
        d_fo = device_u64(arr)
        torch.cuda.synchronize()
        ht = hip.HipText(d_text=addr, nbytes=len(text), delim=0x0A, stream=s.cuda_stream, file_off=d_fo.data_ptr(), nfiles=len(arr) - 1)
        ht._keep = d_fo
        return ht

    ld = hip.LinesDfa(newline_dfa(), 0x0A)

    def good():
        ht = open_with(fo)
        # later work on the caller's stream sees the arrays: a walk enqueued there right away, before any accessor waits
        d_end = torch.full((len(want[0]) - 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ht.exec_device(ld, d_end=d_end.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        check_text(ht, text, 0x0A, fo)
        assert np.array_equal(d_end.cpu().numpy().view(np.uint32), ht.exec(ld)["end"])
        ht.close()

    good()
    first_not_0, decreasing = fo.copy(), fo.copy()
    first_not_0[0] = 1
    k = int(np.flatnonzero(np.diff(fo.astype(np.int64)) > 1)[5])
    decreasing[k], decreasing[k + 1] = fo[k + 1], fo[k]
    last_not_n = np.minimum(fo, np.uint64(len(text) - 1))            # still non-decreasing: only the last entry is wrong
    for bad in (first_not_0, decreasing, last_not_n):
        with pytest.raises(OSError) as ei:
            open_with(bad)
        assert ei.value.errno == errno.EINVAL
        good()
    # the host form checks on the host; nfiles == 0 and a NULL array
    for bad in (first_not_0, decreasing, last_not_n, fo[:1]):
        with pytest.raises(OSError) as ei:
            hip.HipText(text, 0x0A, file_off=bad)
        assert ei.value.errno == errno.EINVAL
    with pytest.raises(OSError) as ei:
        hip.HipText(d_text=addr, nbytes=len(text), delim=0x0A, file_off=0, nfiles=3)
    assert ei.value.errno == errno.EINVAL
    del dev


# ---- the example ---------------------------------------------------------------------------------------------

def test_example_prints_what_grep_H_prints(hip, tmp_path):
    """examples/hipgrep_files.c over five files (one empty, two without a final newline), against output composed from the
    oracle's answers per file"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    det = Golden(os.path.join(GOLDEN, "endids_union_det.npz"))
    table = str(tmp_path / "t.fsmhip")
    det.flat.write_c(table)
    rng = np.random.RandomState(8)
    strings = list(det.strings())
    per_file = []
    for j, k in enumerate((120, 0, 77, 1, 40)):
        ls = [strings[rng.randint(len(strings))] if i % 3 == 0 else bytes(rng.choice(list(b"abcdefor_X"), rng.randint(0, 12)).astype(np.uint8))
              for i in range(k)]
        if j in (0, 3):
            ls[-1] = strings[0]                     # a last line that matches and has no newline after it
        per_file.append(ls)
    names = []
    for j, ls in enumerate(per_file):
        data = b"".join(l + b"\n" for l in ls)
        if j in (0, 3):
            data = data[:-1]
        p = tmp_path / ("f%d.txt" % j)
        p.write_bytes(data)
        names.append(str(p))
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    exe = str(tmp_path / "hipgrep_files")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "hipgrep_files.c"), "-o", exe,
                           "-L" + os.path.join(root, "libfsm_amd"), "-lfsm_hip", "-Wl,-rpath," + os.path.join(root, "libfsm_amd")])
    rets = [oracle_answers(det.flat, ls)[0] == 1 if ls else np.zeros(0, bool) for ls in per_file]
    assert sum(int(r.sum()) for r in rets) >= 10 and sum(int((~r).sum()) for r in rets) >= 10

    def run(*opts, files=names):
        r = subprocess.run([exe, *opts, table, *files], capture_output=True, env=env, timeout=120)
        return r.returncode, r.stdout

    def compose(fmt, invert=False):
        out = b""
        for name, ls, r in zip(names, per_file, rets):
            out += fmt(name.encode(), ls, r ^ invert)
        return out

    plain = lambda nm, ls, r: b"".join(nm + b":" + l + b"\n" for l, s in zip(ls, r) if s)                            # noqa: E731
    numbered = lambda nm, ls, r: b"".join(nm + b":%d:" % (i + 1) + l + b"\n" for i, (l, s) in enumerate(zip(ls, r)) if s)   # noqa: E731
    counted = lambda nm, ls, r: nm + b":%d\n" % int(r.sum())                                                         # noqa: E731
    with_hit = lambda nm, ls, r: nm + b"\n" if r.any() else b""                                                       # noqa: E731
    without = lambda nm, ls, r: b"" if r.any() else nm + b"\n"                                                        # noqa: E731
    assert run() == (0, compose(plain))
    assert run("-n") == (0, compose(numbered))
    assert run("-c") == (0, compose(counted))
    assert run("-l") == (0, compose(with_hit))
    assert run("-L") == (0, compose(without))
    assert compose(without) == names[1].encode() + b"\n"
    assert run("-v") == (0, compose(plain, True))
    assert run("-v", "-n") == (0, compose(numbered, True))
    assert run("-v", "-c") == (0, compose(counted, True))
    assert run(files=[names[1]]) == (1, b"")                   # nothing selected: grep's 1
    assert run("-x")[0] == 2                                   # an error: grep's 2
