"""GPU: context lines for the hits of a text (libfsm_amd/csrc/text.hip: ctx_file_starts, ctx_summary, ctx_scan, ctx_apply,
ctx_marks; include/fsm_hip.h, "Context"): the lines within `before` / `after` lines of a selected line of the same file, with
the core and group marks.

Everything is compared bit for bit with the rule stated in numpy (tests/context_ref.py: the literal definition, and the
nearest-witness form where a text is large), never with anything derived from the code under test; zero context also with
fsm_hip_text_hits_device on the same bitmap (the existing code as the yardstick)."""
import ctypes as C
import errno
import os
import subprocess

import numpy as np
import pytest

from context_ref import compose, context_literal, context_witness, marks_ref, pack_marks
from files_ref import files_ref, hits_ref_off
from hits_ref import pack_bits
from text_ref import split_ref

pytestmark = pytest.mark.gpu

ALL = 2 ** 64 - 1
GARBAGE = np.uint64(0xA5A5A5A5A5A5A5A5)


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()   # raises if the HIP extension is missing: no silent fallback
    return libfsm_amd


@pytest.fixture(scope="module")
def ld_m(hip):
    """the line matcher of grep -x m"""
    return hip.LinesDfa(hip.FlatDfa.from_strings([b"m"], 3), 0x0A)


def text_of(sel, rng, trailing=True):
    """lines of 0..1 bytes: "m" where sel holds, "x" or nothing elsewhere; without `trailing` the last line (given a byte) loses its newline"""
    sel = np.asarray(sel, bool)
    n = len(sel)
    body = np.where(sel, ord("m"), np.where(rng.randint(0, 2, n) == 0, ord("x"), 0)).astype(np.uint8)
    if n and not trailing and body[-1] == 0:
        body[-1] = ord("x")
    text = np.stack([body, np.full(n, 0x0A, np.uint8)], axis=1).reshape(-1)
    text = text[text != 0]
    return np.ascontiguousarray(text if trailing or n == 0 else text[:-1])


def device_bitmap(bits, garbage=1):
    """the bitmap at an ODD word offset inside a larger allocation of garbage, its spare bits all `garbage`: (tensor, address)"""
    import torch
    words = pack_bits(bits, garbage)
    host = np.full(3 + len(words) + 2, GARBAGE, np.uint64)
    host[3:3 + len(words)] = words
    t = torch.from_numpy(host.view(np.int64).copy()).cuda()
    assert (t.data_ptr() + 24) // 8 % 2 == 1
    return t, t.data_ptr() + 24


def expect(text, off, bits, invert, before, after, fl=None, witness=False):
    sel = np.asarray(bits, bool) ^ bool(invert)
    W = (context_witness if witness else context_literal)(sel, before, after, fl)
    lines, out_off, out = hits_ref_off(text, off, W)
    lines2, core, group = marks_ref(sel, W, fl)
    assert np.array_equal(lines, lines2)
    return dict(lines=lines, out_off=out_off, out=out, core=core, group=group, core_count=int(sel.sum()), groups=int(group.sum()), fl=fl)


def check(h, want, want_bytes=True, what=None):
    m = len(want["lines"])
    assert h.count == m, what
    assert h.core_count == want["core_count"], what
    assert np.array_equal(h.lines(), want["lines"]), what
    if want_bytes:
        assert h.nbytes == len(want["out"]), what
        assert np.array_equal(h.offsets(), want["out_off"]), what
        assert np.array_equal(h.bytes(), want["out"]), what
    else:
        assert h.nbytes == 0 and h.offsets_device == 0 and h.bytes_device == 0, what
    core_w, group_w = h.marks_words()                         # whole words: the spare bits are 0
    assert np.array_equal(core_w, pack_marks(want["core"])), what
    assert np.array_equal(group_w, pack_marks(want["group"])), what
    assert np.array_equal(h.core(), want["core"]) and np.array_equal(h.group(), want["group"]), what
    assert h.groups == want["groups"], what
    assert (h.core_ptr != 0) == (m != 0) and (h.group_ptr != 0) == (m != 0), what
    assert h.context_ms() >= 0.0, what
    if want["fl"] is not None:
        assert h.file_first_ptr != 0, what
        assert np.array_equal(h.file_first(), np.searchsorted(want["lines"], want["fl"]).astype(np.uint64)), what
    else:
        assert h.file_first_ptr == 0, what
    h.close()


def sizes(hip):
    L = hip.text_hits_block_lines()
    return [1, 63, 64, 65, 128, L - 1, L, L + 1, 3 * L + 5]


SIZE_IDS = ["1", "63", "64", "65", "128", "L-1", "L", "L+1", "3L+5"]


def context_pairs(n, rng):
    """every k alone in each direction, (k, k), and mixed pairs"""
    ks = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, n, ALL]
    pairs = [(0, k) for k in ks] + [(k, 0) for k in ks[1:]] + [(k, k) for k in ks[1:]]
    pairs += [(ks[rng.randint(len(ks))], ks[rng.randint(len(ks))]) for _ in range(8)]
    return pairs


@pytest.mark.parametrize("si", range(len(SIZE_IDS)), ids=SIZE_IDS)
def test_line_counts_and_contexts(hip, ld_m, si):
    import torch
    n = sizes(hip)[si]
    rng = np.random.RandomState(100 + si)
    s = torch.cuda.Stream()
    for density in (2, 40, 5000):
        bits = rng.randint(0, density, n) == 0
        if density == 5000 and n > 1:
            bits[rng.randint(0, n)] = True                 # a gap longer than a block on both sides of something
        text = text_of(bits, rng, trailing=density != 40)
        off = split_ref(text, 0x0A)
        assert len(off) - 1 == n
        ht = hip.HipText(text, 0x0A)
        got = np.unpackbits(ht.exec(ld_m, want_end=False, want_bitmap=True)["bitmap"].view(np.uint8), bitorder="little")[:n].astype(bool)
        assert np.array_equal(got, bits)                   # the walk selects what the text was built from
        keep, d_bm = device_bitmap(bits, 1)
        for k, (before, after) in enumerate(context_pairs(n, rng)):
            for invert in (False, True):
                want = expect(text, off, bits, invert, before, after)
                what = (n, density, before, after, invert)
                want_bytes = k % 5 != 4                    # under NO_BYTES the marks are still compared
                check(ht.hits_context_device(d_bm, before, after, invert=invert, want_bytes=want_bytes, stream=s.cuda_stream if k % 2 else 0),
                      want, want_bytes, what)
                if k % 3 == 0:
                    check(ht.hits_context(ld_m, before, after, invert=invert, want_bytes=want_bytes), want, want_bytes, what)
        del keep
        ht.close()


def test_extreme_bitmaps(hip, ld_m):
    L = hip.text_hits_block_lines()
    rng = np.random.RandomState(3)
    n = 2 * L + 77
    first, last = np.zeros(n, bool), np.zeros(n, bool)
    first[0] = True
    last[-1] = True
    cases = [("first", first, 0, ALL, n), ("last", last, ALL, 0, n), ("first_1", first, ALL, 1, 2), ("last_1", last, 1, ALL, 2),
             ("none", np.zeros(n, bool), ALL, ALL, 0), ("none_5", np.zeros(n, bool), 5, 5, 0), ("all", np.ones(n, bool), 3, ALL, n),
             ("all_0", np.ones(n, bool), 0, 0, n)]
    for name, bits, before, after, m in cases:
        text = text_of(bits, rng)
        off = split_ref(text, 0x0A)
        ht = hip.HipText(text, 0x0A)
        keep, d_bm = device_bitmap(bits, 1)
        want = expect(text, off, bits, False, before, after)
        assert len(want["lines"]) == m, name
        check(ht.hits_context_device(d_bm, before, after), want, True, name)
        check(ht.hits_context(ld_m, before, after), want, True, name)
        inv = expect(text, off, bits, True, before, after)
        check(ht.hits_context_device(d_bm, before, after, invert=True), inv, True, name)
        del keep
        ht.close()
    # n == 0: no line, no hit, no array; a NULL bitmap is taken
    ht = hip.HipText(b"", 0x0A)
    for h in (ht.hits_context_device(0, ALL, ALL), ht.hits_context(ld_m, 1, 2), ht.hits_context_device(0, 0, 0, want_bytes=False)):
        assert h.count == 0 and h.core_count == 0 and h.groups == 0 and h.core_ptr == 0 and h.group_ptr == 0 and h.nbytes == 0
        assert len(h.core()) == 0 and len(h.group()) == 0 and h.context_ms() >= 0.0
        h.close()
    ht.close()


def files_case(hip, nfiles, rng):
    """(files, bits): n = 3L + 5 lines in nfiles files whose starts fall in mid-word, on a word edge and on a block edge, with
    runs of empty files; one file's first line and another file's last line are selected with nothing selected on the other side
    of the file end, so that a context which crossed it would show"""
    L = hip.text_hits_block_lines()
    n = 3 * L + 5
    if nfiles == 1:
        starts = np.array([0], np.int64)
    else:
        special = np.array([37, 64, L, L, L, 2 * L - 1, 2 * L + 64, 0, n, n], np.int64)       # empty files: at the start, at L, at the end
        starts = np.sort(np.concatenate([[0], special[:nfiles - 1], rng.randint(0, n + 1, max(nfiles - 1 - len(special), 0))]))
    fl = np.concatenate([starts, [n]]).astype(np.uint64)
    assert len(fl) == nfiles + 1
    bits = rng.randint(0, 40, n) == 0
    inner = np.unique(starts[(starts > 0) & (starts < n)])
    if len(inner):
        s1, s2 = int(inner[0]), int(inner[-1])
        bits[max(s1 - 40, 0):s1] = False
        bits[s1] = True                                                                       # a file's first line, nothing before it
        if s2 != s1:
            bits[s2 - 1:s2 + 40] = False
            bits[s2 - 1] = True                                                               # a file's last line, nothing after it
    return n, fl, bits


@pytest.mark.parametrize("nfiles", [1, 2, 7, 500])
def test_files(hip, ld_m, nfiles):
    rng = np.random.RandomState(40 + nfiles)
    L = hip.text_hits_block_lines()
    n, fl, bits = files_case(hip, nfiles, rng)
    text = text_of(bits, rng, trailing=False)
    off_plain = split_ref(text, 0x0A)
    fo = off_plain[fl.astype(np.int64)]                       # the files end at line ends: the lines are the plain text's
    ht = hip.HipText(text, 0x0A, file_off=fo)
    off, fl_got = files_ref(text, 0x0A, fo)
    assert np.array_equal(off, off_plain) and np.array_equal(fl_got, fl) and np.array_equal(ht.file_lines(), fl)
    if nfiles >= 7:
        assert {37, 64, L} <= set(fl.tolist()) and (np.diff(fl.astype(np.int64)) == 0).sum() >= 2
    keep, d_bm = device_bitmap(bits, 1)
    crossed = 0
    for k, (before, after) in enumerate([(0, 0), (1, 1), (0, 2), (2, 0), (63, 64), (65, 1), (1, 1025), (1024, 1023), (n, 0), (0, n), (ALL, ALL), (5, ALL)]):
        for invert in (False, True):
            want = expect(text, off, bits, invert, before, after, fl)
            crossed += int(len(want["lines"]) != len(expect(text, off, bits, invert, before, after)["lines"]))
            what = (nfiles, before, after, invert)
            check(ht.hits_context_device(d_bm, before, after, invert=invert, want_bytes=k % 4 != 3), want, k % 4 != 3, what)
            if k % 4 == 1:
                check(ht.hits_context(ld_m, before, after, invert=invert), want, True, what)
    assert (crossed > 0) == (nfiles > 1)                      # contexts that would cross a file end were cut there
    if nfiles == 1:                                           # one file equals the plain text
        plain = hip.HipText(text, 0x0A)
        for before, after in ((2, 3), (ALL, 0)):
            a, b = ht.hits_context_device(d_bm, before, after), plain.hits_context_device(d_bm, before, after)
            for f in ("lines", "offsets", "bytes", "core", "group"):
                assert np.array_equal(getattr(a, f)(), getattr(b, f)()), f
            assert (a.count, a.core_count, a.groups) == (b.count, b.core_count, b.groups) and b.file_first_ptr == 0
            a.close()
            b.close()
        plain.close()
    del keep
    ht.close()


def test_scan_carries(hip):
    """more blocks of lines than the most workgroups and than two rounds of ctx_scan: a single selected line near each end, and
    contexts that reach across every round in each direction"""
    L, Wg, SB = hip.text_hits_block_lines(), hip.text_max_workgroups(), hip.text_context_scan_block()
    nblocks = max(Wg, 2 * SB) + 3
    n = nblocks * L + 17
    rng = np.random.RandomState(11)
    bits = np.zeros(n, bool)
    bits[5] = True
    bits[n - 7] = True
    text = text_of(bits, rng)
    assert 2 ** 21 <= len(text) <= 2 ** 23                    # a few MB of 0-1-byte lines
    off = split_ref(text, 0x0A)
    fl = np.array([0, 3, n // 2 + 1, n // 2 + 1, n - 100, n], np.uint64)
    fo = off[fl.astype(np.int64)]
    plain, files = hip.HipText(text, 0x0A), hip.HipText(text, 0x0A, file_off=fo)
    keep, d_bm = device_bitmap(bits, 1)
    for before, after in ((0, ALL), (ALL, 0), (n, n), (0, n - 13), (n - 13, 0), (2 * SB * L, 3), (ALL, ALL)):
        for ht, lines_of_files in ((plain, None), (files, fl)):
            want = expect(text, off, bits, False, before, after, lines_of_files, witness=True)
            if lines_of_files is None and before != 3 and after != 3:
                assert len(want["lines"]) > 2 * SB * L        # the reach did cross every round
            check(ht.hits_context_device(d_bm, before, after, want_bytes=False), want, False, (before, after, lines_of_files is None))
    # the inverse: everything but two lines selected, the carries of a dense bitmap; and a sparse random one
    want = expect(text, off, bits, True, 1, 0, fl, witness=True)
    check(files.hits_context_device(d_bm, 1, 0, invert=True), want, True, "inverted")
    sparse = rng.randint(0, 5000, n) == 0
    keep2, d_bm2 = device_bitmap(sparse, 0)
    for before, after in ((1025, 0), (0, 1025), (5000, 70)):
        want = expect(text, off, sparse, False, before, after, fl, witness=True)
        check(files.hits_context_device(d_bm2, before, after, want_bytes=False), want, False, (before, after))
    del keep, keep2
    plain.close()
    files.close()


def test_zero_context_equals_the_plain_hits(hip):
    """before = after = 0 against fsm_hip_text_hits_device on the same bitmap, array for array; core all ones"""
    L = hip.text_hits_block_lines()
    rng = np.random.RandomState(21)
    n = 2 * L + 31
    bits = rng.randint(0, 3, n) == 0
    text = text_of(bits, rng, trailing=False)
    off = split_ref(text, 0x0A)
    fl = np.array([0, 0, 100, L, L, n - 1, n], np.uint64)
    for ht in (hip.HipText(text, 0x0A), hip.HipText(text, 0x0A, file_off=off[fl.astype(np.int64)])):
        keep, d_bm = device_bitmap(bits, 1)
        for invert in (False, True):
            for want_bytes in (True, False):
                a = ht.hits_context_device(d_bm, 0, 0, invert=invert, want_bytes=want_bytes)
                b = ht.hits_device(d_bm, invert=invert, want_bytes=want_bytes)
                assert a.count == b.count == a.core_count and a.nbytes == b.nbytes
                assert np.array_equal(a.lines(), b.lines()) and a.core().all()
                if want_bytes:
                    assert np.array_equal(a.offsets(), b.offsets()) and np.array_equal(a.bytes(), b.bytes())
                if ht.files:
                    assert np.array_equal(a.file_first(), b.file_first())
                lines = b.lines()
                runs = np.ones(len(lines), bool)
                runs[1:] = np.diff(lines.astype(np.int64)) != 1
                if ht.files:
                    runs[1:] |= np.diff(np.searchsorted(fl, lines, side="right")) != 0
                assert np.array_equal(a.group(), runs) and a.groups == int(runs.sum())
                a.close()
                b.close()
        del keep
        ht.close()


def test_unchanged_entry_points(hip, ld_m):
    """hits made by the two existing entry points know no context, and flags 4 and 8 are still EINVAL there"""
    text = np.frombuffer(b"x\nm\nx\n", np.uint8)
    ht = hip.HipText(text, 0x0A)
    keep, d_bm = device_bitmap([False, True, False], 1)
    for h in (ht.hits(ld_m), ht.hits_device(d_bm)):
        assert h.count == 1 and h.lines().tolist() == [1]
        assert h.core_ptr == 0 and h.group_ptr == 0 and h.core_count == 0 and h.groups == 0
        with pytest.raises(OSError) as ei:
            h.core()
        assert ei.value.errno == errno.EINVAL
        C.set_errno(0)
        assert h.context_ms() == -1.0 and C.get_errno() == errno.EINVAL
        h.close()
    for flags in (4, 8, 6):
        with pytest.raises(OSError) as ei:
            ht.hits_device(d_bm, flags=flags)
        assert ei.value.errno == errno.EINVAL
        with pytest.raises(OSError) as ei:
            ht.hits_context_device(d_bm, 1, 1, flags=flags)
        assert ei.value.errno == errno.EINVAL
    del keep
    ht.close()


def test_repeat(hip):
    """one case twice on one text, the hits freed in between: the same answers"""
    L = hip.text_hits_block_lines()
    rng = np.random.RandomState(31)
    n = 3 * L + 5
    bits = rng.randint(0, 40, n) == 0
    text = text_of(bits, rng)
    off = split_ref(text, 0x0A)
    fl = np.array([0, 37, L, L, 2 * L + 64, n], np.uint64)
    ht = hip.HipText(text, 0x0A, file_off=off[fl.astype(np.int64)])
    keep, d_bm = device_bitmap(bits, 1)
    want = expect(text, off, bits, False, 65, 2, fl)
    for _ in range(2):
        check(ht.hits_context_device(d_bm, 65, 2), want, True, "repeat")
    del keep
    ht.close()


GREP_H_N_A1_B1 = b"""a-1-x
a:2:m
a-3-x
--
b-1-x
b:2:m
--
c:1:m
c-2-x
--
c-4-x
c:5:m
c:6:m
c-7-x
"""


def test_example_prints_what_grep_prints_with_context(hip, tmp_path):
    """examples/hipgrep_context.c over a, b, c of the header's transcript plus an empty file, run from the files' directory so
    that the names are grep's"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    table = str(tmp_path / "t.fsmhip")
    hip.FlatDfa.from_strings([b"m"], 3).write_c(table)
    contents = {"a": b"x\nm\nx\n", "b": b"x\nm\n", "c": b"m\nx\nx\nx\nm\nm\nx", "e": b""}
    for name, data in contents.items():
        (tmp_path / name).write_bytes(data)
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    exe = str(tmp_path / "hipgrep_context")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "hipgrep_context.c"), "-o", exe,
                           "-L" + os.path.join(root, "libfsm_amd"), "-lfsm_hip", "-Wl,-rpath," + os.path.join(root, "libfsm_amd")])
    names = ["a", "e", "b", "c"]

    def run(*opts, files=names):
        r = subprocess.run([exe, *opts, table, *files], capture_output=True, env=env, timeout=120, cwd=str(tmp_path))
        return r.returncode, r.stdout

    per_file = [contents[nm].split(b"\n") for nm in names]
    per_file = [ls[:-1] if ls[-1] == b"" else ls for ls in per_file]
    sels = [[l == b"m" for l in ls] for ls in per_file]
    inv = [[not s for s in ss] for ss in sels]
    bnames = [nm.encode() for nm in names]
    assert run("-A", "1", "-B", "1", "-n") == (0, GREP_H_N_A1_B1)
    assert compose(bnames, per_file, sels, 1, 1) == GREP_H_N_A1_B1
    assert run("-v", "-A", "1") == (0, compose(bnames, per_file, inv, 0, 1, number=False))
    assert run("-v", "-A", "1", "-n") == (0, compose(bnames, per_file, inv, 0, 1))
    assert run("-C", "1000") == (0, compose(bnames, per_file, sels, 1000, 1000, number=False))
    assert run("-n", "-B", "2", files=["c"]) == (0, b"c:1:m\n--\nc-3-x\nc-4-x\nc:5:m\nc:6:m\n")
    assert run("-B", str(ALL), "-A", "0", "-n", files=["c"]) == (0, compose([b"c"], per_file[3:], sels[3:], ALL, 0))
    assert run("-C", "3", files=["e"]) == (1, b"")            # nothing selected: grep's 1
    assert run("-A")[0] == 2 and run("-A", "x", "a")[0] == 2   # an error: grep's 2
