"""GPU: the text front (libfsm_amd/csrc/text.hip, lines.cpp): one buffer with a delimiter between records, cut into lines on
the device and walked in one call.

The offsets the three scan kernels leave are compared with text_ref.split_ref (the line rule stated in numpy), never with
anything derived from the code under test; the walk's outputs with the oracle walking every line WITHOUT its delimiter over
the ORIGINAL description, and with the original dfa on a hipgrep.c-style squeezed copy."""
import errno
import os
import subprocess

import numpy as np
import pytest

from common import GOLDEN, Golden
from text_ref import lines_of, newline_dfa, oracle_answers, split_ref, squeeze_ref

pytestmark = pytest.mark.gpu

NO, NO_ID = 0xFFFFFFFF, 0xFFFFFFFE
DELIMS = (0x0A, 0x00, 0x80, 0xFF)


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


def fillers(delim):
    """bytes that differ from the delimiter in one bit, by one, or are the SWAR constants themselves: a byte test with false
    positives (the borrow of the has-zero shortcut, a missed bit 7) counts one of them"""
    c = {delim ^ 0x80, (delim + 1) & 0xFF, (delim - 1) & 0xFF, 0x00, 0x7F, 0x80, 0xFF, delim ^ 0x01}
    return np.array(sorted(c - {delim}), np.uint8)


def sizes(hip):
    B, G = hip.text_block_bytes(), hip.text_max_workgroups()
    assert B >= 1024 and G >= 1
    return [0, 1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, B - 1, B, B + 1, 2 * B + 5, (G + 1) * B + 17]


SIZE_IDS = ["0", "1", "15", "16", "17", "31", "32", "33", "1023", "1024", "1025", "B-1", "B", "B+1", "2B+5", "(G+1)B+17"]


def contents(n, delim, B, rng):
    """(name, positions of the delimiters) for a text of n bytes"""
    def around(step):
        k = np.arange(0, n + step, step, dtype=np.int64)
        p = np.unique(np.concatenate([k - 1, k, k + 1]))
        return p[(p >= 0) & (p < n)]
    out = [("none", np.zeros(0, np.int64)), ("all", np.arange(n, dtype=np.int64))]
    if n:
        out += [("first", np.array([0])), ("last", np.array([n - 1]))]
    out += [("mult16", around(16)), ("mult1024", around(1024)), ("multB", around(B))]
    out += [("rand8", np.flatnonzero(rng.randint(0, 8, n) == 0)), ("rand200", np.flatnonzero(rng.randint(0, 200, n) == 0))]
    return out


@pytest.mark.parametrize("delim", DELIMS, ids=["0x%02x" % d for d in DELIMS])
@pytest.mark.parametrize("si", range(len(SIZE_IDS)), ids=SIZE_IDS)
def test_scan_matches_reference_splitter(hip, si, delim):
    n = sizes(hip)[si]
    B = hip.text_block_bytes()
    rng = np.random.RandomState(1000 * si + delim)
    fill = fillers(delim)
    base = fill[rng.randint(0, len(fill), n)] if n else np.zeros(0, np.uint8)
    for name, pos in contents(n, delim, B, rng):
        buf = base.copy()
        buf[pos] = delim
        want = split_ref(buf, delim)
        t = hip.HipText(buf, delim)
        assert t.lines == len(want) - 1, (name, "open")
        assert np.array_equal(t.offsets(), want), (name, "open")
        t.close()
        dev, addr = to_device(buf)
        t = hip.HipText(d_text=addr, nbytes=n, delim=delim)
        assert t.lines == len(want) - 1, (name, "open_device")
        assert np.array_equal(t.offsets(), want), (name, "open_device")
        t.close()
        del dev


@pytest.mark.parametrize("delim", DELIMS, ids=["0x%02x" % d for d in DELIMS])
@pytest.mark.parametrize("lead", [1, 3, 13])
def test_neighbours_are_not_read_as_text(hip, lead, delim):
    """a text that starts 1, 3, 13 bytes into an allocation, 64 bytes of delimiters before and after it: none of them counts"""
    B = hip.text_block_bytes()
    rng = np.random.RandomState(lead * 7 + delim)
    fill = fillers(delim)
    for n in (0, 1, 5, 16, 17, 1000, B - 3, B + 5, 2 * B + 33):
        buf = fill[rng.randint(0, len(fill), n)] if n else np.zeros(0, np.uint8)
        buf[rng.randint(0, 8, n) == 0] = delim
        if n > 1:
            buf[-1] = fill[0]                         # the last byte is no delimiter: the one behind it must not end the line
        want = split_ref(buf, delim)
        dev, addr = to_device(buf, lead=lead, pad=64, fill=delim)
        t = hip.HipText(d_text=addr, nbytes=n, delim=delim)
        assert t.lines == len(want) - 1, n
        assert np.array_equal(t.offsets(), want), n
        t.close()
        del dev


# ---- parity of the walk ------------------------------------------------------------------------------------

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


def walk_case(hip, name, trailing):
    """the text, the reference's answers line by line, and the objects under test"""
    flat, seeds, alphabet, plant = automata(hip)[name]
    text = make_text(hip, flat, seeds, alphabet, plant, trailing)
    lines = lines_of(text, 0x0A)
    ret, end, ids, sets = oracle_answers(flat, lines)
    return dict(flat=flat, text=text, lines=lines, ret=ret, end=end, ids=ids, sets=sets, ld=hip.LinesDfa(flat, 0x0A), ht=hip.HipText(text, 0x0A))


def expected_ids(c, ld, mode):
    """what id_out holds under FSM_HIP_IDS_EARLIEST / _RET, from the oracle's id tuples"""
    if mode == 2:
        rets = [tuple(int(x) for x in r) for r in ld.inner.ret_sets()]
        return np.array([NO if t is None else rets.index(t) for t in c["ids"]], np.uint32)
    return np.array([NO if t is None else (min(t) if t else NO_ID) for t in c["ids"]], np.uint32)


@pytest.mark.parametrize("trailing", [True, False], ids=["trailing", "no_trailing"])
@pytest.mark.parametrize("name", ["c1", "endids_union_det", "eager40", "newline"])
def test_walk_parity(hip, name, trailing):
    import torch
    c = walk_case(hip, name, trailing)
    ld, ht, n = c["ld"], c["ht"], len(c["lines"])
    assert n == NLINES and ht.lines == n and (c["text"][-1] == 0x0A) == trailing
    assert np.array_equal(ht.offsets(), split_ref(c["text"], 0x0A))
    assert 0.01 * n < int((c["ret"] == 1).sum()) < n, "the text must hold accepted and rejected lines"
    bits_want = c["ret"] == 1
    conflict = any(t is not None and len(t) > 1 for t in c["ids"]) or ld.inner.ids_conflict() is not None
    W = ld.inner.eager_words()
    # the original dfa on the squeezed copy, hipgrep.c's way
    sq, so, k = squeeze_ref(c["text"], 0x0A)
    assert k == n
    end_sq, bm_sq = hip.HipDfa(c["flat"]).exec_batch_offsets(sq, so)
    assert np.array_equal(end_sq, c["end"])
    for mode in (0, 1, 2, 3):
        if mode == 3 and conflict:
            with pytest.raises(OSError) as ei:
                ht.exec(ld, ids_mode=3, want_bitmap=True, want_eager=True)
            assert ei.value.errno == errno.EINVAL
            continue
        out = ht.exec(ld, ids_mode=mode, want_bitmap=True, want_eager=True)
        assert np.array_equal(out["end"], c["end"]), mode
        assert np.array_equal(out["end"], end_sq) and np.array_equal(out["bitmap"], bm_sq), mode
        bits = np.unpackbits(out["bitmap"].view(np.uint8), bitorder="little")[:n].astype(bool)
        assert np.array_equal(bits, bits_want), mode
        if mode:
            assert np.array_equal(out["ids"], expected_ids(c, ld, 1 if mode == 3 else mode)), mode
        got_sets = [frozenset(int(x) for x in s) for s in ld.inner.decode_eager(out["eager"])]
        assert got_sets == c["sets"], mode
        # the device form into device buffers: the same words
        d_end = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        d_bm = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
        d_ids = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_eo = torch.zeros((n, W), dtype=torch.int64, device="cuda")
        ht.exec_device(ld, d_end.data_ptr(), d_bm.data_ptr(), mode, d_ids.data_ptr() if mode else 0, d_eo.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_end.cpu().numpy().view(np.uint32), out["end"]), mode
        assert np.array_equal(d_bm.cpu().numpy().view(np.uint64), out["bitmap"]), mode
        assert np.array_equal(d_eo.cpu().numpy().view(np.uint64), out["eager"]), mode
        if mode:
            assert np.array_equal(d_ids.cpu().numpy().view(np.uint32), out["ids"]), mode
    # single outputs, the others NULL
    assert np.array_equal(ht.exec(ld)["end"], c["end"])
    only_bm = ht.exec(ld, want_end=False, want_bitmap=True)
    assert only_bm["end"] is None and np.array_equal(only_bm["bitmap"], bm_sq)
    # a text opened over device bytes the caller owns: the same answers
    dev, addr = to_device(c["text"], lead=5, pad=64, fill=0x0A)
    ht2 = hip.HipText(d_text=addr, nbytes=len(c["text"]), delim=0x0A)
    assert np.array_equal(ht2.exec(ld)["end"], c["end"])
    ht2.close()


def test_misuse_and_edge_cases(hip):
    flat = newline_dfa()
    c1 = Golden(os.path.join(GOLDEN, "c1.npz")).flat
    text = b"a\naa\nab\n\nb\na"
    lines = lines_of(np.frombuffer(text, np.uint8), 0x0A)
    ht = hip.HipText(text, 0x0A)
    assert ht.lines == len(lines) == 6
    # one text, two line matchers
    for f in (flat, c1):
        ld = hip.LinesDfa(f, 0x0A)
        assert ld.delim == 0x0A
        assert np.array_equal(ht.exec(ld)["end"], oracle_answers(f, lines)[1])
    # a matcher built for another delimiter: EINVAL, outputs untouched
    ld0 = hip.LinesDfa(flat, 0x00)
    out = {"end": np.full(6, 0x11111111, np.uint32), "bitmap": np.full(1, 0x2222, np.uint64), "ids": np.full(6, 0x33, np.uint32),
           "eager": np.full((6, ld0.inner.eager_words()), 0x44, np.uint64)}
    keep = {k: v.copy() for k, v in out.items()}
    with pytest.raises(OSError) as ei:
        ht.exec(ld0, ids_mode=1, out=out)
    assert ei.value.errno == errno.EINVAL
    with pytest.raises(OSError) as ei:
        ht.exec_device(ld0, 0, 0, 0, 0, 0)
    assert ei.value.errno == errno.EINVAL
    assert all(np.array_equal(out[k], keep[k]) for k in out)
    # a text of 0 lines: 0, outputs untouched (both fronts)
    ld = hip.LinesDfa(flat, 0x0A)
    for empty in (hip.HipText(b"", 0x0A), hip.HipText(d_text=0, nbytes=0, delim=0x0A)):
        assert empty.lines == 0 and empty.offsets().tolist() == [0]
        empty.exec(ld, ids_mode=1, out=out)
        empty.exec_device(ld, 0, 0, 0, 0, 0)
        assert all(np.array_equal(out[k], keep[k]) for k in out)
    # a single 100 KB line without a delimiter: n == 1 and the right answer (accepted: "a" * 100000; rejected: a 'b' in it)
    for body, want_ret in ((b"a" * 100000, 1), (b"a" * 70000 + b"b" + b"a" * 29999, 0)):
        big = hip.HipText(body, 0x0A)
        assert big.lines == 1 and big.offsets().tolist() == [0, 100000]
        ret, end, _, _ = oracle_answers(flat, [body])
        assert int(ret[0]) == want_ret
        got = big.exec(ld, want_bitmap=True)
        assert np.array_equal(got["end"], end) and int(got["bitmap"][0]) == want_ret
    with pytest.raises(OSError) as ei:
        hip.HipText(b"abc", 256)
    assert ei.value.errno == errno.EINVAL


def test_example_prints_what_hipgrep_prints(hip, tmp_path):
    """examples/hipgrep_text.c (no host loop over the bytes) against examples/hipgrep.c, built the way test_gpu_parity.py builds
    the latter: identical output on a table written by fsm_hip_desc_write and a file with empty lines and no final newline"""
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
    outs = {}
    for prog in ("hipgrep", "hipgrep_text"):
        exe = str(tmp_path / prog)
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-I" + os.path.join(root, "include"),
                               os.path.join(root, "examples", prog + ".c"), "-o", exe,
                               "-L" + os.path.join(root, "libfsm_amd"), "-lfsm_hip", "-Wl,-rpath," + os.path.join(root, "libfsm_amd")])
        r = subprocess.run([exe, table], input=data, capture_output=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr
        outs[prog] = r.stdout
    assert outs["hipgrep_text"] == outs["hipgrep"]
    ret, end, ids, _ = oracle_answers(det.flat, lines)
    want = [f"{i + 1}:" + ",".join(str(x) for x in ids[i]) for i in range(len(lines)) if ret[i] == 1]
    assert outs["hipgrep_text"].decode().split() == want and len(want) >= 10
