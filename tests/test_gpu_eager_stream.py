"""GPU (-m gpu): eager-output sets for resumed walks (fsm_hip_exec_batch_eager_resume[_device]) and for one big input walked by
the whole device (fsm_hip_match_buffer_big_eager / fsm_hip_match_file_eager).  Everything is compared with the oracle's
fsm_exec + callback over the whole input as ONE input (oracle.pyoracle.Oracle.exec_eager)."""
import ctypes as C
import errno as _errno
import os

import numpy as np
import pytest

from common import GOLDEN

pytestmark = pytest.mark.gpu
NO = 0xFFFFFFFF
START = 0xFFFFFFFD
DEAD = 0xFFFFFFFC
WIN = 32 << 20
LOWER = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()   # raises if the HIP extension is missing: no silent fallback
    return libfsm_amd


def _need_ref():
    from oracle.pyoracle import have_ref
    if not have_ref():
        pytest.skip("oracle/_ref not present")


def _eager40(hip):
    z = np.load(os.path.join(GOLDEN, "bench", "eager40.npz"))
    return hip.FlatDfa.load(z), bytes(z["patterns"]).split(b"\n")


def _union150(hip):
    """fsm_union_repeated_pattern_group over 150 unanchored literals of 6-8 letters: 150 eager ids, W = 3 (the wide sets)"""
    _need_ref()
    from oracle.pyoracle import RefFsm
    rng = np.random.RandomState(150)
    words = []
    while len(words) < 150:
        w = bytes(LOWER[rng.randint(0, 26, rng.randint(6, 9))])
        if w not in words:
            words.append(w)
    f = RefFsm.union_repeated("pcre", words, 1, False)
    return f.flatten(), words


def _want(flat, data: bytes, cap: int):
    """the oracle over the whole input: (ret, end, sorted ids, final state or DEAD)"""
    from oracle.pyoracle import Oracle
    o = Oracle(flat)
    row = np.frombuffer(data, np.uint8)[None, :] if len(data) else np.zeros((1, 0), np.uint8)
    ret, end, sets = o.exec_eager(row, cap=cap)
    st = o.state_walk(row, np.array([START], np.uint32))[0]
    return int(ret[0]), int(end[0]), sets[0], int(st)


def _ids(dfa, words):
    return dfa._eager_ids_of(np.asarray(words, np.uint64))


def _text(rng, pats, n):
    """random lowercase text with patterns planted every ~100 bytes; returns (bytes, planted start positions)"""
    t = bytearray(bytes(LOWER[rng.randint(0, 26, n)]))
    at = []
    pos = int(rng.randint(0, 60))
    while pos < n:
        p = pats[rng.randint(len(pats))]
        t[pos:pos + len(p)] = p
        at.append((pos, len(p)))
        pos += len(p) + int(rng.randint(20, 200))
    return bytes(t[:n]), at


def _cuts(rng, n, planted):
    """1-5 pieces: cut points that include empty pieces, cuts inside a planted pattern and a cut right after the first byte"""
    k = int(rng.randint(1, 6))
    cand = [0, n, n]
    if n:
        cand.append(1)
    inside = [p + int(rng.randint(1, max(2, L))) for p, L in planted if p + L <= n]
    if inside:
        cand += [inside[rng.randint(len(inside))] for _ in range(2)]
    cand += [int(x) for x in rng.randint(0, n + 1, 3)]
    cuts = sorted(int(rng.choice(cand)) for _ in range(k - 1))
    return [0] + cuts + [n]


def _run_pieces(hip, dfa, texts, cuts, form, W):
    """every input's pieces through successive resume calls; form: (host | device) x (stride | off)"""
    import torch
    n = len(texts)
    npieces = max(len(c) - 1 for c in cuts)
    st = np.full(n, START, np.uint32)
    eo = np.zeros(n * W, np.uint64)
    end = np.full(n, NO, np.uint32)
    dev = form[0] == "device"
    if dev:
        d_st = torch.from_numpy(st.view(np.int32).copy()).cuda()
        d_eo = torch.zeros(n * W, dtype=torch.int64, device="cuda")
        d_end = torch.empty(n, dtype=torch.int32, device="cuda")
    for j in range(npieces):
        pieces = [t[c[j]:c[j + 1]] if j + 1 < len(c) else b"" for t, c in zip(texts, cuts)]
        if form[1] == "off":
            off = np.zeros(n + 1, np.uint64)
            off[1:] = np.cumsum([len(p) for p in pieces])
            base = np.frombuffer(b"".join(pieces) or b"\0", np.uint8).copy()
            if dev:
                d_base, d_off = torch.from_numpy(base).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
                dfa.exec_batch_eager_resume_device(d_base.data_ptr(), 0, n, d_st.data_ptr(), d_eo.data_ptr(), d_off=d_off.data_ptr(),
                                                   d_end=d_end.data_ptr())
                torch.cuda.synchronize()
            else:
                st, end, eo = dfa.exec_batch_eager_resume(base, st, eo, off=off)
        else:
            stride = max(16, (max(len(p) for p in pieces) + 15) // 16 * 16)
            rows = np.zeros((n, stride), np.uint8)
            lens = np.array([len(p) for p in pieces], np.uint32)
            for i, p in enumerate(pieces):
                rows[i, :len(p)] = np.frombuffer(p, np.uint8)
            if dev:
                d_rows, d_len = torch.from_numpy(rows).cuda(), torch.from_numpy(lens.view(np.int32)).cuda()
                dfa.exec_batch_eager_resume_device(d_rows.data_ptr(), stride, n, d_st.data_ptr(), d_eo.data_ptr(), d_len=d_len.data_ptr(),
                                                   d_end=d_end.data_ptr())
                torch.cuda.synchronize()
            else:
                st, end, eo = dfa.exec_batch_eager_resume(rows, st, eo, lens=lens)
    if dev:
        st = d_st.cpu().numpy().view(np.uint32)
        eo = d_eo.cpu().numpy().view(np.uint64)
        end = d_end.cpu().numpy().view(np.uint32)
    return st, end, eo.reshape(n, W)


FORMS = [("host", "stride"), ("host", "off"), ("device", "stride"), ("device", "off")]


def _check_resume(hip, flat, pats, seed, layouts=(0,)):
    rng = np.random.RandomState(seed)
    texts, cuts = [], []
    for i in range(48):
        t, at = _text(rng, pats, int(rng.randint(0, 1500)) if i % 8 else int(rng.randint(0, 4)))
        texts.append(t)
        cuts.append(_cuts(rng, len(t), at))
    cap = len(flat.eager_ids) + 8
    want = [_want(flat, t, cap) for t in texts]
    assert sum(len(w[2]) for w in want) > 100
    checked = 0
    for L in layouts:
        try:
            dfa = hip.HipDfa(flat, L)
        except OSError:
            continue
        W = dfa.eager_words()
        for form in FORMS:
            st, end, eo = _run_pieces(hip, dfa, texts, cuts, form, W)
            for i, (ret, wend, wset, wst) in enumerate(want):
                assert np.array_equal(_ids(dfa, eo[i]), wset), (L, form, i, texts[i][:60], cuts[i])
                assert st[i] == wst, (L, form, i)
                assert end[i] == wend, (L, form, i)
            checked += 1
        dfa.close()
    assert checked >= 4


def test_resume_property_eager40(hip):
    """W = 1: zero eager_io, state_io = START, pieces fed one call each -> the set, state and end of fsm_exec over the
    concatenation; stride + len and offsets forms, host and device; the automaton in several layouts (their resumed eager
    kernels)."""
    flat, pats = _eager40(hip)
    _check_resume(hip, flat, pats, 1, (0, hip.LAYOUT_LDS, hip.LAYOUT_COMBSELF, hip.LAYOUT_COMB256, hip.LAYOUT_GLOBAL, hip.LAYOUT_SPARSE))


def test_resume_property_wide(hip):
    """the same over 150 eager ids (W = 3: the wide sets, which the resumed walk must not zero)"""
    flat, words = _union150(hip)
    h = hip.HipDfa(flat)
    assert h.eager_words() == 3
    h.close()
    _check_resume(hip, flat, words, 2, (0, hip.LAYOUT_GLOBAL))


def _start_emits(hip):
    """0 (start, emits 7) -a-> 1 (emits 9) -a-> 1; 'b' from 0 or 1 -> 2 (no outputs); nothing else"""
    nt = np.full((3, 256), -1, np.int64)
    nt[0, ord("a")] = 1
    nt[1, ord("a")] = 1
    nt[0, ord("b")] = nt[1, ord("b")] = 2
    return hip.FlatDfa.from_dense(nt, 0, [0, 1, 1], eager_off=[0, 1, 2, 2], eager_ids=[7, 9])


def test_start_state_outputs(hip):
    """From START with 0 bytes exactly the start state's outputs; from the start state's own id, or from DEAD, nothing."""
    flat = _start_emits(hip)
    dfa = hip.HipDfa(flat)
    rows = np.zeros((4, 16), np.uint8)
    rows[3, :2] = np.frombuffer(b"aa", np.uint8)
    lens = np.array([0, 0, 0, 2], np.uint32)
    st, end, eo = dfa.exec_batch_eager_resume(rows, np.array([START, 0, DEAD, 0], np.uint32), np.zeros(4, np.uint64), lens=lens)
    assert [list(_ids(dfa, eo[i:i + 1])) for i in range(4)] == [[7], [], [], [9]]
    assert list(st) == [0, 0, DEAD, 1]
    assert list(end) == [NO, NO, NO, 1]
    # what was already in eager_io stays: the call only adds
    st, end, eo = dfa.exec_batch_eager_resume(rows[:1], np.array([DEAD], np.uint32), np.array([1 << 1], np.uint64), lens=lens[:1])
    assert list(_ids(dfa, eo)) == [9]
    # the big-input front: empty, small and > 256 KiB inputs
    for data in (b"", b"b", b"a" * 300_000, b"a" * 300_000 + b"b"):
        ret, wend, wset, _ = _want(flat, data, 8)
        r, e, ids = dfa.match_buffer_big_eager(data)
        assert (r, e) == (ret, wend) and np.array_equal(ids, wset), len(data)
    dfa.close()


def test_missing_edge_stops_the_set(hip):
    """A start-anchored eager union (a match leads to a state that accepts every suffix, so only a missing edge before one
    ends the walk) whose input has a missing edge in piece 2: the state is DEAD from there on and the pieces after it add
    nothing, though each of them, walked from START, would fire an output."""
    _need_ref()
    from oracle.pyoracle import RefFsm
    pats = [b"^abc[0-9]+x", b"^q[0-9]+y", b"^zz"]
    f = RefFsm.union_repeated("pcre", pats, 1, False)
    flat = f.flatten()
    dfa = hip.HipDfa(flat)
    pieces = [b"ab", b"c12", b"3Zq1y", b"abc1x", b"zz"]
    ret, wend, wset, wst = _want(flat, b"".join(pieces), 16)
    assert (ret, wend, wst, list(wset)) == (0, NO, DEAD, [])
    for p, want_id in ((b"abc1x", 1), (b"zz", 3), (b"q1y", 2)):
        assert list(_want(flat, p, 16)[2]) == [want_id], p   # alone, from START, they do emit
    for L in (0, hip.LAYOUT_COMBSELF, hip.LAYOUT_GLOBAL):
        try:
            d = hip.HipDfa(flat, L)
        except OSError:
            continue
        st, eo = np.array([START, START], np.uint32), np.zeros(2, np.uint64)
        after = []
        for p in pieces:
            rows = np.zeros((2, 16), np.uint8)
            rows[:, :len(p)] = np.frombuffer(p, np.uint8)
            st, end, eo = d.exec_batch_eager_resume(rows, st, eo, lens=np.array([len(p), len(p)], np.uint32))
            after.append((int(st[0]), list(_ids(d, eo[:1])), int(end[0])))
        assert after[0][0] != DEAD and after[1][0] != DEAD
        assert after[2] == after[3] == after[4] == (DEAD, [], NO), (L, after)
        d.close()
    dfa.close()


def _plant(data: np.ndarray, at: int, p: bytes):
    at = max(0, min(at, len(data) - len(p)))
    data[at:at + len(p)] = np.frombuffer(p, np.uint8)


def _check_big(hip, dfa, flat, data: np.ndarray, tmp_path, cap):
    raw = data.tobytes()
    ret, wend, wset, _ = _want(flat, raw, cap)
    r, e, ids = dfa.match_buffer_big_eager(raw)
    w, p = dfa.match_last_passes()
    assert (r, e) == (ret, wend), len(raw)
    assert np.array_equal(ids, wset), (len(raw), sorted(set(wset) ^ set(ids)))
    if len(raw) >= WIN:
        assert p <= 3 * w, (len(raw), w, p)
    path = str(tmp_path / "in.bin")
    data.tofile(path)
    assert _same(dfa.match_file_eager(path), (r, e, ids)), len(raw)
    os.unlink(path)
    return wset


def _same(a, b):
    return a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])


def _fill_pieces(rng, data: np.ndarray, words):
    """one of `words` inside every 1 KiB piece.  These union automata remember whether some pattern has matched (their end
    states), so a piece guessed from the start state is right only once it contains a match of its own: without one in every
    piece the fixed point is reached one piece per pass, for the plain walk as for this one (out of scope here)."""
    for j in range(len(data) // 1024):
        w = words[rng.randint(len(words))]
        at = j * 1024 + 8 + int(rng.randint(0, 1000 - len(w)))
        data[at:at + len(w)] = np.frombuffer(w, np.uint8)


def test_big_input_eager40(hip, tmp_path):
    """W = 1 over 300 KB .. 64 MiB + 77 777 B (below a window, one, a window and a byte, two and a tail), 7-letter patterns
    planted across a 1 KiB piece boundary, the 32 MiB window boundary and the tail: r, end and the set of fsm_exec; at most 3
    passes a window; the file form = the buffer form."""
    flat, pats = _eager40(hip)
    long_ = [p for p in pats if len(p) == 7]
    short = [p for p in pats if len(p) < 7]
    dfa = hip.HipDfa(flat)
    rng = np.random.RandomState(44)
    for k, size in enumerate((300_000, 1 << 20, WIN - 1024, WIN, WIN + 1, 2 * WIN + 77_777)):
        data = LOWER[rng.randint(0, 26, size, dtype=np.uint8)]
        _fill_pieces(rng, data, short)
        planted = [(1024 * 5 - 3, long_[k % len(long_)]),                               # across a piece boundary
                   ((size // 1024) * 1024 - 3, long_[(k + 1) % len(long_)]),             # the last whole piece into the tail
                   (size - 7, long_[(k + 2) % len(long_)])]                              # the last bytes
        if size >= WIN + 8:
            planted.append((WIN - 4, long_[(k + 3) % len(long_)]))                       # across the window boundary
        kept = []
        for at, p in planted:
            at = max(0, min(at, size - len(p)))
            if all(at + len(p) <= a or a + len(q) <= at for a, q in kept):             # (a size that is a whole number of pieces: no tail)
                _plant(data, at, p)
                kept.append((at, p))
        planted = kept
        wset = set(_check_big(hip, dfa, flat, data, tmp_path, 48).tolist())
        for at, p in planted:
            assert _eager_id_of(flat, p, pats) in wset, (size, at, p)
    dfa.close()


def _eager_id_of(flat, p, pats):
    # tests/golden/make_eager40.py: eager id of pattern k = k + 1
    return pats.index(p) + 1


def test_big_input_wide_sets(hip, tmp_path):
    """150 eager ids (W = 3) over ~40 MiB: 100 of the words inside the pieces, the other 50 planted across piece boundaries,
    the window boundary and the tail."""
    flat, words = _union150(hip)
    dfa = hip.HipDfa(flat)
    assert dfa.eager_words() == 3
    rng = np.random.RandomState(45)
    size = 40 * (1 << 20) + 333
    data = LOWER[rng.randint(0, 26, size, dtype=np.uint8)]
    _fill_pieces(rng, data, words[:100])
    spots = [int(x) * 1024 - 3 for x in rng.choice(np.arange(1, size // 1024), 47, replace=False)] + [WIN - 3, (size // 1024) * 1024 - 4, size - 9]
    for at, w in zip(spots, words[100:]):
        _plant(data, at, w)
    wset = set(_check_big(hip, dfa, flat, data, tmp_path, 160).tolist())
    assert set(range(101, 151)) <= wset
    dfa.close()


def test_guesses_that_emit_wrong_ids_are_discarded(hip):
    """An automaton that does not forget: the parity of a run of 'a'; 'b' from even parity enters a state with id 100, 'b'
    from odd parity one with id 200.  Every 'b' of the input comes at odd parity, so fsm_exec emits 200 only; a piece guessed
    from the start (even) state emits 100 at its 'b's.  Those sets must be thrown away."""
    nt = np.full((4, 256), -1, np.int64)
    nt[0, ord("a")], nt[1, ord("a")], nt[2, ord("a")], nt[3, ord("a")] = 1, 0, 1, 0
    nt[0, ord("b")], nt[1, ord("b")], nt[2, ord("b")], nt[3, ord("b")] = 2, 3, 2, 3
    flat = hip.FlatDfa.from_dense(nt, 0, [1, 1, 1, 1], eager_off=[0, 0, 0, 1, 2], eager_ids=[100, 200])
    rng = np.random.RandomState(46)
    parts = [b"a" * 1001]
    n = 1001
    while n < 330_000:
        L = 2 * int(rng.randint(0, 1500))
        parts.append(b"b" + b"a" * L)
        n += L + 1
    data = b"".join(parts)
    ret, wend, wset, _ = _want(flat, data, 8)
    assert list(wset) == [200]
    dfa = hip.HipDfa(flat)
    r, e, ids = dfa.match_buffer_big_eager(data)
    w, p = dfa.match_last_passes()
    assert w >= 1 and p > 2     # the guesses were wrong: more passes than one correction
    assert (r, e) == (ret, wend) and list(ids) == [200]
    dfa.close()


def test_arguments(hip, tmp_path):
    """NULL eager_out / eager_io / state_io give EINVAL; so do decreasing host offsets."""
    flat, _ = _eager40(hip)
    dfa = hip.HipDfa(flat)
    lib = dfa._lib
    vp = C.c_void_p
    buf = C.create_string_buffer(b"abc")
    e = C.c_uint32(0)
    C.set_errno(0)
    assert lib.fsm_hip_match_buffer_big_eager(vp(dfa._h), buf, C.c_size_t(3), C.byref(e), None) == -1
    assert C.get_errno() == _errno.EINVAL
    p = tmp_path / "f.bin"
    p.write_bytes(b"abc")
    with pytest.raises(OSError) as ei:
        _match_file_null(dfa, str(p))
    assert ei.value.errno == _errno.EINVAL
    st = np.array([START], np.uint32)
    eo = np.zeros(1, np.uint64)
    C.set_errno(0)
    assert lib.fsm_hip_exec_batch_eager_resume(vp(dfa._h), buf, C.c_size_t(3), None, None, C.c_size_t(1), st.ctypes.data_as(vp), None, None) == -1
    assert C.get_errno() == _errno.EINVAL
    C.set_errno(0)
    assert lib.fsm_hip_exec_batch_eager_resume(vp(dfa._h), buf, C.c_size_t(3), None, None, C.c_size_t(1), None, None, eo.ctypes.data_as(vp)) == -1
    assert C.get_errno() == _errno.EINVAL
    C.set_errno(0)
    assert lib.fsm_hip_exec_batch_eager_resume_device(vp(dfa._h), None, C.c_size_t(16), None, None, C.c_size_t(1), None, None, None, None) == -1
    assert C.get_errno() == _errno.EINVAL
    off = np.array([0, 3, 1], np.uint64)
    with pytest.raises(OSError) as ei:
        dfa.exec_batch_eager_resume(np.frombuffer(b"abc", np.uint8), np.full(2, START, np.uint32), np.zeros(2, np.uint64), off=off)
    assert ei.value.errno == _errno.EINVAL
    dfa.close()


def _match_file_null(dfa, path):
    libc = C.CDLL(None, use_errno=True)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    f = libc.fopen(path.encode(), b"rb")
    try:
        C.set_errno(0)
        r = dfa._lib.fsm_hip_match_file_eager(C.c_void_p(dfa._h), C.c_void_p(f), None, None)
    finally:
        libc.fclose(f)
    if r < 0:
        raise OSError(C.get_errno(), "fsm_hip_match_file_eager")
    return r
