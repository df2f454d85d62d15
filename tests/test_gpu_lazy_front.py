"""GPU (-m gpu): the lazy walks of the sparse layout -- walk_lazy (fixed stride) and walk_lazy_lines (whole chunks + tail queue:
every variable-length front, resumed walks, end-ids) of walk_lazy.h -- on automata in which absorbing states are reached
(unanchored literal sets without end-ids: the absorbing accept; rewired tries: DEAD), on automata that are no tries (states
entered with the all-sentinel record, exceptions that are no progression), and at the kernel's own line edges: lines that are
all tail, lines without a tail, 16 * NB bytes and one to either side, a tail that ends at the text's last byte, batch sizes
around the 192 slots of a wavefront and the 256 lines of a piece.

Automata, lines and every expected answer are tests/lazy_front_ref.py: a plain numpy walk of FlatDfa.dense() in the caller's
numbering (global_ref.trace / ends / carried).  Nothing is compared with the planner, another layout, another knob setting or
another front.  tests/test_lazy_front_cases.py shows on the CPU that the lines reach what they are for.  After every launch
the kernel that ran (fsm_hip_last_kernel_name) is asserted: the template and its ABS argument."""
import re

import numpy as np
import pytest

import global_ref as G
import lazy_front_ref as R

pytestmark = pytest.mark.gpu

NO = 0xFFFFFFFF
JUNK32, JUNK8 = 0x5A5A5A5A, 0xA5
KERNEL = re.compile(r"walk_lazy(_lines)?<([^<>]*)>")


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()
    assert G.LIB_DEAD == libfsm_amd.STATE_DEAD and G.LIB_START == libfsm_amd.STATE_START and R.NO_ID == libfsm_amd.NO_ID
    return libfsm_amd


@pytest.fixture(scope="module")
def dfas(hip):
    """one handle per (automaton, flags), opened at its first use; the automata that meet the auto-lazy rule get no knob: the
    lazy walk must be what they launch"""
    made = {}

    def get(name, flags=0):
        if (name, flags) not in made:
            d = hip.HipDfa(R.case(name).flat, hip.LAYOUT_SPARSE | flags)
            assert d.info()["layout_name"] == "sparse"
            if not R.SPEC[name]["auto"]:
                d.tune(hip.KNOB_SPARSE_FAST, 3)
            made[(name, flags)] = d
        return made[(name, flags)]

    yield get
    for d in made.values():
        d.close()


class knobs:
    """knob settings for the length of a block; every one goes back to its default"""
    DEFAULT = {"KNOB_ROWS": 0, "KNOB_NB": 0, "KNOB_EARLY_RETIRE": -1, "KNOB_LAZY_DYN": 1, "KNOB_NT": -1}

    def __init__(self, hip, dfa, **kw):
        self.hip, self.dfa, self.kw = hip, dfa, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.dfa.tune(getattr(self.hip, k), v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.dfa.tune(getattr(self.hip, k), self.DEFAULT[k])


def ran(dfa, lines, abs_, rest=None):
    """the kernel of the last launch: walk_lazy_lines or walk_lazy, its ABS argument, and (rest) the arguments behind it"""
    kn = dfa.last_kernel_name()
    m = KERNEL.search(kn)
    assert m is not None and bool(m.group(1)) == lines, kn
    args = [x.strip() for x in m.group(2).split(",")]
    assert args[0] == ("true" if abs_ else "false"), kn
    if rest is not None:
        assert args[1:1 + len(rest)] == [str(x).lower() for x in rest], (kn, rest)
    return kn


def same(got, want, *tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError((tag, f"{len(bad)} of {len(want)} differ", bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist()))


def words_of(end):
    """the accept bitmap of these end states: bit i of word i / 64, spare bits zero"""
    n = len(end)
    bits = np.zeros((n + 63) // 64 * 64, np.uint8)
    bits[:n] = np.asarray(end) != NO
    return np.packbits(bits, bitorder="little").view(np.uint64) if n else np.zeros(0, np.uint64)


# ---- device buffers ------------------------------------------------------------------------------------------------------

def to_dev(a):
    """the array's bytes on the device, in a buffer of exactly that size (one byte where there are none)"""
    import torch
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(b.copy()).cuda() if b.size else torch.zeros(1, dtype=torch.uint8, device="cuda")


class Out:
    """end_out and the accept bitmap on the device, two entries / two words longer than the batch, pre-filled (the bitmap with
    zeros, or with junk: the variable-length kernel ORs into it, so the front must have cleared the batch's words)"""

    def __init__(self, n, junk_bitmap=False, state=None):
        import torch
        self.n, self.words, self.fill = n, (n + 63) // 64, JUNK8 if junk_bitmap else 0
        self.end = torch.full(((n + 2) * 4,), 0x5A, dtype=torch.uint8, device="cuda")
        self.bm = torch.full(((self.words + 2) * 8,), self.fill, dtype=torch.uint8, device="cuda")
        self.state = None if state is None else to_dev(np.concatenate([np.asarray(state, np.uint32), np.full(2, JUNK32, np.uint32)]))

    def check(self, want_end, *tag, want_state=None):
        import torch
        torch.cuda.synchronize()
        end = self.end.cpu().numpy().view(np.uint32)
        bm = self.bm.cpu().numpy().view(np.uint64)
        same(end[:self.n], want_end, *tag, "end")                        # every entry written ...
        assert (end[self.n:] == JUNK32).all(), (tag, "written behind end_out")
        same(bm[:self.words], words_of(want_end), *tag, "bitmap")        # ... spare bits of the last word zero ...
        assert (bm[self.words:] == int.from_bytes(bytes([self.fill]) * 8, "little")).all(), (tag, "written behind the bitmap")
        if want_state is not None:
            st = self.state.cpu().numpy().view(np.uint32)
            same(st[:self.n], want_state, *tag, "state_io")
            assert (st[self.n:] == JUNK32).all(), (tag, "written behind state_io")


def host_words(bm, want_end, *tag):
    same(bm, words_of(want_end), *tag, "bitmap")


# ---- 1. the variable-length fronts, default knobs --------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.NAMES)
def test_variable_length_fronts(hip, dfas, name):
    """u64 offsets (once from off[0] = 5), u32 offsets, lengths alone, rows + lengths, strides of 72 and 100 without lengths; host
    and device pointers (device texts of exactly off[n] bytes); every batch size, the last line's tail of 0, 1, 7 and 15 bytes in turn"""
    c, dfa = R.case(name), dfas(name)
    abs_ = c.has_abs
    for k, n in enumerate(R.SIZES + (c.FULL,)):
        tail = R.TAILS[(k + 1) % 4] if n != c.FULL else 7
        idx = c.batch(n, tail)
        base, off = c.packed(idx)
        lens, want = c.lens[idx], c.end[idx]
        tag = (name, n, tail)
        # host pointers
        end, bm = dfa.exec_batch_offsets(base, off)
        ran(dfa, True, abs_, (3, 3, 2))
        same(end, want, *tag, "u64 offsets")
        host_words(bm, want, *tag, "u64 offsets")
        end, bm = dfa.exec_batch_offsets(np.concatenate([np.full(5, 0x61, np.uint8), base]), off + np.uint64(5))
        same(end, want, *tag, "u64 offsets from 5")
        host_words(bm, want, *tag, "u64 offsets from 5")
        end, bm = dfa.exec_batch_offsets32(base, off.astype(np.uint32))
        ran(dfa, True, abs_)
        same(end, want, *tag, "u32 offsets")
        host_words(bm, want, *tag, "u32 offsets")
        end, bm = dfa.exec_batch_lengths(base, lens)
        ran(dfa, True, abs_)
        same(end, want, *tag, "lengths")
        host_words(bm, want, *tag, "lengths")
        end, bm = dfa.exec_batch(c.rows[idx], lens)
        ran(dfa, True, abs_)
        same(end, want, *tag, "rows + lengths")
        host_words(bm, want, *tag, "rows + lengths")
        for stride in (72, 100):
            rows, _, fend = c.fixed(stride)
            m = min(n, len(rows))
            end, bm = dfa.exec_batch(rows[:m])
            ran(dfa, True, abs_)
            same(end, fend[:m], *tag, "stride", stride)
            host_words(bm, fend[:m], *tag, "stride", stride)
        # device pointers
        d_base, d_off, d_off32, d_len = to_dev(base), to_dev(off), to_dev(off.astype(np.uint32)), to_dev(lens)
        assert d_base.numel() == max(int(off[-1]), 1)
        for junk in (False, True):
            o = Out(n, junk)
            dfa.exec_batch_offsets_device(d_base.data_ptr(), d_off.data_ptr(), n, o.end.data_ptr(), o.bm.data_ptr())
            ran(dfa, True, abs_)
            o.check(want, *tag, "device u64 offsets", junk)
        o = Out(n, True)
        dfa.exec_batch_offsets32_device(d_base.data_ptr(), d_off32.data_ptr(), n, o.end.data_ptr(), o.bm.data_ptr())
        o.check(want, *tag, "device u32 offsets")
        o = Out(n, True)
        dfa.exec_batch_lengths_device(d_base.data_ptr(), d_len.data_ptr(), n, o.end.data_ptr(), o.bm.data_ptr())
        ran(dfa, True, abs_)
        o.check(want, *tag, "device lengths")
        d5, d_off5 = to_dev(np.concatenate([np.full(5, 0x61, np.uint8), base])), to_dev(off + np.uint64(5))
        o = Out(n)
        dfa.exec_batch_offsets_device(d5.data_ptr(), d_off5.data_ptr(), n, o.end.data_ptr(), o.bm.data_ptr())
        o.check(want, *tag, "device u64 offsets from 5")
        d_rows = to_dev(c.rows[idx])
        o = Out(n, True)
        dfa.exec_batch_device(d_rows.data_ptr(), R.WIDTH, n, o.end.data_ptr(), o.bm.data_ptr(), d_len.data_ptr())
        ran(dfa, True, abs_)
        o.check(want, *tag, "device rows + lengths")
        rows, _, fend = c.fixed(100)
        m = min(n, len(rows))
        o, d_rows = Out(m, True), to_dev(rows[:m])
        dfa.exec_batch_device(d_rows.data_ptr(), 100, m, o.end.data_ptr(), o.bm.data_ptr())
        ran(dfa, True, abs_)
        o.check(fend[:m], *tag, "device stride 100")


# ---- 2. every instantiation a knob reaches ---------------------------------------------------------------------------------

def _three_fronts(dfa, c, idx, abs_, rest, *tag):
    base, off = c.packed(idx)
    want = c.end[idx]
    end, bm = dfa.exec_batch_offsets(base, off)
    ran(dfa, True, abs_, rest)
    same(end, want, *tag, "u64 offsets")
    host_words(bm, want, *tag, "u64 offsets")
    end, bm = dfa.exec_batch_lengths(base, c.lens[idx])
    ran(dfa, True, abs_, rest)
    same(end, want, *tag, "lengths")
    end, bm = dfa.exec_batch(c.rows[idx], c.lens[idx])
    ran(dfa, True, abs_, rest)
    same(end, want, *tag, "rows + lengths")
    host_words(bm, want, *tag, "rows + lengths")


@pytest.mark.parametrize("name", R.NAMES)
def test_every_instantiation_of_the_lines_kernel(hip, dfas, name):
    """walk_lazy_lines<ABS, 2, 2>, <ABS, 2, 4>, <ABS, 3, 2, 8>, <ABS, 3, 4, 2> and the shipped <ABS, 3, 3, 2> on the three blocks
    together; early retire off and on by knob, and off by flag: there the ABS step alone keeps an absorbing state, through every
    later chunk and the queue"""
    c, dfa = R.case(name), dfas(name)
    abs_ = c.has_abs
    for tail in (7, 0):
        idx = c.batch(c.FULL, tail)
        for rows, nb, rest in ((2, 2, (2, 2)), (2, 4, (2, 4)), (0, 2, (3, 2, 8)), (0, 4, (3, 4, 2)), (0, 0, (3, 3, 2))):
            with knobs(hip, dfa, KNOB_ROWS=rows, KNOB_NB=nb):
                _three_fronts(dfa, c, idx, abs_, rest, name, tail, rest)
    idx = c.batch(c.FULL, 15)
    for early in (0, 1):
        for rows, nb, rest in ((0, 0, (3, 3, 2)), (2, 4, (2, 4))):
            with knobs(hip, dfa, KNOB_EARLY_RETIRE=early, KNOB_ROWS=rows, KNOB_NB=nb):
                _three_fronts(dfa, c, idx, abs_, rest, name, "early retire", early, rest)
    keep = dfas(name, hip.NO_EARLY_RETIRE)
    _three_fronts(keep, c, idx, abs_, (3, 3, 2), name, "NO_EARLY_RETIRE")
    for n in (193, 257):
        _three_fronts(keep, c, c.batch(n, 1), abs_, (3, 3, 2), name, "NO_EARLY_RETIRE", n)


# ---- 3. fixed stride: walk_lazy ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", (64, 128, 192, 1024))
@pytest.mark.parametrize("name", R.NAMES)
def test_fixed_stride(hip, dfas, name, stride):
    """walk_lazy<ABS, 3, 4> on rows of 64, 128, 192 and 1 024 bytes (the hand-made lines first, padded with live text), every batch
    size, host and device pointers; then static striding, two rows a lane, nontemporal loads, early retire off and on"""
    c, dfa = R.case(name), dfas(name)
    abs_ = c.has_abs
    rows, _, fend = c.fixed(stride)
    for n in R.SIZES + (len(rows),):
        end, bm = dfa.exec_batch(rows[:n])
        ran(dfa, False, abs_, (3, 4, "false"))
        same(end, fend[:n], name, stride, n)
        host_words(bm, fend[:n], name, stride, n)
        o, d_rows = Out(n, True), to_dev(rows[:n])
        dfa.exec_batch_device(d_rows.data_ptr(), stride, n, o.end.data_ptr(), o.bm.data_ptr())
        ran(dfa, False, abs_, (3, 4, "false"))
        o.check(fend[:n], name, stride, n, "device")
    for kw, rest in ((dict(KNOB_LAZY_DYN=0), (3, 4, "false")), (dict(KNOB_ROWS=2), (2, 4, "false")), (dict(KNOB_ROWS=2, KNOB_NT=1), (2, 4, "true")),
                     (dict(KNOB_ROWS=2, KNOB_LAZY_DYN=0), (2, 4, "false")), (dict(KNOB_EARLY_RETIRE=0), (3, 4, "false")),
                     (dict(KNOB_EARLY_RETIRE=1), (3, 4, "false")), (dict(KNOB_EARLY_RETIRE=0, KNOB_ROWS=2), (2, 4, "false"))):
        with knobs(hip, dfa, **kw):
            for n in (127, 193, len(rows)):
                end, bm = dfa.exec_batch(rows[:n])
                ran(dfa, False, abs_, rest)
                same(end, fend[:n], name, stride, n, kw)
                host_words(bm, fend[:n], name, stride, n, kw)
    keep = dfas(name, hip.NO_EARLY_RETIRE)
    end, bm = keep.exec_batch(rows)
    ran(keep, False, abs_, (3, 4, "false"))
    same(end, fend, name, stride, "NO_EARLY_RETIRE")


# ---- 4. resumed walks -------------------------------------------------------------------------------------------------------

def _resume(hip, dfa, front, rows, lens, state):
    """one piece of every line through one of the resumed fronts -> (state_out, end)"""
    base, off = G.packed(rows, lens)
    n = len(lens)
    if front == "offsets":
        return dfa.exec_offsets_resume(base, off, state)
    if front == "packed u64":
        return dfa.exec_packed_resume(base, hip.META_OFF64, off, n, state)
    if front == "packed u32":
        return dfa.exec_packed_resume(base, hip.META_OFF32, off.astype(np.uint32), n, state)
    if front == "packed lengths":
        return dfa.exec_packed_resume(base, hip.META_LENGTHS, np.ascontiguousarray(lens, np.uint32), n, state)
    assert front == "rows"
    return dfa.exec_batch_resume(rows, state, lens)


FRONTS = ("offsets", "packed u64", "packed u32", "packed lengths", "rows")


@pytest.mark.parametrize("name", R.NAMES)
def test_resumed_in_two_pieces(hip, dfas, name):
    """every line cut at a random byte, at byte 16, 32 and 48, and at 0: the states carried after the first piece are the
    reference's, in the caller's ids (never a clone's); the second piece ends where the whole line ends.  A resumed walk may be
    handed DEAD, so the kernel is the ABS one on every automaton."""
    c, dfa = R.case(name), dfas(name)
    for k, kind in enumerate(R.CUTS):
        idx = c.batch(c.FULL if kind == "random" else 513, R.TAILS[k % 4])
        n = len(idx)
        cut = c.cut[kind][idx]
        mid = c.state_at(idx, cut)
        rest_rows, rest_lens = c.rest(idx, cut)
        for front in (FRONTS if kind == "random" else (FRONTS[k % 5], "rows")):
            tag = (name, kind, front)
            st, end = _resume(hip, dfa, front, c.rows[idx], cut, np.full(n, hip.STATE_START, np.uint32))
            ran(dfa, True, True, (3, 3, 2))
            same(st, G.carried(mid), *tag, "carried after the first piece")
            assert ((st < c.S) | (st == hip.STATE_DEAD)).all(), tag
            same(end, G.ends(c.flat, mid), *tag, "end after the first piece")
            st2, end2 = _resume(hip, dfa, front, rest_rows, rest_lens, st)
            ran(dfa, True, True)
            same(end2, c.end[idx], *tag, "end after the second piece")
            same(st2, G.carried(c.st[idx]), *tag, "carried after the second piece")
    # the device form, once: the random cut, u32 offsets, outputs two entries longer than the batch
    idx = c.batch(c.FULL, 15)
    n = len(idx)
    cut = c.cut["random"][idx]
    mid = c.state_at(idx, cut)
    base, off = G.packed(c.rows[idx], cut)
    o = Out(n, True, state=np.full(n, hip.STATE_START, np.uint32))
    d_base, d_off32 = to_dev(base), to_dev(off.astype(np.uint32))        # (held to the check: a freed tensor's block is the next one's)
    dfa.exec_packed_resume_device(d_base.data_ptr(), hip.META_OFF32, d_off32.data_ptr(), n, o.state.data_ptr(), o.end.data_ptr(), o.bm.data_ptr())
    ran(dfa, True, True)
    o.check(G.ends(c.flat, mid), name, "device, first piece", want_state=G.carried(mid))
    rest_rows, rest_lens = c.rest(idx, cut)
    base, off = G.packed(rest_rows, rest_lens)
    o2 = Out(n, False, state=G.carried(mid))
    d_base, d_off = to_dev(base), to_dev(off)
    dfa.exec_packed_resume_device(d_base.data_ptr(), hip.META_OFF64, d_off.data_ptr(), n, o2.state.data_ptr(), o2.end.data_ptr(), o2.bm.data_ptr())
    o2.check(c.end[idx], name, "device, second piece", want_state=G.carried(c.st[idx]))


@pytest.mark.parametrize("name", R.NAMES)
def test_pieces_handed_dead_and_the_absorbing_accept(hip, dfas, name):
    """a piece handed STATE_DEAD stays dead whatever it reads; one handed the absorbing accept state stays there (empty pieces
    included); one handed the state one byte before a word's end turns absorbing at its byte 0"""
    c, dfa = R.case(name), dfas(name)
    idx = c.batch(c.FULL, 7)
    n = len(idx)
    for front in ("offsets", "packed lengths", "rows"):
        st, end = _resume(hip, dfa, front, c.rows[idx], c.lens[idx], np.full(n, hip.STATE_DEAD, np.uint32))
        ran(dfa, True, True)
        assert (end == NO).all() and (st == hip.STATE_DEAD).all(), (name, front)
    if name in ("abs_accept16", "abs_accept64"):
        acc = int(np.nonzero(c.absorbing)[0][0])
        for front in ("offsets", "packed u32", "rows"):
            st, end = _resume(hip, dfa, front, c.rows[idx], c.lens[idx], np.full(n, acc, np.uint32))
            assert (end == acc).all() and (st == acc).all(), (name, front)
    # mixed: every third line handed DEAD, the others the reference's state after their first byte
    one = np.minimum(c.lens[idx], 1).astype(np.uint32)
    mid = c.state_at(idx, one).copy()
    mid[::3] = -1
    rest_rows, rest_lens = c.rest(idx, one)
    want = G.walk(c.dense, R.IDENT, c.start, rest_rows, rest_lens, mid)
    st, end = _resume(hip, dfa, "offsets", rest_rows, rest_lens, G.carried(mid))
    same(end, G.ends(c.flat, want), name, "mixed")
    same(st, G.carried(want), name, "mixed")
    if c.has_abs:
        # the hand-made lines cut right before the byte that makes them absorbing: it is the second piece's byte 0
        hand = np.array([i for i, _, k in c.hand if k is not None], np.int64)
        cut = np.array([k for _, _, k in c.hand if k is not None], np.uint32)
        mid = c.state_at(hand, cut)
        assert (mid >= 0).all() and not c.absorbing[mid].any()
        rest_rows, rest_lens = c.rest(hand, cut)
        for front in ("offsets", "rows"):
            st, end = _resume(hip, dfa, front, rest_rows, rest_lens, G.carried(mid))
            same(end, c.end[hand], name, front, "absorbing at byte 0")
            same(st, G.carried(c.st[hand]), name, front, "absorbing at byte 0")


# ---- 5. end-ids riding along ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.WITH_IDS)
def test_end_ids_ride_along(hip, dfas, name):
    """FSM_HIP_IDS_EARLIEST and FSM_HIP_IDS_RET from the same kernel, through u64 offsets and rows + lengths"""
    c, dfa = R.case(name), dfas(name)
    sets = [s.tolist() for s in dfa.ret_sets()]
    for n, tail in ((c.FULL, 7), (257, 15), (192, 0)):
        idx = c.batch(n, tail)
        base, off = c.packed(idx)
        low = c.lowest_id(c.st[idx])
        for front in ("offsets", "rows"):
            run = (lambda mode: dfa.exec_offsets_ids(base, off, mode)) if front == "offsets" else (lambda mode: dfa.exec_batch_ids(c.rows[idx], mode, c.lens[idx]))
            got = run(1)
            ran(dfa, True, c.has_abs, (3, 3, 2))
            same(got, low, name, n, front, "lowest id")
            got = run(2)
            ran(dfa, True, c.has_abs)
            hit = c.end[idx] != NO
            assert (got[~hit] == NO).all(), (name, n, front)
            for i in np.nonzero(hit)[0].tolist():
                assert sets[int(got[i])] == c.ids_of(int(c.st[idx[i]])), (name, n, front, i)
    assert (low != NO).sum() > 20 and len({tuple(s) for s in sets}) > 3
