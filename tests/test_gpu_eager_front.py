"""GPU (-m gpu): the single-DFA eager walks on every layout and input path -- fsm_hip_exec_batch_eager{,_device,_offsets,
_offsets_device} and fsm_hip_exec_batch_eager_resume{,_device}: EagerPol / EagerWidePol (walk_kernels.h), plain and
resumed, behind walk_ldsdma, walk_direct, walk_generic and walk_ragged (launch.h launch_eager_pol).

Automata, inputs and the reference's answers are tests/eager_front_ref.py (global_ref.affine at sizes the LDS layouts take;
tests/test_eager_front_cases.py asserts the table on the CPU).  The judge of every answer is global_ref.walk_eager / ends /
carried -- the closed formula byte by byte in numpy -- and sets are compared as uint64 words in the automaton's own bit order.
Nothing is compared with another layout, kernel, knob setting or front of the library.  After the first launch of every
configuration the kernel that ran (fsm_hip_last_kernel_name) is asserted: its walk, its policy, plain or resumed."""
import errno
import re

import numpy as np
import pytest

import eager_front_ref as R
import global_ref as G

pytestmark = pytest.mark.gpu

NO = 0xFFFFFFFF
N, L, HALF = R.N, R.L, R.HALF
LDS_LIMIT = 163840                       # all of a workgroup's LDS on this device
DMA_TILE, RAGGED_WAVE = 8192, 8192 + 64 * 16 + 1024      # per wavefront: an LDS-DMA tile; the ragged kernel's tile + ring + row records
JUNK32, JUNK64 = 0x5A5A5A5A, 0xA5A5A5A5A5A5A5A5
POLICY = {"tiny": "TinyPol<unsigned long>", "lds": "LdsPol", "ldsself": "LdsSelfPol", "comb": "CombPol", "comb256": "Comb256Pol",
          "combself": "CombSelfPol", "sparse": "SparsePol", "global": "Glob16Pol"}
RESUMED = re.compile(r"Eager(?:Wide)?Pol<fsmhip::\w+(?:<[^<>]*>)?, true>")
PLAIN = re.compile(r"Eager(?:Wide)?Pol<fsmhip::\w+(?:<[^<>]*>)?, false>")
PAIR_IDS = [f"{a}-{lay}" for a, lay in R.PAIRS]


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()
    assert G.LIB_DEAD == libfsm_amd.STATE_DEAD and G.LIB_START == libfsm_amd.STATE_START
    return libfsm_amd


def same(got, want, *tag):
    got = np.asarray(got).reshape(np.shape(want))
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).reshape(len(want), -1).any(axis=1))[0]
        raise AssertionError((tag, f"{len(bad)} of {len(want)} differ", bad[:8].tolist(), got[bad[:4]].tolist(), np.asarray(want)[bad[:4]].tolist()))


def alone(got, piece, *tag):
    """a later piece's sets of its own: everything a change of state emits, nothing the piece does not emit by fsm_exec's rule
    (eager_front_ref.Piece) -- so never the outputs of the state it was handed, unless the piece itself comes back to it"""
    got = np.asarray(got, np.uint64).reshape(-1, piece.words.shape[1])
    bad = piece.holds(got)
    if len(bad):
        raise AssertionError((tag, f"{len(bad)} of {len(got)} outside the bounds", bad[:8].tolist(), got[bad[:4]].tolist(),
                              piece.changed[bad[:4]].tolist(), piece.words[bad[:4]].tolist()))


def open_dfa(hip, c, lay):
    dfa = hip.HipDfa(c.flat, R.LAYOUT_OF[lay])
    assert dfa.info()["layout_name"] == lay
    assert dfa.eager_words() == c.W and dfa.eager_id_count() == len(c.ids)
    assert [dfa.eager_id(b) for b in range(len(c.ids))] == c.ids.tolist()      # the bit order the reference's words are built in
    return dfa


def table_lds(dfa, hip):
    """the LDS the table takes in front of any tile: what info() reports behind a per-lane kernel"""
    dfa.tune(hip.KNOB_INPUT_MODE, hip.IN_GENERIC)
    v = dfa.info()["lds_bytes"]
    dfa.tune(hip.KNOB_INPUT_MODE, -1)
    return v


def set_mode(dfa, hip, mode, seg=0):
    dfa.tune(hip.KNOB_INPUT_MODE, mode)
    dfa.tune(hip.KNOB_SEG, seg)


def ran(dfa, c, lay, walk, resumed):
    """the kernel of the last launch: this walk, the layout's policy wrapped by the set width's eager policy, plain or resumed"""
    kn = dfa.last_kernel_name()
    assert walk + "<" in kn, (kn, walk)
    assert POLICY[lay] in kn, (kn, lay)
    assert ("EagerWidePol<" in kn) == (c.W > 1) and ("EagerPol<" in kn) == (c.W == 1), kn
    assert bool(RESUMED.search(kn)) == resumed and bool(PLAIN.search(kn)) == (not resumed), kn
    return kn


def fixed_settings(hip, c, lay, tl):
    """(label, input mode, segment knob, the walk pick_cfg gives a 64-byte-multiple stride)"""
    wide = c.W > 1
    dma = not wide and (lay == "tiny" or tl + 12 * DMA_TILE <= LDS_LIMIT)
    ragged = "walk_ragged" if tl + 4 * RAGGED_WAVE <= LDS_LIMIT else "walk_generic"
    return (("default", -1, 0, "walk_ldsdma" if dma else "walk_direct"),
            ("lds-dma 64", hip.IN_LDSDMA, 64, "walk_direct"),                       # the eager LDS-DMA kernels take 128-byte segments only
            ("lds-dma 128", hip.IN_LDSDMA, 128, "walk_direct" if wide else "walk_ldsdma"),
            ("direct", hip.IN_DIRECT, 0, "walk_direct"),
            ("generic", hip.IN_GENERIC, 0, "walk_generic"),
            ("ragged", hip.IN_RAGGED, 0, ragged))


# ---- device buffers ------------------------------------------------------------------------------------------------------

def to_dev(a, pad=0):
    import torch
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    if pad:
        b = np.concatenate([b, np.zeros(pad, np.uint8)])
    return torch.from_numpy(b.copy()).cuda()


def from_dev(t, dtype):
    return t.cpu().numpy().view(dtype)


class Out:
    """end_out and the sets on the device, two entries longer than the batch, pre-filled: 0x5A.. and 0xA5.."""

    def __init__(self, n, W, sets=None):
        import torch
        self.n, self.W = n, W
        self.end = torch.full(((n + 2) * 4,), 0x5A, dtype=torch.uint8, device="cuda")
        if sets is None:
            self.sets = torch.full(((n + 2) * W * 8,), 0xA5, dtype=torch.uint8, device="cuda")
        else:
            self.sets = to_dev(np.concatenate([np.asarray(sets, np.uint64).reshape(-1), np.full(2 * W, JUNK64, np.uint64)]))

    def check(self, want_end, want_words, *tag):
        import torch
        torch.cuda.synchronize()
        end, words = from_dev(self.end, np.uint32), from_dev(self.sets, np.uint64).reshape(-1, self.W)
        if want_end is not None:
            same(end[:self.n], want_end, "end", *tag)          # every entry written: no junk is a state or NO_MATCH
        else:
            assert (end == JUNK32).all(), tag
        same(words[:self.n], want_words, "sets", *tag)
        assert (end[self.n:] == JUNK32).all() and (words[self.n:] == JUNK64).all(), tag


# ---- fixed stride --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,lay", R.PAIRS, ids=PAIR_IDS)
def test_fixed_stride_plain_and_resumed_in_halves(hip, name, lay):
    c = R.case(name)
    rows = R.inputs(c.dying)[0]
    first_rows, second_rows = np.ascontiguousarray(rows[:, :HALF]), np.ascontiguousarray(rows[:, HALF:])
    dfa = open_dfa(hip, c, lay)
    tl = table_lds(dfa, hip)
    start = np.full(N, hip.STATE_START, np.uint32)
    for label, mode, seg, walk in fixed_settings(hip, c, lay, tl):
        set_mode(dfa, hip, mode, seg)
        for n in R.SUBS:
            end, eo = dfa.exec_eager_words(rows[:n])
            if n == R.SUBS[0]:
                kn = ran(dfa, c, lay, walk, False)
            same(end, c.all.end[:n], name, lay, label, n, "end")
            same(eo, c.all.words[:n], name, lay, label, n, "sets")
        # in two equal pieces, no lengths: what the big-input walk launches
        for n in (65, N):
            z = np.zeros(n * c.W, np.uint64)
            st, end, eo = dfa.exec_batch_eager_resume(first_rows[:n], start[:n], z)
            knr = ran(dfa, c, lay, walk, True)
            same(st, c.first.carried[:n], name, lay, label, n, "first piece: carried")
            same(end, c.first.end[:n], name, lay, label, n, "first piece: end")
            same(eo, c.first.words[:n], name, lay, label, n, "first piece: sets")
            st2, end2, eo2 = dfa.exec_batch_eager_resume(second_rows[:n], st, eo)
            same(st2, c.all.carried[:n], name, lay, label, n, "second piece: carried")
            same(end2, c.all.end[:n], name, lay, label, n, "second piece: end")
            same(eo2, c.all.words[:n], name, lay, label, n, "second piece: sets")
            # the second piece into sets of its own: what it adds, and never the outputs of the state it is handed
            _, _, eo3 = dfa.exec_batch_eager_resume(second_rows[:n], st, z)
            alone(eo3, c.second, name, lay, label, n, "second piece alone: sets")
        print(f"{name} {lay} {label}: {kn} | {knr}")
    dfa.close()


# ---- rows with lengths, packed with u64 offsets; host and device pointers -------------------------------------------------

@pytest.mark.parametrize("name,lay", R.PAIRS, ids=PAIR_IDS)
def test_lengths_and_offsets_host_and_device(hip, name, lay):
    c = R.case(name)
    rows, lens = R.inputs(c.dying)
    base, off = c.packed
    base5, off5 = np.concatenate([np.full(5, 0xFF, np.uint8), base]), off + np.uint64(5)       # off[0] = 5
    d_rows, d_lens = to_dev(rows, 64), to_dev(lens)
    d_base, d_off, d_base5, d_off5 = to_dev(base, 64), to_dev(off), to_dev(base5, 64), to_dev(off5)
    dfa = open_dfa(hip, c, lay)
    ragged = "walk_ragged" if table_lds(dfa, hip) + 4 * RAGGED_WAVE <= LDS_LIMIT else "walk_generic"
    assert lens.mean() > 100                    # a host front sends these to the ragged kernel by itself
    for mode, walk in ((-1, ragged), (hip.IN_RAGGED, ragged), (hip.IN_GENERIC, "walk_generic")):
        set_mode(dfa, hip, mode)
        for n in R.SUBS:
            want = (c.len.end[:n], c.len.words[:n])
            tag = (name, lay, mode, n)
            nb = int(off[n])
            host = {"rows + lens": dfa.exec_eager_words(rows[:n], lens[:n]),
                    "offsets": dfa.exec_eager_words(base[:nb], off=off[:n + 1]),
                    "offsets from 5": dfa.exec_eager_words(base5[:nb + 5], off=off5[:n + 1])}
            if n == N:
                ran(dfa, c, lay, walk, False)
            for form, (end, eo) in host.items():
                same(end, want[0], *tag, form, "end")
                same(eo, want[1], *tag, form, "sets")
            o = Out(n, c.W)
            dfa.exec_batch_eager_device(d_rows.data_ptr(), L, n, o.end.data_ptr(), o.sets.data_ptr(), d_len=d_lens.data_ptr())
            o.check(*want, *tag, "device rows + lens")
            if n == N:      # (no knob: both candidates were launched, the batch's mean length chose on the device)
                ran(dfa, c, lay, walk, False)
            o = Out(n, c.W)
            dfa.exec_batch_eager_offsets_device(d_base.data_ptr(), d_off.data_ptr(), n, o.end.data_ptr(), o.sets.data_ptr())
            o.check(*want, *tag, "device offsets")
            if n == N:
                ran(dfa, c, lay, walk, False)
            o = Out(n, c.W)
            dfa.exec_batch_eager_offsets_device(d_base5.data_ptr(), d_off5.data_ptr(), n, o.end.data_ptr(), o.sets.data_ptr())
            o.check(*want, *tag, "device offsets from 5")
    dfa.close()


# ---- a device-pointer batch with no knob set: two kernels are launched, offsets_pick chooses --------------------------------

def hand_over(dfa, hip, c, lay):
    """the mean input length from which a variable-length batch goes to walk_ragged, asked of the library: host batches of 64
    lines of m bytes each, the smallest m that the host front (which knows the mean) sends there"""
    rows = R.inputs(c.dying)[0]

    def goes_ragged(m):
        dfa.exec_eager_words(np.ascontiguousarray(rows[:64, :m]).reshape(-1), off=np.arange(65, dtype=np.uint64) * np.uint64(m))
        kn = dfa.last_kernel_name()
        assert ("walk_ragged<" in kn) != ("walk_generic<" in kn), kn
        return "walk_ragged<" in kn

    lo, hi = 1, L
    assert not goes_ragged(lo) and goes_ragged(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if goes_ragged(mid) else (mid, hi)
    return hi


@pytest.mark.parametrize("name,lay", [("s200", "lds"), ("s200_dying", "comb"), ("s1000", "lds"), ("s1000_dying", "global"), ("s15_dying", "tiny")])
def test_device_pointer_pick_between_generic_and_ragged(hip, name, lay):
    c = R.case(name)
    rows = R.inputs(c.dying)[0]
    dfa = open_dfa(hip, c, lay)
    assert table_lds(dfa, hip) + 4 * RAGGED_WAVE <= LDS_LIMIT
    T = hand_over(dfa, hip, c, lay)
    print(f"{name} {lay}: variable-length batches go to walk_ragged from a mean of {T} bytes")
    assert 16 <= T <= L - 8
    d_rows = to_dev(rows, 64)
    start = np.full(N, hip.STATE_START, np.uint32)
    for mean, walk, other in ((T - 1, "walk_generic", "walk_ragged"), (T, "walk_ragged", "walk_generic")):
        lens = np.full(N, mean, np.uint32)
        lens[0:N - 1:2] += 7
        lens[1:N - 1:2] -= 7                      # N is odd: the last line keeps the mean, the sum is N * mean exactly
        assert int(lens.sum()) // N == mean and int(lens.sum()) == N * mean
        want = R.Ref(c, rows, lens)
        base, off = G.packed(rows, lens)
        d_lens, d_base, d_off = to_dev(lens), to_dev(base, 64), to_dev(off)
        for form in ("rows + lens", "offsets"):
            o = Out(N, c.W)
            if form == "offsets":
                dfa.exec_batch_eager_offsets_device(d_base.data_ptr(), d_off.data_ptr(), N, o.end.data_ptr(), o.sets.data_ptr())
            else:
                dfa.exec_batch_eager_device(d_rows.data_ptr(), L, N, o.end.data_ptr(), o.sets.data_ptr(), d_len=d_lens.data_ptr())
            o.check(want.end, want.words, name, lay, mean, form)
            kn = ran(dfa, c, lay, walk, False)
            assert other not in kn and "1 of 2 launched" in kn, kn
            # resumed: state_io is read and written by the kernel that runs -- had the other one run too, it would have started
            # from the states the first left and OR-ed a second walk's outputs into the sets
            d_st = to_dev(start)
            o = Out(N, c.W, sets=np.zeros((N, c.W), np.uint64))
            if form == "offsets":
                dfa.exec_batch_eager_resume_device(d_base.data_ptr(), 0, N, d_st.data_ptr(), o.sets.data_ptr(), d_off=d_off.data_ptr(), d_end=o.end.data_ptr())
            else:
                dfa.exec_batch_eager_resume_device(d_rows.data_ptr(), L, N, d_st.data_ptr(), o.sets.data_ptr(), d_len=d_lens.data_ptr(), d_end=o.end.data_ptr())
            o.check(want.end, want.words, name, lay, mean, form, "resumed")
            same(from_dev(d_st, np.uint32), want.carried, name, lay, mean, form, "carried")
            kn = ran(dfa, c, lay, walk, True)
            assert other not in kn and "1 of 2 launched" in kn, kn
    dfa.close()


# ---- lane refill: every wavefront of the ragged kernel owns at least three tiles of short lines ------------------------------

REFILL_PAIRS = [(a, lay) for a, lay in R.PAIRS if a in ("s200", "s200_dying", "s1000", "s1000_dying")] + [("s15_dying", "tiny"), ("s15_dying", "comb256")]


@pytest.mark.parametrize("name,lay", REFILL_PAIRS, ids=[f"{a}-{lay}" for a, lay in REFILL_PAIRS])
def test_lane_refill(hip, name, lay):
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 3 * 64 * ncu + 37
    assert ((n + 63) // 64 + ncu - 1) // ncu * 64 >= 192        # per = ceil(words / nwaves) * 64 inputs a wavefront, one wavefront a CU
    c = R.case(name)
    r = R.refill(name, n)
    rows, lens, cut = R.refill_inputs(n)
    if c.dying:
        assert ((r.first.st < 0) & (cut > 0)).sum() > 100       # first pieces that end DEAD
    assert ((r.first.st == 0) & (cut == 0)).sum() > 1000        # ... and empty ones: the start state's own id is carried, not START
    assert (r.second.em[(cut == 0) & (lens > 0)][:, c.start_cols] == 0).any()    # where firing them again would show
    dfa = open_dfa(hip, c, lay)
    assert table_lds(dfa, hip) + RAGGED_WAVE <= LDS_LIMIT
    dfa.tune(hip.KNOB_WAVES, 1)
    dfa.tune(hip.KNOB_BLOCKS_PER_CU, 1)
    dfa.tune(hip.KNOB_INPUT_MODE, hip.IN_RAGGED)
    base, off = r.packed
    # plain: u64 offsets, u32 offsets, lengths alone, and rows + lengths
    got = {"eager_offsets": dfa.exec_eager_words(base, off=off)}
    ran(dfa, c, lay, "walk_ragged", False)
    for form, meta in ((hip.META_OFF64, off), (hip.META_OFF32, off.astype(np.uint32)), (hip.META_LENGTHS, lens)):
        a = dfa.exec_packed_all_form(base, form, meta, n, want_eager=True)
        ran(dfa, c, lay, "walk_ragged", False)
        got[f"packed_all form {form}"] = (a["end"], a["eager"])
    got["rows + lens"] = dfa.exec_eager_words(rows, lens)
    ran(dfa, c, lay, "walk_ragged", False)
    for form, (end, eo) in got.items():
        same(end, r.whole.end, name, lay, form, "end")
        same(eo, r.whole.words, name, lay, form, "sets")
    # resumed: every line cut at a random byte, two calls; packed (u64 offsets: the one packed form this front has) and rows + lengths
    start, z = np.full(n, hip.STATE_START, np.uint32), np.zeros(n * c.W, np.uint64)
    b1, o1 = r.packed_first
    b2, o2 = r.packed_rest
    for form in ("offsets", "rows + lens"):
        if form == "offsets":
            st, end, eo = dfa.exec_batch_eager_resume(b1, start, z, off=o1)
        else:
            st, end, eo = dfa.exec_batch_eager_resume(rows, start, z, lens=cut)
        ran(dfa, c, lay, "walk_ragged", True)
        same(st, r.first.carried, name, lay, form, "first piece: carried")
        same(end, r.first.end, name, lay, form, "first piece: end")
        same(eo, r.first.words, name, lay, form, "first piece: sets")
        for into in (eo, z):
            if form == "offsets":
                st2, end2, eo2 = dfa.exec_batch_eager_resume(b2, st, into, off=o2)
            else:
                st2, end2, eo2 = dfa.exec_batch_eager_resume(r.rest_rows, st, into, lens=r.rest_lens)
            same(st2, r.whole.carried, name, lay, form, "second piece: carried")
            same(end2, r.whole.end, name, lay, form, "second piece: end")
            if into is eo:
                same(eo2, r.whole.words, name, lay, form, "second piece: sets")
            else:
                alone(eo2, r.second, name, lay, form, "second piece alone: sets")
    dfa.close()


# ---- output discipline -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,lay", R.PAIRS, ids=PAIR_IDS)
def test_output_discipline(hip, name, lay):
    c = R.case(name)
    rows = R.inputs(c.dying)[0]
    first_rows, second_rows = np.ascontiguousarray(rows[:, :HALF]), np.ascontiguousarray(rows[:, HALF:])
    d_rows, d_first, d_second = to_dev(rows, 64), to_dev(first_rows, 64), to_dev(second_rows, 64)
    base, off = c.packed
    d_base, d_off = to_dev(base, 64), to_dev(off)
    dfa = open_dfa(hip, c, lay)
    bit = len(c.ids)                                             # one bit above the id count: no walk may touch it
    assert bit % 64 != 0
    marker = np.zeros((1, c.W), np.uint64)
    marker[0, bit // 64] = np.uint64(1) << np.uint64(bit % 64)
    for n in (129, N):
        tag = (name, lay, n)
        # plain: the sets pre-filled with 0xA5 bytes come back as exact words (W = 1: stored; W = 2: cleared before the walk)
        o = Out(n, c.W)
        dfa.exec_batch_eager_device(d_rows.data_ptr(), L, n, o.end.data_ptr(), o.sets.data_ptr())
        o.check(c.all.end[:n], c.all.words[:n], *tag, "plain")
        # ... without end_out
        o = Out(n, c.W)
        dfa.exec_batch_eager_device(d_rows.data_ptr(), L, n, 0, o.sets.data_ptr())
        o.check(None, c.all.words[:n], *tag, "plain, no end_out")
        o = Out(n, c.W)
        dfa.exec_batch_eager_offsets_device(d_base.data_ptr(), d_off.data_ptr(), n, 0, o.sets.data_ptr())
        o.check(None, c.len.words[:n], *tag, "offsets, no end_out")
        # ... and, where the ABI lets the sets be left out, with end_out alone: the all-outputs front
        o = Out(n, c.W)
        dfa.exec_packed_all_device(d_base.data_ptr(), hip.META_OFF64, d_off.data_ptr(), n, d_end=o.end.data_ptr())
        o.check(c.len.end[:n], np.full((n, c.W), JUNK64, np.uint64), *tag, "packed_all, no sets")
        o = Out(n, c.W)
        dfa.exec_packed_all_device(d_base.data_ptr(), hip.META_OFF64, d_off.data_ptr(), n, d_eager=o.sets.data_ptr())
        o.check(None, c.len.words[:n], *tag, "packed_all, sets alone")
        # resumed: OR-ed into what the sets hold, never stored, never cleared
        d_st = to_dev(np.full(n, hip.STATE_START, np.uint32))
        o = Out(n, c.W, sets=np.tile(marker, (n, 1)))
        dfa.exec_batch_eager_resume_device(d_first.data_ptr(), HALF, n, d_st.data_ptr(), o.sets.data_ptr(), d_end=o.end.data_ptr())
        o.check(c.first.end[:n], c.first.words[:n] | marker, *tag, "resumed, first piece")
        same(from_dev(d_st, np.uint32), c.first.carried[:n], *tag, "resumed, first piece: carried")
        o = Out(n, c.W, sets=c.first.words[:n] | marker)
        dfa.exec_batch_eager_resume_device(d_second.data_ptr(), HALF, n, d_st.data_ptr(), o.sets.data_ptr())      # (no end_out)
        o.check(None, c.all.words[:n] | marker, *tag, "resumed, second piece")
        same(from_dev(d_st, np.uint32), c.all.carried[:n], *tag, "resumed, second piece: carried")
    # the host fronts without end_out
    _, eo = dfa.exec_eager_words(rows[:129], want_end=False)
    same(eo, c.all.words[:129], name, lay, "host, no end_out")
    st, end, eo = dfa.exec_batch_eager_resume(first_rows[:129], np.full(129, hip.STATE_START, np.uint32), np.tile(marker, (129, 1)), want_end=False)
    assert end is None
    same(eo, c.first.words[:129] | marker, name, lay, "host resumed, no end_out")
    same(st, c.first.carried[:129], name, lay, "host resumed, no end_out: carried")
    dfa.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------

def refused(call):
    with pytest.raises(OSError) as ei:
        call()
    assert ei.value.errno == errno.EINVAL


@pytest.mark.parametrize("name", ["s200", "s1000"])
def test_refusals(hip, name):
    c = R.case(name)
    rows, lens = R.inputs(c.dying)
    n = 65
    base, off = G.packed(rows[:n], lens[:n])
    d_rows, d_base, d_off = to_dev(rows[:n], 64), to_dev(base, 64), to_dev(off)
    dfa = open_dfa(hip, c, R.AUTO[name])
    start = np.full(n, hip.STATE_START, np.uint32)
    z = np.zeros(n * c.W, np.uint64)
    # no sets to write to
    refused(lambda: dfa.exec_eager_words(rows[:n], null_sets=True))
    refused(lambda: dfa.exec_eager_words(base, off=off, null_sets=True))
    refused(lambda: dfa.exec_batch_eager_resume(rows[:n], start, None))
    refused(lambda: dfa.exec_batch_eager_resume(rows[:n], None, z))
    o = Out(n, c.W)
    d_st = to_dev(start)
    refused(lambda: dfa.exec_batch_eager_device(d_rows.data_ptr(), L, n, o.end.data_ptr(), 0))
    refused(lambda: dfa.exec_batch_eager_offsets_device(d_base.data_ptr(), d_off.data_ptr(), n, o.end.data_ptr(), 0))
    refused(lambda: dfa.exec_batch_eager_offsets_device(d_base.data_ptr(), 0, n, o.end.data_ptr(), o.sets.data_ptr()))
    refused(lambda: dfa.exec_batch_eager_resume_device(d_rows.data_ptr(), L, n, d_st.data_ptr(), 0, d_end=o.end.data_ptr()))
    refused(lambda: dfa.exec_batch_eager_resume_device(d_rows.data_ptr(), L, n, 0, o.sets.data_ptr(), d_end=o.end.data_ptr()))
    # decreasing host offsets; a length beyond the stride
    bad = off.copy()
    bad[7] = bad[6] - np.uint64(1)
    refused(lambda: dfa.exec_eager_words(base, off=bad))
    refused(lambda: dfa.exec_batch_eager_resume(base, start, z, off=bad))
    long = lens[:n].copy()
    long[9] = L + 1
    refused(lambda: dfa.exec_eager_words(rows[:n], long))
    # every refused call left the device buffers as they were, and the next call answers
    o.check(None, np.full((n, c.W), JUNK64, np.uint64), name, "after the refusals")
    same(from_dev(d_st, np.uint32), start, name, "state_io after the refusals")
    end, eo = dfa.exec_eager_words(rows[:n], lens[:n])
    same(end, c.len.end[:n], name, "after the refusals: end")
    same(eo, c.len.words[:n], name, "after the refusals: sets")
    dfa.close()


def test_automaton_without_eager_outputs_asked_for_sets(hip):
    """the eager fronts on an automaton no state of which emits: one all-zero word an input (fsm_hip_eager_words is at least 1),
    the end states of the plain walk; the resumed front leaves the carried sets as they are"""
    n = 129
    rows, lens = R.inputs(False)
    flat, dense, cls = G.affine(200, 4)
    assert flat.eager_off is None
    dfa = hip.HipDfa(flat)
    assert dfa.eager_id_count() == 0 and dfa.eager_words() == 1
    st_all, st_len = G.walk(dense, cls, 0, rows[:n]), G.walk(dense, cls, 0, rows[:n], lens[:n])
    zeros = np.zeros((n, 1), np.uint64)
    end, eo = dfa.exec_eager_words(rows[:n], eager_out=np.full((n, 1), JUNK64, np.uint64))
    same(end, G.ends(flat, st_all), "rows: end")
    same(eo, zeros, "rows: sets")
    assert "Eager" not in dfa.last_kernel_name()
    base, off = G.packed(rows[:n], lens[:n])
    end, eo = dfa.exec_eager_words(base, off=off, eager_out=np.full((n, 1), JUNK64, np.uint64))
    same(end, G.ends(flat, st_len), "offsets: end")
    same(eo, zeros, "offsets: sets")
    d_rows, d_base, d_off = to_dev(rows[:n], 64), to_dev(base, 64), to_dev(off)
    o = Out(n, 1)
    dfa.exec_batch_eager_device(d_rows.data_ptr(), L, n, o.end.data_ptr(), o.sets.data_ptr())
    o.check(G.ends(flat, st_all), zeros, "device rows")
    o = Out(n, 1)
    dfa.exec_batch_eager_offsets_device(d_base.data_ptr(), d_off.data_ptr(), n, o.end.data_ptr(), o.sets.data_ptr())
    o.check(G.ends(flat, st_len), zeros, "device offsets")
    keep = np.arange(n, dtype=np.uint64) * np.uint64(0x0101010101010101) + np.uint64(3)
    st, end, eo = dfa.exec_batch_eager_resume(rows[:n], np.full(n, hip.STATE_START, np.uint32), keep)
    same(st, G.carried(st_all), "resumed: carried")
    same(end, G.ends(flat, st_all), "resumed: end")
    same(eo, keep, "resumed: sets")
    dfa.close()
