"""GPU (-m gpu): the self-loop-mask layouts (FSM_HIP_LAYOUT_COMBSELF / _LDSSELF: CombSelfPol, LdsSelfPol) at the edges of their
chunk skips -- self-loop ranges at 0, 127, 128 and 255 and ranges the planner must refuse, wavefronts whose lanes sit in
different looping states when the vote is taken, a looping state entered inside a chunk, 32 classes (no spare class: the
predicated tail), a start state with a loop of its own, walks resumed in looping, dead and absorbing states.

Automata, rows and why they bite are tests/selfloop_ref.py (tests/test_selfloop_cases.py asserts its conditions on the CPU).
Every answer is compared bit for bit with oracle.pyoracle.Oracle; every configuration runs with the chunk skip on and off
(FSM_HIP_KNOB_EARLY_RETIRE bit 2, FSM_HIP_KNOB_NOSKIP), and after every launch the kernel that ran is held against the
family the knobs ask for and the layout's policy."""
import functools

import numpy as np
import pytest

import selfloop_ref as R

pytestmark = pytest.mark.gpu

NO = R.NO
IN_DIRECT, IN_LDSDMA, IN_GENERIC, IN_RAGGED = 0, 1, 2, 3
NOSKIP, NO_LINES32 = 4, 32                                # FSM_HIP_KNOB_EARLY_RETIRE bit 2: never skip a chunk; bit 5: walk_generic's own body
EARLY = (0, 1, 3, 0 | NOSKIP, 1 | NOSKIP, 3 | NOSKIP)
POLS = {"combself": "fsmhip::CombSelfPol", "ldsself": "fsmhip::LdsSelfPol"}

#          label, input mode, segment, pack
SETTINGS = (("default", -1, 0, -1), ("direct", IN_DIRECT, 0, -1), ("lds-dma 64", IN_LDSDMA, 64, 0), ("lds-dma 128", IN_LDSDMA, 128, 0),
            ("packing", IN_LDSDMA, 128, 1), ("generic", IN_GENERIC, 0, -1), ("ragged", IN_RAGGED, 0, -1))

CASES = {
    "select28": lambda: R.select(0),
    "select31": lambda: R.select(3),
    "select32": lambda: R.select(4),
    "absorbing28": lambda: R.select(0, acc="absorbing"),
    "absorbing32": lambda: R.select(4, acc="absorbing"),
    "startloop31": lambda: R.select(2, start_loop=True),
    "startloop32": lambda: R.select(3, start_loop=True),
    "accepting28": lambda: R.select(0, loops_accept=True),
    "accepting32": lambda: R.select(4, loops_accept=True),
    "pingpong": R.pingpong,
}
CLASSES = dict(select28=28, select31=31, select32=32, absorbing28=28, absorbing32=32, startloop31=31, startloop32=32, accepting28=28, accepting32=32,
               pingpong=3)
BOTH = [(c, l) for c in CASES for l in POLS]


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()
    assert (libfsm_amd.IN_DIRECT, libfsm_amd.IN_LDSDMA, libfsm_amd.IN_GENERIC, libfsm_amd.IN_RAGGED) == (IN_DIRECT, IN_LDSDMA, IN_GENERIC, IN_RAGGED)
    assert (R.START, R.DEAD) == (libfsm_amd.STATE_START, libfsm_amd.STATE_DEAD)
    return libfsm_amd


def opened(hip, name, layout):
    c = CASES[name]()
    dfa = hip.HipDfa(c.flat, getattr(hip, "LAYOUT_" + layout.upper()))
    assert dfa.info()["layout_name"] == layout
    assert hip.Plan(c.flat, getattr(hip, "LAYOUT_" + layout.upper())).C == CLASSES[name]
    return c, dfa


def ran(dfa, layout, parts, *tag):
    kn = dfa.last_kernel_name()
    assert any(p in kn for p in parts) and POLS[layout] in kn, (tag, "expected one of", parts, POLS[layout], "ran", kn)
    return kn.split(" (")[0]


def to_dev(a):
    import torch
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([b, np.zeros(64, np.uint8)])).cuda()


@functools.lru_cache(maxsize=None)
def batch(name, L, varlen=False, part=0):
    """-> (rows, lens, the oracle's end states, the rows on the device, the lengths on the device)"""
    c = CASES[name]()
    rows, lens, _ = R.rows_of(c, L, varlen, part)
    assert len(rows) <= 20000
    want = c.ends(rows, lens if varlen else None)
    want.setflags(write=False)
    return rows, lens, want, to_dev(rows), to_dev(lens)


def check(end, bm, want, *tag):
    n = len(want)
    bad = np.nonzero(end != want)[0]
    assert len(bad) == 0, (tag, f"{len(bad)} of {n} end states differ", bad[:8].tolist(), end[bad[:8]].tolist(), want[bad[:8]].tolist())
    got = np.unpackbits(np.ascontiguousarray(bm).view(np.uint8), bitorder="little")[:n].astype(bool)
    assert np.array_equal(got, want != NO), (tag, "bitmap")


def outputs(n):
    import torch
    return torch.full((n + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"), torch.full(((n + 63) // 64 + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")


def fetched(n, end, bm):
    import torch
    torch.cuda.synchronize()
    e, b = end.cpu().numpy().view(np.uint32), bm.cpu().numpy().view(np.uint64)
    w = (n + 63) // 64
    assert (e[n:] == 0x5A5A5A5A).all() and (b[w:] == 0x5A5A5A5A5A5A5A5A).all(), "written behind the batch"
    return e[:n], b[:w]


def walk_rows(dfa, on_dev, rows, lens, d_rows, d_lens, n):
    """fixed-stride rows (lens: None for whole rows) through the host or the device front -> (end, bitmap)"""
    if not on_dev:
        return dfa.exec_batch(rows[:n], None if lens is None else lens[:n])
    end, bm = outputs(n)
    dfa.exec_batch_device(d_rows.data_ptr(), rows.shape[1], n, end.data_ptr(), bm.data_ptr(), 0 if lens is None else d_lens.data_ptr())
    return fetched(n, end, bm)


def set_knobs(dfa, hip, mode, seg, pack, early, waves=0):
    for k, v in ((hip.KNOB_INPUT_MODE, mode), (hip.KNOB_SEG, seg), (hip.KNOB_PACK, pack), (hip.KNOB_EARLY_RETIRE, early), (hip.KNOB_WAVES, waves),
                 (hip.KNOB_NOSKIP, 0)):
        dfa.tune(k, v)


def fixed_family(label, L, pol):
    """the kernel family a whole-row batch of stride L runs in under a setting: rows of 48 bytes are no multiple of 64, which
    both staging paths need (fsm_hip.hip pick_cfg), and go to walk_ragged whatever staging path the knob asks for"""
    if label == "generic":
        return ("walk_generic<",)
    if label == "ragged" or L % 64:
        return ("walk_ragged<",)
    if label == "direct":
        return ("walk_direct<", "walk_direct_np<")
    if label == "lds-dma 64":
        return (f"walk_ldsdma<{pol}, 64,",)
    if label == "lds-dma 128":
        return (f"walk_ldsdma<{pol}, 128,",)
    if label == "packing":
        return ("walk_ldsdma_pack<",) if L >= 256 else (f"walk_ldsdma<{pol}, 128,",)
    return ("walk_ldsdma<", "walk_ldsdma_pack<")


# ---- 1. fixed stride: every input mode, skips on and off ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,layout", BOTH, ids=[f"{c}-{l}" for c, l in BOTH])
def test_fixed_stride(hip, name, layout):
    c, dfa = opened(hip, name, layout)
    seen = {}
    for L, part in R.BATCHES:
        if part and c.kind == "pingpong":
            continue
        rows, _, want, d_rows, _ = batch(name, L, False, part)
        n = len(rows)
        for label, mode, seg, pack in SETTINGS:
            fam = fixed_family(label, L, POLS[layout])
            for early in EARLY:
                set_knobs(dfa, hip, mode, seg, pack, early)
                for on_dev in (False, True):
                    end, bm = walk_rows(dfa, on_dev, rows, None, d_rows, None, n)
                    check(end, bm, want, name, layout, L, part, label, early, on_dev, dfa.last_kernel_name())
                    seen[(L, label)] = ran(dfa, layout, fam, name, L, label, early, on_dev)
            # the same switch by its own knob; workgroups of one and of four wavefronts; the row counts around a wavefront
            set_knobs(dfa, hip, mode, seg, pack, 3)
            dfa.tune(hip.KNOB_NOSKIP, 1)
            check(*walk_rows(dfa, True, rows, None, d_rows, None, n), want, name, layout, L, label, "noskip knob")
            for waves in (1, 4):
                for early in (3, 3 | NOSKIP):
                    set_knobs(dfa, hip, mode, seg, pack, early, waves)
                    check(*walk_rows(dfa, True, rows, None, d_rows, None, n), want, name, layout, L, label, early, "waves", waves)
                    ran(dfa, layout, fam, name, L, label, "waves", waves)
            for sub in R.SUBS:
                for early in (-1, 3 | NOSKIP):
                    set_knobs(dfa, hip, mode, seg, pack, early)
                    for on_dev in (False, True):
                        check(*walk_rows(dfa, on_dev, rows, None, d_rows, None, sub), want[:sub], name, layout, L, label, early, on_dev, "n", sub)
    for key, kn in seen.items():
        print(f"{name} {layout} {key}: {kn}")
    dfa.close()


# ---- 2. variable lengths: stride + lengths, packed lines in every metadata form ---------------------------------------------------

OFF0 = 1                                                     # bytes before the first packed line: every line starts at an odd address first


@functools.lru_cache(maxsize=None)
def packed(name, L):
    rows, lens, want, _, d_lens = batch(name, L, True)
    base, off = R.packed_from(rows, lens, OFF0)
    return base, off, off.astype(np.uint32), to_dev(base), to_dev(off), to_dev(off.astype(np.uint32)), to_dev(base[OFF0:])


def walk_packed(dfa, form, on_dev, name, L, n):
    rows, lens, want, _, d_lens = batch(name, L, True)
    base, off, off32, d_base, d_off, d_off32, d_base_l = packed(name, L)
    if not on_dev:
        if form == "u64":
            return dfa.exec_batch_offsets(base, off[:n + 1])
        if form == "u32":
            return dfa.exec_batch_offsets32(base, off32[:n + 1])
        return dfa.exec_batch_lengths(base[OFF0:], lens[:n])
    end, bm = outputs(n)
    if form == "u64":
        dfa.exec_batch_offsets_device(d_base.data_ptr(), d_off.data_ptr(), n, end.data_ptr(), bm.data_ptr())
    elif form == "u32":
        dfa.exec_batch_offsets32_device(d_base.data_ptr(), d_off32.data_ptr(), n, end.data_ptr(), bm.data_ptr())
    else:
        dfa.exec_batch_lengths_device(d_base_l.data_ptr(), d_lens.data_ptr(), n, end.data_ptr(), bm.data_ptr())
    return fetched(n, end, bm)


VAR_MODES = (("default", -1, 0), ("generic", IN_GENERIC, 0), ("generic, walk_generic's own body", IN_GENERIC, NO_LINES32), ("ragged", IN_RAGGED, 0))


@pytest.mark.parametrize("name,layout", BOTH, ids=[f"{c}-{l}" for c, l in BOTH])
def test_variable_lengths(hip, name, layout):
    c, dfa = opened(hip, name, layout)
    seen = {}
    for L in (128, 256):
        rows, lens, want, d_rows, d_lens = batch(name, L, True)
        n = len(rows)
        for label, mode, bit in VAR_MODES:
            for early in EARLY:
                set_knobs(dfa, hip, mode, 0, -1, early | bit)
                for on_dev in (False, True):
                    for form in ("stride + lengths", "u64", "u32", "lengths"):
                        if form == "stride + lengths":
                            end, bm = walk_rows(dfa, on_dev, rows, lens, d_rows, d_lens, n)
                        else:
                            end, bm = walk_packed(dfa, form, on_dev, name, L, n)
                        tag = (name, layout, L, label, early, on_dev, form)
                        check(end, bm, want, *tag, dfa.last_kernel_name())
                        fam = ("walk_ragged<",) if mode == IN_RAGGED else ("walk_ragged<", "walk_generic<", "walk_lines32<") if mode < 0 \
                            else ("walk_generic<",) if bit or form == "stride + lengths" else ("walk_lines32<",)
                        seen[(L, label, form, on_dev)] = ran(dfa, layout, fam, *tag)
        for sub in R.SUBS:                                   # the row counts around a wavefront, skips on and off
            for mode in (IN_GENERIC, IN_RAGGED):
                for early in (3, 3 | NOSKIP):
                    set_knobs(dfa, hip, mode, 0, -1, early)
                    for form in ("stride + lengths", "u64", "lengths"):
                        end, bm = walk_rows(dfa, True, rows, lens, d_rows, d_lens, sub) if form == "stride + lengths" else walk_packed(dfa, form, True, name, L, sub)
                        check(end, bm, want[:sub], name, layout, L, mode, early, form, "n", sub)
    names = set(seen.values())
    for part in ("walk_lines32<", "walk_generic<", "walk_ragged<"):
        assert any(part in s for s in names), (part, names)
    for key, kn in seen.items():
        print(f"{name} {layout} {key}: {kn}")
    dfa.close()


# ---- 3. end-ids where the looping states accept ------------------------------------------------------------------------------------

IDS = [(c, l) for c in ("accepting28", "accepting32") for l in POLS]


@pytest.mark.parametrize("name,layout", IDS, ids=[f"{c}-{l}" for c, l in IDS])
def test_end_ids(hip, name, layout):
    c, dfa = opened(hip, name, layout)
    sets = dfa.ret_sets()
    for L, varlen in ((128, False), (256, True)):
        rows, lens, want, _, _ = batch(name, L, varlen)
        hit = want != NO
        assert hit.sum() >= 1000 and (~hit).sum() >= 1000 and len(set(want[hit].tolist())) == R.K + 1
        lowest = np.array([int(c.oracle.endids(s).min()) for s in range(len(c.dense)) if c.is_end[s]], np.uint32)
        lowest_of = np.zeros(len(c.dense), np.uint32)
        lowest_of[np.nonzero(c.is_end)[0]] = lowest
        for mode_knob in (IN_GENERIC, IN_RAGGED, -1):
            for early in (3, 3 | NOSKIP):
                set_knobs(dfa, hip, mode_knob, 0, -1, early)
                for mode in (hip.IDS_EARLIEST, hip.IDS_RET):
                    ids = dfa.exec_batch_ids(rows, mode, lens if varlen else None)
                    tag = (name, layout, L, varlen, mode_knob, early, mode, dfa.last_kernel_name())
                    assert np.array_equal(ids == NO, ~hit), tag
                    if mode == hip.IDS_EARLIEST:
                        assert np.array_equal(ids[hit], lowest_of[want[hit]]), tag
                    else:
                        for s, k in set(zip(want[hit].tolist(), ids[hit].tolist())):
                            assert k < len(sets) and set(sets[k].tolist()) == set(c.oracle.endids(s).tolist()), (tag, s, k)
                    assert POLS[layout] in dfa.last_kernel_name(), tag
    dfa.close()


# ---- 4. resumed walks: seeded in looping states, in DEAD, in the absorbing ACC ---------------------------------------------------------

RESUMED = [(c, l) for c in ("select28", "select32", "absorbing28", "absorbing32", "startloop32", "pingpong") for l in POLS]


@pytest.mark.parametrize("name,layout", RESUMED, ids=[f"{c}-{l}" for c, l in RESUMED])
def test_resumed_walks(hip, name, layout):
    c, dfa = opened(hip, name, layout)
    L = 128
    rows, _, want, _, _ = batch(name, L)
    n = len(rows)
    start = np.full(n, hip.STATE_START, np.uint32)
    whole = c.oracle.state_walk(rows, start)
    assert np.array_equal(c.end_of_states(whole), want)
    seen = set()
    for cut in (1, 15, 16, 17, L // 2):
        first, rest = np.ascontiguousarray(rows[:, :cut]), np.ascontiguousarray(rows[:, cut:])
        mid = c.oracle.state_walk(first, start)
        k_mid = mid.astype(np.int64) - 1
        if c.kind == "select" and cut > 1:
            looping = (k_mid >= 0) & (k_mid < R.K)
            assert len(set(k_mid[looping].tolist())) == R.K and (mid == hip.STATE_DEAD).sum() >= (16 if cut > 15 else 1)
            if "absorbing" in name and cut >= 17:
                assert (mid == 1 + R.K).sum() >= 1             # ... and rows already in the absorbing ACC
        assert np.array_equal(c.oracle.state_walk(rest, mid), whole)
        for mode in (-1, IN_GENERIC, IN_RAGGED):
            for early in (-1, 1, 1 | NOSKIP):
                set_knobs(dfa, hip, mode, 0, -1, early)
                tag = (name, layout, cut, mode, early)
                st, end = dfa.exec_batch_resume(first, start)
                assert np.array_equal(st, mid) and np.array_equal(end, c.end_of_states(mid)), (tag, "first piece", dfa.last_kernel_name())
                st, end = dfa.exec_batch_resume(rest, mid)                 # seeded with the ORACLE's carried states
                bad = np.nonzero(st != whole)[0]
                assert len(bad) == 0, (tag, "second piece", len(bad), bad[:8].tolist(), st[bad[:8]].tolist(), whole[bad[:8]].tolist(), dfa.last_kernel_name())
                assert np.array_equal(end, want), (tag, "second piece: end states")
                assert POLS[layout] in dfa.last_kernel_name(), tag
                seen.add(dfa.last_kernel_name().split(" (")[0])
                # the second piece as packed lines, each cut to its own length
                lens2 = ((np.arange(n) * 13) % (L - cut + 1)).astype(np.uint32)
                base, off = R.packed_from(rest, lens2, 1)
                st, end = dfa.exec_offsets_resume(base, off, mid)
                want_st = c.oracle.state_walk(rest, mid, lens2)
                assert np.array_equal(st, want_st) and np.array_equal(end, c.end_of_states(want_st)), (tag, "second piece, packed", dfa.last_kernel_name())
    # handed DEAD a row stays dead, handed the absorbing ACC it stays there, whatever it reads
    set_knobs(dfa, hip, -1, 0, -1, -1)
    dead = np.full(n, hip.STATE_DEAD, np.uint32)
    st, end = dfa.exec_batch_resume(rows, dead)
    assert (st == hip.STATE_DEAD).all() and (end == NO).all()
    if "absorbing" in name:
        acc = np.full(n, 1 + R.K, np.uint32)
        st, end = dfa.exec_batch_resume(rows, acc)
        assert (st == 1 + R.K).all() and (end == 1 + R.K).all()
    print(name, layout, "resumed:", sorted(seen))
    dfa.close()


# ---- 5. eager sets: every looping state announces itself ---------------------------------------------------------------------------

EAGER = [(f, l) for f in (0, 4) for l in POLS]


@pytest.mark.parametrize("fillers,layout", EAGER, ids=[f"select{28 + f}-{l}" for f, l in EAGER])
def test_eager_sets(hip, fillers, layout):
    c = R.select(fillers, eager=True)
    dfa = hip.HipDfa(c.flat, getattr(hip, "LAYOUT_" + layout.upper()))
    assert dfa.info()["layout_name"] == layout
    for L, varlen in ((128, False), (256, False), (128, True)):
        rows, lens, _ = R.rows_of(c, L, varlen)
        lens = lens if varlen else None
        _, want_end, want_ids = c.oracle.exec_eager(rows, lens)
        want_words = np.zeros(len(rows), np.uint64)
        for i, ids in enumerate(want_ids):
            for x in ids:
                want_words[i] |= np.uint64(1) << np.uint64(int(x))
        assert len(set(want_words.tolist())) == R.K + int(varlen)  # every L_k (and rows cut before their selector)
        for mode in (-1, IN_DIRECT, IN_LDSDMA, IN_GENERIC, IN_RAGGED):
            for early in (-1, 1, 1 | NOSKIP):
                set_knobs(dfa, hip, mode, 0, -1, early)
                end, words = dfa.exec_eager_words(rows, lens)
                tag = (fillers, layout, L, varlen, mode, early, dfa.last_kernel_name())
                assert np.array_equal(end, want_end), tag
                got = dfa.decode_eager(words)
                bad = [i for i in range(len(rows)) if not np.array_equal(np.sort(got[i]), want_ids[i])]
                assert not bad, (tag, len(bad), bad[:8])
                assert POLS[layout] in dfa.last_kernel_name(), tag
    dfa.close()


# ---- 6. AUTO, whatever it picks, agrees ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_auto_agrees(hip, name):
    c = CASES[name]()
    dfa = hip.HipDfa(c.flat, 0)
    for L in (128, 256):
        rows, _, want, d_rows, _ = batch(name, L)
        for early in (-1, 3 | NOSKIP):
            dfa.tune(hip.KNOB_EARLY_RETIRE, early)
            check(*walk_rows(dfa, False, rows, None, d_rows, None, len(rows)), want, name, "auto", L, early)
            check(*walk_rows(dfa, True, rows, None, d_rows, None, len(rows)), want, name, "auto", L, early, "device")
        rows, lens, want, _, _ = batch(name, L, True)
        for form in ("u64", "u32", "lengths"):
            for on_dev in (False, True):
                check(*walk_packed(dfa, form, on_dev, name, L, len(rows)), want, name, "auto", L, form, on_dev)
    print(name, "auto:", dfa.info()["layout_name"], dfa.last_kernel_name())
    dfa.close()
