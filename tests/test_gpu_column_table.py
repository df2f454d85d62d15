"""GPU (-m gpu): the column-table (FSM_HIP_LAYOUT_TINY) walks on every input path and at their edges -- both images (the 5-bit
form Tiny5Pol for S1 <= 6, the 64-bit nibble form TinyPol<uint64_t> up to S1 = 16, where DEAD is nibble 15 and the state is
carried unmasked), bytes at and above 0x80 in the LDS addresses formed by v_perm_b32, every cell of every lane's private copy,
lanes held in a mid-table state across a resume, walk_ragged's ring in the holes of the 5-bit table at several wavefront
counts and wrapping, and the thread caps that differ inside the family.

Automata, inputs and expected answers are tests/column_table_ref.py (tests/test_column_table_cases.py asserts its conditions
on the CPU): global_ref's judge applied byte by byte in numpy to a closed formula is the only judge.  Nothing is compared with
another layout, kernel, knob setting or front of the library, and the oracle's table walk is not used.

Every output buffer is two entries longer than the batch and pre-filled with junk; nothing behind the batch may be written
(tests/walk_buffers.py).  After the first launch of every configuration the kernel that ran (fsm_hip_last_kernel_name) is held
against expected(): fsm_hip.hip pick_cfg + launch.h launch_pol restated for a plain walk on a column table, and the LDS the
library reports (info()["lds_bytes"]) against lds_expected()."""
import functools
import time

import numpy as np
import pytest

import global_ref as G
import column_table_ref as R
import walk_buffers
from walk_buffers import (DEFAULT, IN_DIRECT, IN_GENERIC, IN_LDSDMA, IN_RAGGED, JUNK32, NO_LINES32, PACKED_FORMS, SETTINGS, Buf, Out, Packed, call,
                          set_knobs, walk_rows)

pytestmark = pytest.mark.gpu

NO = R.NO
N, L = R.N, R.L
LDS_LIMIT = 163840                                       # all of a workgroup's LDS on this device
TABLE = R.TABLE_LDS                                      # 65 536 bytes in both forms: 64 copies of 4 bytes, or 32 of 8, of 256 columns
DMA_TILE = 8192                                          # per wavefront: an LDS-DMA tile of 128-byte segments
RAGGED_WAVE = {5: 8192, 64: 8192 + 64 * 16 + 1024}       # walk_ragged's tile; its ring and row records lie in the 5-bit table's holes, else behind the tile
RAGGED_WAVES = {5: 12, 64: 9}                            # ... wavefronts of it beside the table: 65 536 + 12 * 8 192 = 163 840 = 65 536 + 9.6 * 10 240
POL = {5: "fsmhip::Tiny5Pol", 64: "fsmhip::TinyPol<unsigned long>"}
PACK_THREADS = {5: 1024, 64: 768}                        # launch.h ldsdma_pack_threads
assert walk_buffers.OFF0 == R.OFF0


def form_of(c):
    """which image the planner keeps: the 5-bit form for five states + DEAD and fewer, else the 64-bit one"""
    return 5 if c.S + 1 <= 6 else 64


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()
    assert G.LIB_DEAD == libfsm_amd.STATE_DEAD and G.LIB_START == libfsm_amd.STATE_START
    assert (libfsm_amd.IN_DIRECT, libfsm_amd.IN_LDSDMA, libfsm_amd.IN_GENERIC, libfsm_amd.IN_RAGGED) == (IN_DIRECT, IN_LDSDMA, IN_GENERIC, IN_RAGGED)
    return libfsm_amd


# ---- which kernel: fsm_hip.hip pick_cfg and launch.h launch_pol, restated ------------------------------------------------------

def expected(form, k, stride, fast, short=False, resumed=False, early=3, packed_plain=False):
    """the kernel's name as far as the launch decides it.  form: 5 or 64; k: the knobs; fast: whole rows, 16 | stride, aligned
    base (and the input-mode knob not IN_GENERIC); short: the front knows (host) or finds (device, no input-mode knob) the
    mean length below the pick threshold; early: WalkArgs::early; packed_plain: a packed front asking for end states / the
    bitmap alone, whose per-lane kernel is walk_lines32 unless bit 5 of `early` says otherwise.

    pick_cfg for this family: four wavefronts of walk_ragged always fit beside the 64 KiB table, so a batch that is not short
    takes walk_ragged, a short one a per-lane kernel; IN_GENERIC and IN_RAGGED by knob always.  A fast batch takes LDS-DMA by
    default (twelve 8 KiB tiles fit exactly; the family takes it whatever fits), or whichever of the two the knob asks; LDS-DMA
    needs 64 | stride (segments of 64 unless 128 | stride and the knob does not say 64), per-lane loads 64 | stride too (8
    chunks in flight where 128 | stride, 4 by knob or without prefetch), and a stride that is neither leaves the choice of the
    first line.  The packing kernel: LDS-DMA, 128-byte segments, stride >= 256, not resumed, FSM_HIP_KNOB_PACK != 0 -- and bit
    1 of `early` or the knob at 1 (launch_walk); compiled for 768 threads on the 64-bit form, 1024 on the 5-bit one."""
    pol = POL[form]
    assert TABLE + 4 * RAGGED_WAVE[form] <= LDS_LIMIT and TABLE + 12 * DMA_TILE <= LDS_LIMIT
    mode = "generic" if short else "ragged"
    seg, nb, pre, nt = 128, 8, k.pre != 0, k.nt != 0
    if k.mode in (IN_GENERIC, IN_RAGGED):
        mode = "generic" if k.mode == IN_GENERIC else "ragged"
    elif fast:
        m = "dma"
        if k.mode in (IN_DIRECT, IN_LDSDMA):
            m = "direct" if k.mode == IN_DIRECT else "dma"
        if m == "dma" and stride % 64:
            m = "direct"
        if m == "dma":
            seg = 64 if k.seg == 64 or stride % 128 else 128
        if m == "direct":
            nb = k.nb if k.nb in (4, 8) else 8
            if not pre or (stride // 16) % 8:
                nb = 4
            if (stride // 16) % 4:
                m = None
        if m:
            mode = m
    pack = mode == "dma" and seg == 128 and not resumed and stride >= 256 and k.pack != 0 and ((early & 2) or k.pack >= 1)
    if mode == "dma":
        return f"walk_ldsdma_pack<{pol}, {2 if nt else 0}, {PACK_THREADS[form]}>" if pack else f"walk_ldsdma<{pol}, {seg}, {2 if nt and seg == 128 else 0}, 1024>"
    if mode == "direct":
        return f"walk_direct_np<{pol}, 4>" if not pre and nb == 4 else f"walk_direct<{pol}, {nb}, 1>"
    if mode == "ragged":
        return f"walk_ragged<{pol}, 768"
    return f"walk_lines32<{pol}, " if packed_plain and not (early & NO_LINES32) else f"walk_generic<{pol}, "


def lds_expected(form, k, waves=0):
    """info()["lds_bytes"]: pick_cfg for whole 1 KiB rows under the knobs -- the table, and behind it one tile per wavefront:
    LDS-DMA 12 x 8 192 (128-byte segments: 16 do not fit, 14 neither) or 16 x 4 096, walk_ragged 12 x 8 192 in the 5-bit
    form and 9 x 10 240 in the 64-bit one (or `waves` by knob); the per-lane kernels keep the table alone"""
    if k.mode == IN_RAGGED:
        return TABLE + (waves or RAGGED_WAVES[form]) * RAGGED_WAVE[form]
    if k.mode in (IN_GENERIC, IN_DIRECT):
        return TABLE
    return TABLE + (16 * 4096 if k.seg == 64 else 12 * DMA_TILE)


def ran(dfa, want, form, *tag):
    kn = dfa.last_kernel_name()
    assert want in kn and POL[form] in kn and POL[69 - form] not in kn, (tag, "expected", want, "ran", kn)
    return kn


def opened(hip, c, flags, extra=0):
    """HipDfa(flat) or HipDfa(flat, LAYOUT_TINY): a column table either way -> (dfa, 5 or 64)"""
    dfa = hip.HipDfa(c.flat, flags | extra)
    assert dfa.info()["layout_name"] == "tiny", (c.name, flags, dfa.info()["layout_name"])
    form = form_of(c)
    for k in (DEFAULT, SETTINGS[-2], SETTINGS[-1]):      # default (LDS-DMA, 128-byte segments), per-lane, walk_ragged
        dfa.tune(hip.KNOB_INPUT_MODE, k.mode)
        assert dfa.info()["lds_bytes"] == lds_expected(form, k), (c.name, k.label, dfa.info())
    dfa.tune(hip.KNOB_INPUT_MODE, -1)
    return dfa, form


def early_of(c):
    return 3 if c.absorbing(c.tr).any() else 1           # bit 1 (the per-lane load skip) only where an absorbing state is reachable


@functools.lru_cache(maxsize=None)
def strided(stride):
    """the pool's rows cut to `stride` bytes, their lengths clipped to it"""
    rows, lens, _ = R.pool()
    short = np.minimum(lens, stride).astype(np.uint32)
    return Buf(rows[:, :stride], 64), Buf(short), short


def took(t0, *what):
    print("wall time", *what, f"{time.time() - t0:.2f} s")


# ---- 1. fixed stride, every input mode -----------------------------------------------------------------------------------------------

FIXED = [("five", False), ("five", True), ("six", False), ("fifteen", False), ("fifteen", True), ("complete15", False)]


def test_the_lds_the_library_reports(hip):
    """163 840 for `five` under walk_ragged (12 wavefronts, tiles of 8 192, ring and row records in the holes), 163 840 for both
    forms behind LDS-DMA with 128-byte segments, 65 536 + 9 * 10 240 for `six` under walk_ragged"""
    assert lds_expected(5, SETTINGS[-1]) == 163840 == lds_expected(5, DEFAULT) == lds_expected(64, DEFAULT)
    assert lds_expected(64, SETTINGS[-1]) == 65536 + 9 * 10240 == 157696
    for name in ("five", "six"):
        dfa, form = opened(hip, R.case(name), 0)
        for k in SETTINGS:
            set_knobs(dfa, hip, k)
            info = dfa.info()
            assert info["lds_bytes"] == lds_expected(form, k), (name, k.label, info)
            if k.mode == IN_RAGGED:
                assert info["waves_per_block"] == RAGGED_WAVES[form], (name, info)
            elif k.mode < 0 or (k.mode == IN_LDSDMA and k.seg != 64):
                assert info["waves_per_block"] == 12, (name, k.label, info)
            print(name, k.label, info["lds_bytes"], info["waves_per_block"])
        dfa.close()


@pytest.mark.parametrize("name,forced", FIXED, ids=[f"{a}-{'forced' if f else 'auto'}" for a, f in FIXED])
def test_fixed_stride_every_input_mode(hip, name, forced):
    t0 = time.time()
    c = R.case(name)
    dfa, form = opened(hip, c, hip.LAYOUT_TINY if forced else 0)
    early = early_of(c)
    seen = {}
    for k in SETTINGS:
        set_knobs(dfa, hip, k)
        assert dfa.info()["lds_bytes"] == lds_expected(form, k), (name, k.label, dfa.info())
        for stride in R.STRIDES:
            rows, lens, short = strided(stride)
            want_all, want_len = c.ends(c.tr[:, stride]), c.ends(c.at(short))
            for with_lens in (False, True):
                fast = not with_lens and stride % 16 == 0
                for dev in (False, True):
                    for n in R.SUBS:
                        o = Out(n, dev)
                        walk_rows(dfa, dev, rows, stride, lens if with_lens else None, n, o)
                        o.check((want_len if with_lens else want_all)[:n], name, forced, k.label, stride, with_lens, dev, n, dfa.last_kernel_name())
                        # rows + lengths: a host front knows the mean, the device finds it where no input-mode knob is set (and
                        # walk_ragged is the other candidate); below 96 bytes the batch goes to a per-lane kernel
                        is_short = with_lens and int(short[:n].sum()) // n < 96 and (not dev or k.mode < 0)
                        kn = ran(dfa, expected(form, k, stride, fast, is_short, early=early), form, name, forced, k.label, stride, with_lens, dev, n)
                        seen[(k.label, stride, with_lens)] = kn.split(" (")[0]           # (the whole pool's: the last sub-batch)
    for key, kn in seen.items():
        print(f"{name} {'forced' if forced else 'auto'} {key}: {kn}")
    dfa.close()
    took(t0, "fixed stride", name, forced)


@pytest.mark.parametrize("name", ["one", "two"])
def test_the_smallest_tables(hip, name):
    """S1 = 2 and 3: stride 256 and 37, the whole pool, default knobs and walk_ragged by knob"""
    t0 = time.time()
    c = R.case(name)
    dfa, form = opened(hip, c, 0)
    assert form == 5
    for k in (DEFAULT, SETTINGS[-1]):
        set_knobs(dfa, hip, k)
        for stride in (256, 37):
            rows, lens, short = strided(stride)
            for with_lens, want in ((False, c.ends(c.tr[:, stride])), (True, c.ends(c.at(short)))):
                assert 0.05 * N < int((want != NO).sum()) < 0.95 * N
                for dev in (False, True):
                    o = Out(N, dev)
                    walk_rows(dfa, dev, rows, stride, lens if with_lens else None, N, o)
                    o.check(want, name, k.label, stride, with_lens, dev, dfa.last_kernel_name())
                    is_short = with_lens and int(short.sum()) // N < 96 and (not dev or k.mode < 0)
                    kn = ran(dfa, expected(form, k, stride, not with_lens and stride % 16 == 0, is_short, early=early_of(c)), form, name, k.label, stride, with_lens, dev)
                    print(f"{name} {k.label} stride {stride} {'rows + lens' if with_lens else 'rows'} {'device' if dev else 'host'}: {kn.split(' (')[0]}")
    dfa.close()
    took(t0, "smallest tables", name)


# ---- 2. variable-length fronts -----------------------------------------------------------------------------------------------------

VARLEN = ["five", "six", "fifteen"]
VAR_WAVES = {"five": (1, 7), "six": (1, 9), "fifteen": ()}     # walk_ragged by knob also at these wavefront counts


@pytest.mark.parametrize("name", VARLEN)
def test_variable_length_fronts(hip, name):
    t0 = time.time()
    c = R.case(name)
    rows = R.pool()[0]
    dfa, form = opened(hip, c, 0)
    batches = [(which, lens, n) for which, lens in R.edge_batches().items() for n in ((65, N) if which == "head" else (N,))]
    seen = {}
    #          input mode, pick mean, early knob, KNOB_WAVES: which kernel
    picks = [("default", -1, -1, -1, 0), ("mean above the threshold", -1, None, -1, 0), ("mean below the threshold", -1, None, -1, 0),
             ("per-lane by knob", IN_GENERIC, -1, -1, 0), ("per-lane by knob, walk_generic's own body", IN_GENERIC, -1, 3 | NO_LINES32, 0),
             ("ragged by knob", IN_RAGGED, -1, -1, 0)]
    # in the holes the address of a ring entry depends on the wavefront's index: one wavefront, an odd count, the most there are
    picks += [(f"ragged by knob, {w} wavefronts", IN_RAGGED, -1, -1, w) for w in VAR_WAVES[name]]
    for which, lens, n in batches:
        pk = Packed(rows, lens, n)
        assert pk.base.a.size == pk.total == R.OFF0 + int(np.asarray(lens[:n], np.int64).sum())       # the device text is exactly off[n] bytes long
        want = c.ends(c.at(lens[:n]))
        lo, hi = pk.mean(True, "u64 offsets"), pk.mean(False, "u64 offsets") + 1         # no front finds the mean below lo, every one below hi
        for label, mode, pm, ek, waves in picks:
            pm = lo if "above" in label else hi if "below" in label else pm
            dfa.tune(hip.KNOB_INPUT_MODE, mode)
            dfa.tune(hip.KNOB_PICK_MEAN, pm)
            dfa.tune(hip.KNOB_EARLY_RETIRE, ek)
            dfa.tune(hip.KNOB_WAVES, waves)
            k = DEFAULT._replace(mode=mode)
            if mode == IN_RAGGED:
                info = dfa.info()
                assert info["waves_per_block"] == (waves or RAGGED_WAVES[form]) and info["lds_bytes"] == lds_expected(form, k, waves), (name, label, info)
            for pform in PACKED_FORMS:
                for dev in (False, True):
                    o = Out(n, dev)
                    pk.walk(dfa, dev, pform, o)
                    o.check(want, name, which, n, label, pform, dev, dfa.last_kernel_name())
                    # the threshold: the knob, else 128 where walk_lines32 is the per-lane kernel the front counts on (the plain
                    # packed fronts; on the device every packed front below 4 GiB), 96 elsewhere (the host's packed_all)
                    thr = pm if pm >= 0 else 128 if (dev or not pform.startswith("packed_all")) else 96
                    is_short = mode < 0 and pk.mean(dev, pform) < thr
                    kn = ran(dfa, expected(form, k, 0, False, is_short, early=3 if ek < 0 else ek, packed_plain=True), form, name, which, n, label, pform, dev)
                    if dev and mode < 0:
                        assert "on the device" in kn, kn          # the candidates were launched, the batch's mean chose
                    seen[(label, pform, dev)] = kn.split(" (")[0]
    dfa.tune(hip.KNOB_EARLY_RETIRE, -1)
    dfa.tune(hip.KNOB_WAVES, 0)
    names = set(seen.values())
    assert any("walk_lines32<" in s for s in names), names
    assert len({s for s in names if "walk_generic<" in s}) == 3, names      # one instantiation per metadata form
    assert any("walk_ragged<" in s for s in names), names
    for key, kn in seen.items():
        print(f"{name} {key}: {kn}")
    dfa.close()
    took(t0, "variable-length fronts", name)


# ---- 3. the ring wraps --------------------------------------------------------------------------------------------------------------

RING_LEN = 40


@pytest.mark.parametrize("name", ["five", "fifteen"])
def test_the_ring_wraps(hip, name):
    """walk_ragged's ring holds 64 inputs and is topped up 32 at a time; a wavefront gets more than 64 inputs only where the
    batch has more than 64 x CUs x blocks_per_cu x waves of them (the grid is min(ceil(tiles / waves), CUs x blocks_per_cu), a
    wavefront's range ceil(words / wavefronts) bitmap words).  `five`: the ring lies in the table's holes, in rows 16 w ..
    16 w + 15 of wavefront w -- rows that the batch's bytes (uniformly random) index all the time; `fifteen`: behind the tile."""
    import torch
    t0 = time.time()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    c = R.case(name)
    dfa, form = opened(hip, c, 0)
    dfa.tune(hip.KNOB_INPUT_MODE, IN_RAGGED)
    dfa.tune(hip.KNOB_BLOCKS_PER_CU, 1)
    k = DEFAULT._replace(mode=IN_RAGGED)
    full = RAGGED_WAVES[form]
    for label, waves, n in (("one wavefront", 1, 200 * cus), ("default wavefronts", 0, 64 * cus * full * 2 + 777)):
        dfa.tune(hip.KNOB_WAVES, waves)
        w = waves or full
        info = dfa.info()
        assert info["waves_per_block"] == w and info["lds_bytes"] == lds_expected(form, k, waves), (name, label, info)
        # inputs per wavefront, as the kernel partitions the batch: more than the ring holds, so that it wraps
        words = (n + 63) // 64
        grid = min((words + w - 1) // w, cus)
        per = (words + grid * w - 1) // (grid * w) * 64
        assert grid == cus and per >= 192, (name, label, grid, per)
        rng = np.random.RandomState(1000 + w)
        rows = rng.randint(0, 256, (n, RING_LEN)).astype(np.uint8)
        lens = rng.randint(0, RING_LEN + 1, n).astype(np.uint32)
        lens[:len(R.EDGE_LENS)] = R.EDGE_LENS
        tr = G.trace(c.dense, c.cls, 0, rows)                 # ONE trace over 40 columns
        want = c.ends(tr[np.arange(n), lens.astype(np.int64)])
        hits = int((want != NO).sum())
        assert 0.10 * n < hits < 0.90 * n, (name, label, hits, n)
        assert float((rows >= 0x80).mean()) >= 0.40
        pk = Packed(rows, lens, n)
        o = Out(n, True)
        pk.walk(dfa, True, "u64 offsets", o)
        o.check(want, name, label, n, dfa.last_kernel_name())       # every end state and every bitmap word
        kn = ran(dfa, expected(form, k, 0, False, packed_plain=True), form, name, label, n)
        print(f"{name} {label}: {n} inputs, {pk.total} bytes, {grid} x {w} wavefronts of {per} inputs, {hits} hits: {kn.split(' (')[0]}")
    dfa.close()
    took(t0, "the ring wraps", name)


# ---- 4. end-ids ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["five", "six", "fifteen"])
def test_end_ids(hip, name):
    t0 = time.time()
    c = R.case(name)
    rows_np, lens_np, _ = R.pool()
    dfa, form = opened(hip, c, 0)
    sets = dfa.ret_sets()                                   # fsm_hip_ret_get: what an IDS_RET index stands for
    rows, lens, _ = strided(L)
    for n in (129, N):
        pk = Packed(rows_np, lens_np, n)
        for batch, want_st in (("rows", c.st_all[:n]), ("rows + lens", c.st_len[:n]), ("offsets", c.st_len[:n])):
            want = c.ends(want_st)
            hit = want != NO
            assert hit.sum() >= 5 and (~hit).sum() >= 5
            for mode in (hip.IDS_EARLIEST, hip.IDS_RET):
                for dev in (False, True):
                    o = Out(n, dev, ids=True)
                    if batch == "offsets":
                        call("fsm_hip_exec_batch_ids_offsets", dev, dfa, pk.base.p(dev), pk.off.p(dev), n, mode, o.p("ids"))
                        kn = ran(dfa, expected(form, DEFAULT, 0, False, pk.mean(dev, "u64 offsets") < 96), form, name, batch, mode, dev, n)
                    else:
                        call("fsm_hip_exec_batch_ids", dev, dfa, rows.p(dev), L, lens.p(dev) if batch == "rows + lens" else None, n, mode, o.p("ids"))
                        kn = ran(dfa, expected(form, DEFAULT, L, batch == "rows", batch != "rows" and int(lens_np[:n].sum()) // n < 96), form, name, batch, mode, dev, n)
                    tag = (name, batch, mode, dev, n, kn)
                    if dev:
                        import torch
                        torch.cuda.synchronize()
                        o.a["ids"] = o.t["ids"].cpu().numpy().view(np.uint32)
                    ids = o.a["ids"]
                    assert (ids[n:] == JUNK32).all(), (tag, "ids behind the batch written")
                    ids = ids[:n]
                    assert not (ids == JUNK32).any() and np.array_equal(ids == NO, ~hit), tag       # every entry written; an id where the row is accepted
                    if mode == hip.IDS_EARLIEST:
                        assert np.array_equal(ids[hit], c.slots[want[hit].astype(np.int64), 0].astype(np.uint32)), tag
                    else:
                        for s, k2 in set(zip(want[hit].tolist(), ids[hit].tolist())):
                            assert k2 < len(sets) and set(sets[k2].tolist()) == set(c.ids_of(s).tolist()), (tag, s, k2)
                    if n == N and mode == hip.IDS_RET:
                        print(f"{name} ids {batch} {'device' if dev else 'host'}: {kn.split(' (')[0]}")
    dfa.close()
    took(t0, "end-ids", name)


# ---- 5. resumed walks ---------------------------------------------------------------------------------------------------------------

META = {"u64 offsets": 0, "u32 offsets": 1, "lengths": 2}


def resume(dfa, dev, form, rows, lens, pk, n, o):
    if form == "stride":
        args = (rows.p(dev), L, lens.p(dev), n, o.p("st"), o.p("end"))
        call("fsm_hip_exec_batch_resume", dev, dfa, *args, *((o.p("bm"),) if dev else ()))
    elif form == "offsets":
        call("fsm_hip_exec_batch_resume_offsets", dev, dfa, pk.base.p(dev), pk.off.p(dev), n, o.p("st"), o.p("end"), *((o.p("bm"),) if dev else ()))
    else:
        base, meta = (pk.base_l, pk.lens) if form == "lengths" else (pk.base, pk.off if form == "u64 offsets" else pk.off32)
        call("fsm_hip_exec_batch_resume_packed", dev, dfa, base.p(dev), META[form], meta.p(dev), n, o.p("st"), o.p("end"), *((o.p("bm"),) if dev else ()))


@pytest.mark.parametrize("name", ["five", "six", "fifteen"])
def test_resumed_walks(hip, name):
    t0 = time.time()
    c = R.case(name)
    rows_np, _, cut = R.pool()
    dfa, form = opened(hip, c, 0)
    start = np.full(N, hip.STATE_START, np.uint32)
    first_rows, first_lens, rest_rows, rest_lens = Buf(rows_np, 64), Buf(cut), Buf(c.rest, 64), Buf(c.rest_lens)
    car_cut, car_all = G.carried(c.st_cut), G.carried(c.st_all)
    end_cut, end_all = c.ends(c.st_cut), c.ends(c.st_all)
    assert (c.rest_lens == 0).sum() >= 1 and (car_cut == hip.STATE_DEAD).sum() >= 50
    # a lane is held in EVERY state across the resume: mid-table states, the sink and DEAD
    assert sorted(set(car_cut.tolist())) == list(range(c.S)) + [hip.STATE_DEAD]
    seen = {}
    for n in R.SUBS:
        pk1, pk2 = Packed(rows_np, cut, n), Packed(c.rest, c.rest_lens, n)
        for rform in ("stride", "offsets") + tuple(META):
            for dev in (False, True):
                tag = (name, rform, dev, n)
                o = Out(n, dev, state=start)
                resume(dfa, dev, rform, first_rows, first_lens, pk1, n, o)
                o.check(end_cut[:n], *tag, "first piece", carried=car_cut[:n], bitmap=dev)
                # (a resumed front holds the mean against 96 bytes; the device finds it)
                mean = int(cut[:n].sum()) // n if rform == "stride" else pk1.mean(dev, rform if rform != "offsets" else "u64 offsets")
                kn = ran(dfa, expected(form, DEFAULT, L if rform == "stride" else 0, False, mean < 96, resumed=True), form, *tag)
                seen[(rform, dev)] = kn.split(" (")[0]
                # the second piece from the JUDGE's carried states: it ends where the whole row ends
                o = Out(n, dev, state=car_cut)
                resume(dfa, dev, rform, rest_rows, rest_lens, pk2, n, o)
                o.check(end_all[:n], *tag, "second piece", carried=car_all[:n], bitmap=dev)
    # every row handed each state in turn -- every q of the automaton and DEAD: the judge walks the same bytes from q.  The whole
    # pool's mean is above the threshold (walk_ragged); the resumed per-lane kernel takes the same batches by knob
    pk1 = Packed(rows_np, cut, N)
    for q in c.states():
        handed = np.full(N, hip.STATE_DEAD if q < 0 else q, np.uint32)
        st = G.walk(c.dense, c.cls, 0, rows_np, cut, state_in=np.full(N, q, np.int64))
        if q < 0 or q >= c.S - c.sinks:
            assert (st == q).all()                           # DEAD stays dead and the sink stays the sink, whatever is read
        else:
            assert len(np.unique(st)) >= min(c.S, 4)
        for mode in (-1, IN_GENERIC):
            dfa.tune(hip.KNOB_INPUT_MODE, mode)
            for rform, dev in (("stride", False), ("stride", True), ("lengths", True), ("u32 offsets", False), ("offsets", True)):
                o = Out(N, dev, state=handed)
                resume(dfa, dev, rform, first_rows, first_lens, pk1, N, o)
                o.check(c.ends(st), name, "handed", q, mode, rform, dev, dfa.last_kernel_name(), carried=G.carried(st), bitmap=dev)
                kn = ran(dfa, expected(form, DEFAULT._replace(mode=mode), L if rform == "stride" else 0, False, resumed=True), form, name, "handed", q, mode, rform, dev)
                seen[("handed a state", "per-lane by knob" if mode >= 0 else "default", rform, dev)] = kn.split(" (")[0]
    dfa.tune(hip.KNOB_INPUT_MODE, -1)
    assert any("walk_ragged<" in s for s in seen.values()) and any("walk_generic<" in s for s in seen.values()), seen
    for key, kn in seen.items():
        print(f"{name} resumed {key}: {kn}")
    dfa.close()
    took(t0, "resumed walks", name)


# ---- 6. every cell of every copy ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["five", "fifteen"])
def test_every_cell_of_every_copy(hip, name):
    """64 x 256 x S1 one-byte inputs through the resumed per-lane kernel: input i has byte (i // 64) % 256 and is handed state
    i // (64 x 256), DEAD last -- each lane of a wavefront meets every byte from every state, so every cell of every lane's
    private copy of every column is read, and judged by dense[][] itself.  Then the same bytes from the start state through the
    plain packed fronts (walk_lines32, walk_generic's own body, walk_ragged: lanes 32 to 63 on copies 0 to 31 there)."""
    t0 = time.time()
    c = R.case(name)
    dfa, form = opened(hip, c, 0)
    S1 = c.S + 1
    n = 64 * 256 * S1
    i = np.arange(n)
    byte = ((i // 64) % 256).astype(np.uint8)
    q = i // (64 * 256)
    tab = np.vstack([c.dense, np.full((1, c.dense.shape[1]), -1, np.int64)])      # row S: DEAD stays DEAD
    nxt = tab[q, c.cls[byte]]
    handed = np.where(q == c.S, hip.STATE_DEAD, q).astype(np.uint32)
    assert sorted(set(nxt.tolist())) == list(range(-1, c.S))                      # every state is some cell's answer
    pk = Packed(byte[:, None], np.ones(n, np.uint32), n)
    dfa.tune(hip.KNOB_INPUT_MODE, IN_GENERIC)
    o = Out(n, True, state=handed)
    resume(dfa, True, "lengths", None, None, pk, n, o)
    o.check(c.ends(nxt), name, "resumed", carried=G.carried(nxt), bitmap=True)
    kn = ran(dfa, f"walk_generic<{POL[form]}, ", form, name, "resumed")
    print(f"{name} every cell, resumed, {n} inputs: {kn.split(' (')[0]}")
    # ... and from the start state: 64 x 256 inputs
    n0 = 64 * 256
    pk = Packed(byte[:n0, None], np.ones(n0, np.uint32), n0)
    want = c.ends(nxt[:n0])
    assert 0.05 * n0 < int((want != NO).sum()) < 0.95 * n0
    for label, mode, ek in (("default", -1, -1), ("walk_generic's own body", IN_GENERIC, 3 | NO_LINES32), ("ragged by knob", IN_RAGGED, -1)):
        dfa.tune(hip.KNOB_INPUT_MODE, mode)
        dfa.tune(hip.KNOB_EARLY_RETIRE, ek)
        for pform in PACKED_FORMS[:3]:
            o = Out(n0, True)
            pk.walk(dfa, True, pform, o)
            o.check(want, name, label, pform, dfa.last_kernel_name())
            kn = ran(dfa, expected(form, DEFAULT._replace(mode=mode), 0, False, mode < 0, early=3 if ek < 0 else ek, packed_plain=True), form, name, label, pform)
            print(f"{name} every cell, {label}, {pform}: {kn.split(' (')[0]}")
    dfa.close()
    took(t0, "every cell of every copy", name)


# ---- 7. absorbing lanes ---------------------------------------------------------------------------------------------------------------

ABS_SETTINGS = tuple(k for k in SETTINGS if k.label in ("lds-dma 64", "lds-dma 128, nontemporal", "lds-dma 128, temporal", "direct, no prefetch",
                                                         "packing, nontemporal", "packing, temporal"))


@pytest.mark.parametrize("name", ["five", "six", "fifteen"])
def test_absorbing_lanes(hip, name):
    t0 = time.time()
    c = R.case(name)
    subs = (129, N)
    R.bites(c, 129, bands=0.05)                              # what makes this group bite, for the rows actually launched
    R.bites(c, N)
    for what, st in (("L", c.st_all), ("lens", c.st_len)):
        assert sorted(set(st.tolist())) == list(range(-1, c.S)), (name, what)
    seen = {}
    pol = POL[form_of(c)]
    for create, knob in ((hip.NO_EARLY_RETIRE, -1), (0, 1), (0, 3), (0, -1)):
        dfa, form = opened(hip, c, 0, create)
        dfa.tune(hip.KNOB_EARLY_RETIRE, knob)
        early = knob if knob >= 0 else 0 if create else 3
        for k in ABS_SETTINGS:
            set_knobs(dfa, hip, k)
            for stride in (256, 192):
                rows, lens, short = strided(stride)
                for with_lens, want in ((False, c.ends(c.tr[:, stride])), (True, c.ends(c.at(short)))):
                    if with_lens and k is not ABS_SETTINGS[0]:
                        continue                               # (rows + lengths take no staging knob: once per handle)
                    for dev in (False, True):
                        for n in subs:
                            o = Out(n, dev)
                            walk_rows(dfa, dev, rows, stride, lens if with_lens else None, n, o)
                            o.check(want[:n], name, create, knob, k.label, stride, with_lens, dev, n, dfa.last_kernel_name())
                            is_short = with_lens and int(short[:n].sum()) // n < 96 and not dev      # (an input-mode knob is set: the device front does not ask)
                            kn = ran(dfa, expected(form, k, stride, not with_lens, is_short, early=early), form, name, create, knob, k.label, stride, with_lens, dev, n)
                            seen[(early, k.label, stride, with_lens)] = kn.split(" (")[0]
        dfa.close()
    ks = set(seen.values())
    for part in (f"walk_ldsdma<{pol}, 64,", f"walk_ldsdma<{pol}, 128,", f"walk_direct_np<{pol}", f"walk_ldsdma_pack<{pol}, 2, {PACK_THREADS[form]}>",
                 f"walk_ldsdma_pack<{pol}, 0, {PACK_THREADS[form]}>"):
        assert any(part in s for s in ks), (part, ks)
    for key, kn in seen.items():
        print(f"{name} early={key[0]} {key[1:]}: {kn}")
    took(t0, "absorbing lanes", name)
