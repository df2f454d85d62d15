"""GPU (-m gpu): the pair-table (FSM_HIP_LAYOUT_LDS2, Lds2Pol) walks on every input path and at their edges -- lone bytes
through the identity class (odd lengths, unaligned heads and tails), a lane turning absorbing on either byte of a pair, the
largest 16-bit table, the hand-over to a second image, and staging paths asked for by knob beside a table that nearly fills LDS.

Automata, inputs and expected answers are tests/pair_table_ref.py (tests/test_pair_table_cases.py asserts its conditions on
the CPU): global_ref's closed formula applied byte by byte in numpy is the only judge.  Nothing is compared with another
layout, kernel, knob setting or front of the library, and the oracle's table walk is not used.

Every output buffer is two entries longer than the batch and pre-filled with junk; nothing behind the batch may be written.
After the first launch of every configuration the kernel that ran (fsm_hip_last_kernel_name) is held against expected():
fsm_hip.hip pick_cfg + launch.h launch_pol restated for a plain walk on the pair table."""
import functools

import numpy as np
import pytest

import global_ref as G
import pair_table_ref as R
# the buffers, calls and knob settings this suite shares with tests/test_gpu_column_table.py
from walk_buffers import (DEFAULT, IN_DIRECT, IN_GENERIC, IN_LDSDMA, IN_RAGGED, JUNK32, NO_LINES32, PACKED_FORMS, SETTINGS, Buf, Out, Packed, call,
                          set_knobs, walk_rows)

pytestmark = pytest.mark.gpu

NO = R.NO
N, L = R.N, R.L
LDS_LIMIT = 163840                                       # all of a workgroup's LDS on this device
DMA_TILE, RAGGED_WAVE = 8192, 8192 + 64 * 16 + 1024      # per wavefront: an LDS-DMA tile of 128-byte segments; walk_ragged's tile + ring + row records
HAND_OVER = LDS_LIMIT - 8 * RAGGED_WAVE                  # 81 920: a pair table (with its byte map) above it keeps a second image
POL = "fsmhip::Lds2Pol"


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

def expected(tl, k, stride, fast, short=False, resumed=False, early=3, packed_plain=False):
    """the kernel's name as far as the launch decides it.  tl: the table's LDS (byte map + table); k: the knobs; fast: whole
    rows, 16 | stride, aligned base (and the input-mode knob not IN_GENERIC); short: the front knows (host) or finds (device,
    no input-mode knob) the mean length below the pick threshold; early: WalkArgs::early; packed_plain: a packed front asking
    for end states / the bitmap alone, whose per-lane kernel is walk_lines32 unless bit 5 of `early` says otherwise.

    pick_cfg: walk_ragged where four wavefronts' tiles fit beside the table and the batch is not short, else a per-lane kernel;
    IN_GENERIC by knob always, IN_RAGGED by knob where it fits; else for `fast` batches LDS-DMA where twelve 8 KiB tiles fit,
    per-lane loads otherwise, or whichever of the two the knob asks; LDS-DMA needs 64 | stride (segments of 64 unless 128 |
    stride and the knob does not say 64), per-lane loads 64 | stride too (8 chunks in flight where 128 | stride, 4 by knob or
    without prefetch), and a stride that is neither leaves the choice of the first line.  A staging path beside a table that
    leaves no room for ONE wavefront's tile falls to the per-lane kernel of its class.  The packing kernel: LDS-DMA, 128-byte
    segments, stride >= 256, not resumed, FSM_HIP_KNOB_PACK != 0 -- and bit 1 of `early` or the knob at 1 (launch_walk)."""
    ragged_fits = tl + 4 * RAGGED_WAVE <= LDS_LIMIT
    mode = "ragged" if ragged_fits and not short else "generic"
    seg, nb, pre, nt = 128, 8, k.pre != 0, k.nt != 0
    if k.mode == IN_GENERIC or (k.mode == IN_RAGGED and ragged_fits):
        mode = "generic" if k.mode == IN_GENERIC else "ragged"
    elif fast:
        m = "dma" if tl + 12 * DMA_TILE <= LDS_LIMIT else "direct"
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
    if (mode == "dma" and tl + 64 * seg > LDS_LIMIT) or (mode == "ragged" and tl + RAGGED_WAVE > LDS_LIMIT):
        mode = "direct" if mode == "dma" else "generic"
        if mode == "direct":
            nb = 8 if k.nb == 8 and (stride // 16) % 8 == 0 else 4
            if (stride // 16) % 4:
                mode = "generic"
    pack = mode == "dma" and seg == 128 and not resumed and stride >= 256 and k.pack != 0 and ((early & 2) or k.pack >= 1)
    if mode == "dma":
        return f"walk_ldsdma_pack<{POL}, {2 if nt else 0}, 1024>" if pack else f"walk_ldsdma<{POL}, {seg}, {2 if nt and seg == 128 else 0}, 1024>"
    if mode == "direct":
        return f"walk_direct_np<{POL}, 4>" if not pre and nb == 4 else f"walk_direct<{POL}, {nb}, 1>"
    if mode == "ragged":
        return f"walk_ragged<{POL}, 768"
    return f"walk_lines32<{POL}, " if packed_plain and not (early & NO_LINES32) else f"walk_generic<{POL}, "


def ran(dfa, want, *tag):
    kn = dfa.last_kernel_name()
    assert want in kn and POL in kn, (tag, "expected", want, "ran", kn)
    return kn


def opened(hip, c, flags, extra=0):
    """HipDfa(flat) or HipDfa(flat, LAYOUT_LDS2): the pair table either way -> (dfa, the table's LDS as the library counts it)"""
    dfa = hip.HipDfa(c.flat, flags | extra)
    assert dfa.info()["layout_name"] == "lds2", (c.name, flags)
    dfa.tune(hip.KNOB_INPUT_MODE, IN_GENERIC)            # no tiles behind the table: lds_bytes is the table's alone
    tl = dfa.info()["lds_bytes"]
    dfa.tune(hip.KNOB_INPUT_MODE, -1)
    assert tl == R.pair_lds_bytes(c.entries), (c.name, tl)
    return dfa, tl


# ---- buffers and calls ------------------------------------------------------------------------------------------------------------

# (to_dev, Buf, Out, call, walk_rows, PACKED_FORMS and Packed: tests/walk_buffers.py)

@functools.lru_cache(maxsize=None)
def strided(stride):
    """the pool's rows cut to `stride` bytes, their lengths clipped to it"""
    rows, lens, _ = R.pool()
    short = np.minimum(lens, stride).astype(np.uint32)
    return Buf(rows[:, :stride], 64), Buf(short), short


# ---- 1. fixed stride, every input mode -----------------------------------------------------------------------------------------------

FIXED = [("small", False), ("small", True), ("odd_c1", False), ("odd_c1", True), ("full", True), ("complete", True)]


@pytest.mark.parametrize("name,forced", FIXED, ids=[f"{a}-{'forced' if f else 'auto'}" for a, f in FIXED])
def test_fixed_stride_every_input_mode(hip, name, forced):
    c = R.case(name)
    dfa, tl = opened(hip, c, hip.LAYOUT_LDS2 if forced else 0)
    early = 3 if c.absorbing(c.tr).any() else 1          # bit 1 (the per-lane load skip) only where an absorbing state is reachable
    seen = {}
    for k in SETTINGS:
        set_knobs(dfa, hip, k)
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
                        kn = ran(dfa, expected(tl, k, stride, fast, is_short, early=early), name, forced, k.label, stride, with_lens, dev, n)
                        seen[(k.label, stride, with_lens)] = kn.split(" (")[0]           # (the whole pool's: the last sub-batch)
    for key, kn in seen.items():
        print(f"{name} {'forced' if forced else 'auto'} {key}: {kn}")
    dfa.close()


# ---- 2. variable-length fronts -----------------------------------------------------------------------------------------------------

VARLEN = [("small", False), ("small", True), ("one_image_max", False), ("one_image_max", True), ("full", True)]


@pytest.mark.parametrize("name,forced", VARLEN, ids=[f"{a}-{'forced' if f else 'auto'}" for a, f in VARLEN])
def test_variable_length_fronts(hip, name, forced):
    c = R.case(name)
    rows = R.pool()[0]
    dfa, tl = opened(hip, c, hip.LAYOUT_LDS2 if forced else 0)
    ragged_fits = tl + 4 * RAGGED_WAVE <= LDS_LIMIT
    batches = [(which, lens, n) for which, lens in R.edge_batches().items() for n in ((65, N) if which == "head" else (N,))]
    seen = {}
    for which, lens, n in batches:
        pk = Packed(rows, lens, n)
        want = c.ends(c.at(lens[:n]))
        lo, hi = pk.mean(True, "u64 offsets"), pk.mean(False, "u64 offsets") + 1         # no front finds the mean below lo, every one below hi
        #          input mode, pick mean, early knob: which kernel
        for label, mode, pm, ek in (("default", -1, -1, -1), ("mean above the threshold", -1, lo, -1), ("mean below the threshold", -1, hi, -1),
                                    ("per-lane by knob", IN_GENERIC, -1, -1), ("per-lane by knob, walk_generic's own body", IN_GENERIC, -1, 3 | NO_LINES32),
                                    ("ragged by knob", IN_RAGGED, -1, -1)):
            dfa.tune(hip.KNOB_INPUT_MODE, mode)
            dfa.tune(hip.KNOB_PICK_MEAN, pm)
            dfa.tune(hip.KNOB_EARLY_RETIRE, ek)
            k = DEFAULT._replace(mode=mode)
            for form in PACKED_FORMS:
                for dev in (False, True):
                    o = Out(n, dev)
                    pk.walk(dfa, dev, form, o)
                    o.check(want, name, forced, which, n, label, form, dev, dfa.last_kernel_name())
                    # the threshold: the knob, else 128 where walk_lines32 is the per-lane kernel the front counts on (the plain
                    # packed fronts; on the device every packed front below 4 GiB), 96 elsewhere (the host's packed_all)
                    thr = pm if pm >= 0 else 128 if (dev or not form.startswith("packed_all")) else 96
                    is_short = mode < 0 and pk.mean(dev, form) < thr
                    kn = ran(dfa, expected(tl, k, 0, False, is_short, early=3 if ek < 0 else ek, packed_plain=True), name, forced, which, n, label, form, dev)
                    if dev and mode < 0 and ragged_fits:
                        assert "on the device" in kn, kn          # the candidates were launched, the batch's mean chose
                    seen[(label, form, dev)] = kn.split(" (")[0]
    dfa.tune(hip.KNOB_EARLY_RETIRE, -1)
    names = set(seen.values())
    assert any("walk_lines32<" in s for s in names), names            # ... where the front can pick it
    assert len({s for s in names if "walk_generic<" in s}) == 3, names      # one instantiation per metadata form
    assert any("walk_ragged<" in s for s in names) == ragged_fits, names
    for key, kn in seen.items():
        print(f"{name} {'forced' if forced else 'auto'} {key}: {kn}")
    dfa.close()


# ---- 3. end-ids ---------------------------------------------------------------------------------------------------------------------

IDS = [("small", False), ("small", True), ("one_image_max", False), ("one_image_max", True), ("full", True)]


@pytest.mark.parametrize("name,forced", IDS, ids=[f"{a}-{'forced' if f else 'auto'}" for a, f in IDS])
def test_end_ids(hip, name, forced):
    c = R.case(name)
    rows_np, lens_np, _ = R.pool()
    dfa, tl = opened(hip, c, hip.LAYOUT_LDS2 if forced else 0)
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
                        kn = ran(dfa, expected(tl, DEFAULT, 0, False, pk.mean(dev, "u64 offsets") < 96), name, batch, mode, dev, n)
                    else:
                        call("fsm_hip_exec_batch_ids", dev, dfa, rows.p(dev), L, lens.p(dev) if batch == "rows + lens" else None, n, mode, o.p("ids"))
                        kn = ran(dfa, expected(tl, DEFAULT, L, batch == "rows", batch != "rows" and int(lens_np[:n].sum()) // n < 96), name, batch, mode, dev, n)
                    tag = (name, forced, batch, mode, dev, n, kn)
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
    dfa.close()


# ---- 4. resumed walks ---------------------------------------------------------------------------------------------------------------

RESUMED = [("small", False), ("small", True), ("one_image_max", False), ("one_image_max", True), ("two_images_min", False), ("full", True)]
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


@pytest.mark.parametrize("name,forced", RESUMED, ids=[f"{a}-{'forced' if f else 'auto'}" for a, f in RESUMED])
def test_resumed_walks(hip, name, forced):
    c = R.case(name)
    rows_np, _, cut = R.pool()
    dfa = hip.HipDfa(c.flat, hip.LAYOUT_LDS2 if forced else 0)
    assert dfa.info()["layout_name"] == "lds2"
    tl = R.pair_lds_bytes(c.entries)
    second_image = not forced and tl > HAND_OVER
    assert second_image == (name == "two_images_min")
    start = np.full(N, hip.STATE_START, np.uint32)
    first_rows, first_lens, rest_rows, rest_lens = Buf(rows_np, 64), Buf(cut), Buf(c.rest, 64), Buf(c.rest_lens)
    car_cut, car_all = G.carried(c.st_cut), G.carried(c.st_all)
    end_cut, end_all = c.ends(c.st_cut), c.ends(c.st_all)
    assert (c.rest_lens == 0).sum() >= 1 and (car_cut == hip.STATE_DEAD).sum() >= 50
    dead = np.full(N, hip.STATE_DEAD, np.uint32)
    seen = {}
    for n in R.SUBS:
        pk1, pk2 = Packed(rows_np, cut, n), Packed(c.rest, c.rest_lens, n)
        for form in ("stride", "offsets") + tuple(META):
            for dev in (False, True):
                tag = (name, forced, form, dev, n)
                o = Out(n, dev, state=start)
                resume(dfa, dev, form, first_rows, first_lens, pk1, n, o)
                o.check(end_cut[:n], *tag, "first piece", carried=car_cut[:n], bitmap=dev)
                kn = dfa.last_kernel_name()
                if second_image:
                    assert POL not in kn and "walk_" in kn, kn             # the resumed walks of a dfa with a second image run there
                else:
                    # (a resumed front holds the mean against 96 bytes; the device finds it where walk_ragged fits)
                    mean = int(cut[:n].sum()) // n if form == "stride" else pk1.mean(dev, form if form != "offsets" else "u64 offsets")
                    ran(dfa, expected(tl, DEFAULT, L if form == "stride" else 0, False, mean < 96, resumed=True), *tag)
                    if name == "full":
                        assert f"walk_generic<{POL}" in kn, kn
                seen[(form, dev)] = kn.split(" (")[0]
                # the second piece from the JUDGE's carried states: it ends where the whole row ends
                o = Out(n, dev, state=car_cut)
                resume(dfa, dev, form, rest_rows, rest_lens, pk2, n, o)
                o.check(end_all[:n], *tag, "second piece", carried=car_all[:n], bitmap=dev)
        # handed DEAD, a piece stays dead whatever it reads; handed the absorbing accept, it stays there
        for dev in (False, True):
            o = Out(n, dev, state=dead)
            resume(dfa, dev, "stride", first_rows, first_lens, pk1, n, o)
            o.check(np.full(n, NO, np.uint32), name, forced, dev, n, "handed DEAD", carried=dead[:n], bitmap=dev)
            o = Out(n, dev, state=dead)
            resume(dfa, dev, "offsets", first_rows, first_lens, pk2, n, o)
            o.check(np.full(n, NO, np.uint32), name, forced, dev, n, "handed DEAD, offsets", carried=dead[:n], bitmap=dev)
            if c.sinks:
                sink = np.full(N, c.S - 1, np.uint32)
                for form, pk in (("stride", pk1), ("u32 offsets", pk2)):
                    o = Out(n, dev, state=sink)
                    resume(dfa, dev, form, first_rows, first_lens, pk, n, o)
                    o.check(sink[:n], name, forced, dev, n, "handed the absorbing accept", form, carried=sink[:n], bitmap=dev)
    for key, kn in seen.items():
        print(f"{name} {'forced' if forced else 'auto'} resumed {key}: {kn}")
    dfa.close()


# ---- 5. absorbing lanes ---------------------------------------------------------------------------------------------------------------

ABSORBING = [("small", False), ("full", True), ("odd_c1", False)]
ABS_SETTINGS = tuple(k for k in SETTINGS if k.label in ("lds-dma 64", "lds-dma 128, nontemporal", "lds-dma 128, temporal", "direct, no prefetch",
                                                         "packing, nontemporal", "packing, temporal"))


@pytest.mark.parametrize("name,forced", ABSORBING, ids=[f"{a}-{'forced' if f else 'auto'}" for a, f in ABSORBING])
def test_absorbing_lanes(hip, name, forced):
    c = R.case(name)
    subs = (129, N)
    for n in subs:                                           # what makes this group bite, for the rows actually launched
        if name == "odd_c1":
            s = c.shares(n)
            assert min(s["dead"], s["accept"], s["band0"], s["odd"], s["second"]) >= 0.10, (n, s)
        else:
            R.bites(c, n)
    seen = {}
    for create, knob in ((hip.NO_EARLY_RETIRE, -1), (0, 1), (0, 3), (0, -1)):
        dfa, tl = opened(hip, c, hip.LAYOUT_LDS2 if forced else 0, create)
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
                            kn = ran(dfa, expected(tl, k, stride, not with_lens, is_short, early=early), name, create, knob, k.label, stride, with_lens, dev, n)
                            seen[(early, k.label, stride, with_lens)] = kn.split(" (")[0]
        dfa.close()
    ks = set(seen.values())
    for part in (f"walk_ldsdma<{POL}, 64,", f"walk_ldsdma<{POL}, 128,", f"walk_direct_np<{POL}", f"walk_ldsdma_pack<{POL}"):
        assert any(part in s for s in ks), (part, ks)
    for key, kn in seen.items():
        print(f"{name} early={key[0]} {key[1:]}: {kn}")


# ---- 6. the hand-over to a second image ----------------------------------------------------------------------------------------------

def test_hand_over_to_the_second_image(hip):
    rows_np, lens_np, _ = R.pool()
    rows, _, _ = strided(L)
    pk = Packed(rows_np, lens_np, N)
    side = {}
    for name in ("one_image_max", "two_images_min", "complete"):
        c = R.case(name)
        dfa, tl = opened(hip, c, 0)
        second = tl > HAND_OVER                              # by the library's own info()["lds_bytes"]
        side[name] = (tl, second)
        want = c.ends(c.st_len)
        for form in PACKED_FORMS:
            for dev in (False, True):
                o = Out(N, dev)
                pk.walk(dfa, dev, form, o)
                o.check(want, name, form, dev)
                kn = dfa.last_kernel_name()
                assert "walk_" in kn and (POL in kn) == (not second), (name, form, dev, tl, kn)
        for dev in (False, True):                            # fixed-stride rows: the pair table on either side
            o = Out(N, dev)
            walk_rows(dfa, dev, rows, L, None, N, o)
            o.check(c.ends(c.st_all), name, "rows", dev)
            ran(dfa, expected(tl, DEFAULT, L, True, early=3 if c.absorbing(c.tr).any() else 1), name, "rows", dev)
        print(f"{name}: the pair table takes {tl} bytes of LDS, hand-over above {HAND_OVER}: {'a second image' if second else 'one image'}")
        dfa.close()
    assert [s for _, s in side.values()] == [False, True, True], side
    assert side["one_image_max"][0] <= HAND_OVER < side["two_images_min"][0]
