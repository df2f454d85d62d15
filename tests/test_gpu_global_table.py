"""GPU (-m gpu): the global-table walks (Glob16Pol: 2-byte entries up to 65 535 states; GlobPol: 4-byte entries beyond)
OFF the head of the table that every workgroup keeps in LDS, and at the switch between the two entry widths.

The automata are tests/global_ref.py's affine family: every byte class permutes the states, so uniformly random bytes
spread the walk over the whole table and most steps take the path behind the wave vote (a global load) -- which the
goldens reach only by accident, the planner ordering their rows so that they do not.  Before any launch the shape of
every automaton is asserted on the CPU (which table the planner emits, whether its rows are re-ordered, what share of the
steps lies beyond what LDS can hold); after the first launch, that the kernel that ran is the policy's.

The judge of every answer is global_ref.walk / walk_eager / endid_slots: the automaton's closed formula applied byte by
byte in numpy.  Nothing is compared with another layout, kernel or knob setting of the library."""
import functools

import numpy as np
import pytest

import global_ref as G

pytestmark = pytest.mark.gpu

NO = 0xFFFFFFFF
N, L = 4099, 256                        # odd, no multiple of 64 or 128, several tiles at two inputs per lane
SUBS = (1, 2, 63, 65, 129, N)
LDS_CAN_HOLD = 163840                   # bytes: an upper bound of the head (all of a workgroup's LDS on this device)
NAMES = tuple(G.FAMILY)
COLD_BAND = ("last16", "first32", "dying", "eager40", "eager100")


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()
    return libfsm_amd


def bits(bm, n):
    return np.unpackbits(bm.view(np.uint8), bitorder="little")[:n].astype(bool)


@functools.lru_cache(maxsize=None)
def inputs():
    """the rows every test walks, their lengths for the variable-length fronts and the byte at which a resumed walk is cut"""
    rows = np.random.RandomState(4099).randint(0, 256, (N, L)).astype(np.uint8)
    rng = np.random.RandomState(7)
    lens = G.varlens(N, L, rng)
    cut = rng.randint(0, L + 1, N).astype(np.uint32)
    cut[:4] = (0, L, 1, L - 1)
    rows.setflags(write=False)
    lens.setflags(write=False)
    cut.setflags(write=False)
    return rows, lens, cut


class Case:
    """one automaton and the reference's answers on inputs(), computed once and left as they are"""

    def __init__(self, name):
        self.name = name
        self.flat, self.dense, self.cls = G.family(name)
        self.kw = G.FAMILY[name][2]
        rows, lens, cut = inputs()
        ar = np.arange(N)
        self.tr = G.trace(self.dense, self.cls, 0, rows)                   # [N][L + 1]: the state before every byte
        self.tr.setflags(write=False)
        self.st_all = G.walk(self.dense, self.cls, 0, rows)
        self.st_len = G.walk(self.dense, self.cls, 0, rows, lens)
        self.st_cut = G.walk(self.dense, self.cls, 0, rows, cut)
        # the second piece of a resumed walk: the rest of every row moved to its front
        self.rest = np.zeros((N, L), np.uint8)
        for i in range(N):
            self.rest[i, :L - cut[i]] = rows[i, cut[i]:]
        assert np.array_equal(G.walk(self.dense, self.cls, 0, self.rest, L - cut.astype(np.int64), state_in=self.st_cut), self.st_all)
        assert np.array_equal(self.st_len, self.tr[ar, lens]) and np.array_equal(self.st_all, self.tr[:, -1])
        self.end_all, self.end_len, self.end_cut = G.ends(self.flat, self.st_all), G.ends(self.flat, self.st_len), G.ends(self.flat, self.st_cut)
        self.packed, self.off = G.packed(rows, lens)

    def plan(self, hip, flags):
        return hip.Plan(self.flat, flags)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def layouts(hip, c):
    """LAYOUT_GLOBAL, and no flag at all where the planner then chooses the global layout by itself"""
    out = [hip.LAYOUT_GLOBAL]
    if hip.Plan(c.flat, 0).layout == hip.LAYOUT_GLOBAL:
        out.append(0)
    return out


def row_bytes_of(p):
    return p.C * (2 if len(p.get("glob_tab16")) else 4)


def rows_visited(p, flat, states):
    """the table row of every state of a trace: through the renumbering and, where rows are re-ordered, the rank"""
    new2old = p.get("new2old").astype(np.int64)
    new2old[p.S1 - 1] = flat.nstates
    old2new = np.empty(p.S1, np.int64)
    old2new[new2old] = np.arange(p.S1)
    r = old2new[np.where(states < 0, flat.nstates, states)]
    rank = p.get("glob16_rank").astype(np.int64)
    return rank[r] if len(rank) else r


def policy_ran(dfa, p):
    """the kernel of the last launch is the one of the table's entry width"""
    kn = dfa.last_kernel_name()
    assert ("Glob16Pol" in kn) == (p.S1 <= 65535) and ("GlobPol" in kn) == (p.S1 > 65535), kn
    return kn


def hot_values(dfa, p, hip):
    """FSM_HIP_KNOB_HOT_BYTES settings (None: untouched), after asserting how the library rounds and clamps them: by the LDS a
    launch would take (info()'s lds_bytes: byte -> class map + the head, 16-byte granules, behind a per-lane kernel)"""
    rb = row_bytes_of(p)
    table = p.S1 * rb
    r16 = lambda x: (x + 15) // 16 * 16
    dfa.tune(hip.KNOB_INPUT_MODE, hip.IN_GENERIC)       # no tiles behind the table: lds_bytes is the table's alone

    def lds(v):
        dfa.tune(hip.KNOB_HOT_BYTES, v)
        return dfa.info()["lds_bytes"]

    one, three = lds(rb), lds(3 * rb)
    btab = one - r16(rb)                                                    # the byte -> class map in front of the head
    assert 0 < btab <= 4096 and three - one == r16(3 * rb) - r16(rb)
    assert lds(3 * rb + 1) == three and lds(4 * rb - 1) == three           # whole rows only
    assert lds(0) == one and lds(1) == one                                  # one row at least
    big = lds(table + 1000)
    assert big == lds(1 << 30) == lds(table) and big <= LDS_CAN_HOLD        # clamped: to the table, and to what LDS holds
    held = big - btab
    print(f"hot bytes: one row {rb}, table {table}, head at the clamp {held} (+ {btab} in front of it)")
    if table + btab + 8 * 4096 <= LDS_CAN_HOLD:
        assert held == r16(table)
    else:       # (the library keeps room for at most eight 4 KiB tiles beside the head)
        assert LDS_CAN_HOLD - btab - 8 * 4096 - rb - 16 < held <= min(r16(table), LDS_CAN_HOLD - btab)
    dfa.tune(hip.KNOB_INPUT_MODE, -1)
    return rb, (rb, 3 * rb + 1, table + 1000, 0)


def set_mode(dfa, hip, mode, nb, seg, pre):
    dfa.tune(hip.KNOB_INPUT_MODE, mode)
    dfa.tune(hip.KNOB_NB, nb)
    dfa.tune(hip.KNOB_SEG, seg)
    dfa.tune(hip.KNOB_PREFETCH, pre)


def plain_settings(hip):
    return (("front's own", -1, 0, 0, -1), ("direct 4", hip.IN_DIRECT, 4, 0, 1), ("direct 8", hip.IN_DIRECT, 8, 0, 1),
            ("direct 4, no prefetch", hip.IN_DIRECT, 4, 0, 0), ("lds-dma 64", hip.IN_LDSDMA, 0, 64, -1), ("lds-dma 128", hip.IN_LDSDMA, 0, 128, -1),
            ("generic", hip.IN_GENERIC, 0, 0, -1), ("ragged", hip.IN_RAGGED, 0, 0, -1))


# ---- the shape of the automata and of the inputs: CPU only, before any launch -------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_shape_of_automaton_and_inputs(hip, name):
    c = case(name)
    S, K, kw = G.FAMILY[name]
    for flags in layouts(hip, c):
        p = c.plan(hip, flags)
        assert p.layout == hip.LAYOUT_GLOBAL and p.S1 == S + 1 and p.C == K
        t16, rank = p.get("glob_tab16"), p.get("glob16_rank")
        assert (len(t16) != 0) == (p.S1 <= 65535)
        assert (len(rank) == 0) == (name in ("first32", "bytewise_plain", "eager40", "eager100")), name
        rb = row_bytes_of(p)
        assert rb == {"last16": 8, "first32": 16, "odd_rows": 58, "all_hot": 8, "bytewise_reordered": 512, "bytewise_plain": 512,
                      "dying": 8, "eager40": 8, "eager100": 8}[name]
        r = rows_visited(p, c.flat, c.tr[:, :-1])                    # the row every step looks up
        share = float((r >= LDS_CAN_HOLD // rb).mean())
        print(f"{name} flags={flags}: rows={p.S1} row_bytes={rb} table={p.S1 * rb} B, share of steps beyond what LDS can hold = {share:.4f}")
        if name in COLD_BAND:
            assert 0.3 <= share <= 0.9, (name, share)          # any pairing of rows into lanes meets all four hot / cold cases of next2
        if name in ("odd_rows", "bytewise_reordered", "bytewise_plain"):
            assert share > 0, name
        if name == "all_hot":
            assert p.S1 * rb < 32768 and share == 0        # all of it in LDS by default; all but one row cold at a head of one row
            assert float((r >= 1).mean()) > 0.99
        if name == "odd_rows":
            assert p.S1 * rb > LDS_CAN_HOLD and rb % 16 != 0 and (3 * rb) % 16 != 0      # no head of whole rows ends on a 16-byte granule
    if name == "dying":
        dead = c.st_all < 0
        sink = c.st_all >= S - kw["sinks"]
        print(f"dying: {dead.mean():.4f} of the rows end in DEAD, {sink.mean():.4f} in an absorbing accept")
        assert dead.sum() > 0 and sink.sum() > 0
        assert 0.25 <= float((dead | sink).mean()) <= 0.75
        assert (c.end_all[sink] != NO).all() and (c.end_all[dead] == NO).all()
        dl = (c.st_len < 0) | (c.st_len >= S - kw["sinks"])
        assert 0.1 <= float(dl.mean()) <= 0.75
    else:
        assert (c.st_all >= 0).all()
    # accepts and rejects both occur, at every length
    assert 0.05 < float((c.end_all != NO).mean()) < 0.5 and (c.end_len != NO).sum() > 100


# ---- plain walk, fixed stride ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in NAMES if not n.startswith("eager")])
def test_plain_walk_off_the_lds_head(hip, name):
    c = case(name)
    rows_all, _, _ = inputs()
    want_all = c.end_all
    first = True
    for flags in layouts(hip, c):
        p = c.plan(hip, flags)
        for early in ((0, hip.NO_EARLY_RETIRE) if name == "dying" else (0,)):
            dfa = hip.HipDfa(c.flat, flags | early)
            assert dfa.info()["layout"] == hip.LAYOUT_GLOBAL
            end, bm = dfa.exec_batch(rows_all)                       # (before any knob is touched)
            kn = policy_ran(dfa, p)
            assert np.array_equal(end, want_all) and np.array_equal(bits(bm, N), want_all != NO), (name, flags, early, kn)
            rb, hots = hot_values(dfa, p, hip)
            dfa.close()
            dfa = hip.HipDfa(c.flat, flags | early)                  # a fresh one: its head is the default's, untouched
            # (dying under NO_EARLY_RETIRE: the kernels that have the load skip and the default, as for the flag's absence)
            settings = plain_settings(hip)
            if early:
                settings = tuple(s for s in settings if s[0] in ("front's own", "lds-dma 64", "lds-dma 128", "direct 4, no prefetch"))
            for hot in (None,) + hots + (1 << 30,):                  # ... and back to a large value: the same answers again
                if hot is not None:
                    dfa.tune(hip.KNOB_HOT_BYTES, hot)
                for label, mode, nb, seg, pre in settings:
                    set_mode(dfa, hip, mode, nb, seg, pre)
                    for n in SUBS:
                        end, bm = dfa.exec_batch(np.ascontiguousarray(rows_all[:n]))
                        bad = np.nonzero(end != want_all[:n])[0]
                        assert len(bad) == 0, (name, flags, early, hot, label, n, bad[:8], end[bad[:8]], want_all[bad[:8]], dfa.last_kernel_name())
                        assert np.array_equal(bits(bm, n), want_all[:n] != NO), (name, flags, early, hot, label, n)
                    kn = policy_ran(dfa, p)
                    if mode == hip.IN_DIRECT:
                        assert "walk_direct" in kn, kn
                    if mode == hip.IN_GENERIC:
                        assert "walk_generic" in kn, kn
                    if first and hot in (None, rb):
                        print(f"{name} hot={hot} {label}: {kn}")
            first = False
            dfa.close()


# ---- variable-length fronts --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in NAMES if not n.startswith("eager")])
def test_variable_length_fronts_off_the_lds_head(hip, name):
    c = case(name)
    rows_all, lens_all, _ = inputs()
    for flags in layouts(hip, c):
        p = c.plan(hip, flags)
        dfa = hip.HipDfa(c.flat, flags)
        for hot in (None, row_bytes_of(p)):
            if hot is not None:
                dfa.tune(hip.KNOB_HOT_BYTES, hot)
            for mode in (-1, hip.IN_GENERIC, hip.IN_RAGGED):
                dfa.tune(hip.KNOB_INPUT_MODE, mode)
                for n in SUBS:
                    want = c.end_len[:n]
                    rows, lens, off = np.ascontiguousarray(rows_all[:n]), lens_all[:n], c.off[:n + 1]
                    base = c.packed[:int(off[n])]
                    got = {"rows + lens": dfa.exec_batch(rows, lens)}
                    policy_ran(dfa, p)
                    got["u64 offsets"] = dfa.exec_batch_offsets(base, off)
                    policy_ran(dfa, p)
                    got["u32 offsets"] = dfa.exec_batch_offsets32(base, off.astype(np.uint32))
                    got["lengths"] = dfa.exec_batch_lengths(base, lens)
                    policy_ran(dfa, p)
                    for form, (end, bm) in got.items():
                        bad = np.nonzero(end != want)[0]
                        assert len(bad) == 0, (name, flags, hot, mode, n, form, bad[:8], lens[bad[:8]], end[bad[:8]], want[bad[:8]])
                        assert np.array_equal(bits(bm, n), want != NO), (name, flags, hot, mode, n, form)
        dfa.close()


# ---- end-ids -----------------------------------------------------------------------------------------------------------

def test_end_ids_off_the_lds_head(hip):
    c = case("dying")
    rows_all, lens_all, _ = inputs()
    slots = G.endid_slots(c.flat.nstates, c.flat.is_end.astype(bool))
    ids_of = lambda s: slots[s][slots[s] >= 0].astype(np.uint32)
    assert {len(ids_of(int(s))) for s in c.end_all[c.end_all != NO]} == {1, 2, 3} and int(slots.max()) >= 256
    for flags in layouts(hip, c):
        p = c.plan(hip, flags)
        dfa = hip.HipDfa(c.flat, flags)
        sets = dfa.ret_sets()
        assert len(sets) < 64                       # few distinct sets: many states share one
        for hot in (None, row_bytes_of(p)):
            if hot is not None:
                dfa.tune(hip.KNOB_HOT_BYTES, hot)
            for n in SUBS:
                rows = np.ascontiguousarray(rows_all[:n])
                off = c.off[:n + 1]
                base = c.packed[:int(off[n])]
                for form, want, run in (("rows", c.end_all[:n], lambda m: dfa.exec_batch_ids(rows, m)),
                                        ("rows + lens", c.end_len[:n], lambda m: dfa.exec_batch_ids(rows, m, lens_all[:n])),
                                        ("offsets", c.end_len[:n], lambda m: dfa.exec_offsets_ids(base, off, m))):
                    e1, e2 = run(1), run(2)
                    policy_ran(dfa, p)
                    assert np.array_equal(e1 == NO, want == NO) and np.array_equal(e2 == NO, want == NO), (flags, hot, n, form)
                    hit = want != NO
                    lowest = slots[want[hit].astype(np.int64), 0]
                    assert np.array_equal(e1[hit], lowest.astype(np.uint32)), (flags, hot, n, form)
                    for s, k2 in set(zip(want[hit].tolist(), e2[hit].tolist())):
                        assert k2 < len(sets) and np.array_equal(sets[k2], ids_of(s)), (flags, hot, n, form, s, k2)
        dfa.close()


# ---- resumed walks -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["last16", "first32", "dying"])
def test_resumed_walk_off_the_lds_head(hip, name):
    c = case(name)
    rows_all, _, cut_all = inputs()
    START = hip.STATE_START
    assert G.LIB_DEAD == hip.STATE_DEAD and G.LIB_START == START
    for flags in layouts(hip, c):
        p = c.plan(hip, flags)
        dfa = hip.HipDfa(c.flat, flags)
        for hot in (None, row_bytes_of(p)):
            if hot is not None:
                dfa.tune(hip.KNOB_HOT_BYTES, hot)
            for n in SUBS:
                rows, cut = np.ascontiguousarray(rows_all[:n]), cut_all[:n]
                st, end = dfa.exec_batch_resume(rows, np.full(n, START, np.uint32), cut)
                policy_ran(dfa, p)
                # the carried states: the walk to the cut in the caller's numbering, DEAD the library's code
                bad = np.nonzero(st != G.carried(c.st_cut[:n]))[0]
                assert len(bad) == 0, (name, flags, hot, n, bad[:8], cut[bad[:8]], st[bad[:8]], c.st_cut[bad[:8]])
                assert np.array_equal(end, c.end_cut[:n]), (name, flags, hot, n)
                st2, end2 = dfa.exec_batch_resume(np.ascontiguousarray(c.rest[:n]), st, (L - cut.astype(np.int64)).astype(np.uint32))
                bad = np.nonzero(end2 != c.end_all[:n])[0]
                assert len(bad) == 0, (name, flags, hot, n, bad[:8], cut[bad[:8]], end2[bad[:8]], c.end_all[bad[:8]])
                assert np.array_equal(st2, G.carried(c.st_all[:n])), (name, flags, hot, n)
        dfa.close()


# ---- eager outputs -----------------------------------------------------------------------------------------------------

def same_sets(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("name", ["eager40", "eager100"])
def test_eager_walk_off_the_lds_head(hip, name):
    c = case(name)
    E = c.kw["eager"]
    rows_all, lens_all, cut_all = inputs()
    st_all, em_all = G.walk_eager(c.dense, c.cls, 0, rows_all, E)
    st_len, em_len = G.walk_eager(c.dense, c.cls, 0, rows_all, E, lens_all)
    st_cut, em_cut = G.walk_eager(c.dense, c.cls, 0, rows_all, E, cut_all)
    _, em_rest = G.walk_eager(c.dense, c.cls, 0, c.rest, E, L - cut_all.astype(np.int64), state_in=st_cut)
    assert np.array_equal(st_all, c.st_all) and np.array_equal(st_len, c.st_len) and np.array_equal(em_cut | em_rest, em_all)
    sets_all, sets_len, sets_cut = G.eager_sets(em_all), G.eager_sets(em_len), G.eager_sets(em_cut)
    # what the sets are for: most rows emit several ids, every id occurs, short rows emit the start state's alone
    assert em_all.any(axis=0).all() and float((em_all.sum(axis=1) >= 3).mean()) > 0.9 and em_len[0].sum() == 1
    for flags in layouts(hip, c):
        p = c.plan(hip, flags)
        dfa = hip.HipDfa(c.flat, flags)
        assert dfa.eager_id_count() == E and dfa.eager_words() == (E + 63) // 64
        for hot in (None, row_bytes_of(p)):
            if hot is not None:
                dfa.tune(hip.KNOB_HOT_BYTES, hot)
            for mode in (-1, hip.IN_GENERIC, hip.IN_LDSDMA):
                dfa.tune(hip.KNOB_INPUT_MODE, mode)
                dfa.tune(hip.KNOB_SEG, 128 if mode == hip.IN_LDSDMA else 0)
                for n in SUBS:
                    rows, lens, cut, off = np.ascontiguousarray(rows_all[:n]), lens_all[:n], cut_all[:n], c.off[:n + 1]
                    tag = (name, flags, hot, mode, n)
                    end, sets = dfa.exec_batch_eager(rows)
                    policy_ran(dfa, p)
                    assert np.array_equal(end, c.end_all[:n]) and same_sets(sets, sets_all[:n]), tag
                    end, sets = dfa.exec_batch_eager(rows, lens)
                    assert np.array_equal(end, c.end_len[:n]) and same_sets(sets, sets_len[:n]), tag
                    end, sets = dfa.exec_offsets_eager(c.packed[:int(off[n])], off)
                    policy_ran(dfa, p)
                    assert np.array_equal(end, c.end_len[:n]) and same_sets(sets, sets_len[:n]), tag
                    # in two pieces
                    st, end, eo = dfa.exec_batch_eager_resume(rows, np.full(n, hip.STATE_START, np.uint32), np.zeros(n * dfa.eager_words(), np.uint64), lens=cut)
                    policy_ran(dfa, p)
                    assert np.array_equal(st, G.carried(c.st_cut[:n])) and np.array_equal(end, c.end_cut[:n]), tag
                    assert same_sets(dfa.decode_eager(eo), sets_cut[:n]), tag
                    st, end, eo = dfa.exec_batch_eager_resume(np.ascontiguousarray(c.rest[:n]), st, eo, lens=(L - cut.astype(np.int64)).astype(np.uint32))
                    assert np.array_equal(st, G.carried(c.st_all[:n])) and np.array_equal(end, c.end_all[:n]), tag
                    assert same_sets(dfa.decode_eager(eo), sets_all[:n]), tag
        dfa.close()
