"""CPU: the case table of tests/test_gpu_selfloop.py, checked before anything is launched -- how every automaton of
tests/selfloop_ref.py plans on the two self-loop-mask layouts (class counts, the self-loop byte range of every looping state,
the self-loop masks), that the inputs reach every branch of the chunk skip (selfloop_ref.Model: conditions, not
measurements), and that the SWAR range test of CombSelfPol::skip16_raw (walk_kernels.h), transcribed in numpy, answers
"all 16 bytes lie in lo..hi" exactly where the planner hands it a range.  Nothing here needs a GPU."""
import errno

import numpy as np
import pytest

import selfloop_ref as R

NO = R.NO


@pytest.fixture(scope="module")
def hip(built):
    import libfsm_amd
    libfsm_amd.load_library()
    return libfsm_amd


def layouts(hip):
    return {"combself": hip.LAYOUT_COMBSELF, "ldsself": hip.LAYOUT_LDSSELF}


def rng_of(hip, case, state):
    """(lo, hi) of a state's self-loop range in the COMBSELF plan, None for "no range\""""
    p = hip.Plan(case.flat, hip.LAYOUT_COMBSELF)
    new2old = p.get("new2old")[:p.S1 - 1].tolist()
    v = int(p.get("comb_rng")[p.get("comb_off")[new2old.index(state)]])
    return None if v == R.RNG_NONE else (v & 0xff, v >> 8)


# ---- plans ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fillers,classes", [(0, 28), (3, 31), (4, 32)])
@pytest.mark.parametrize("layout", ["combself", "ldsself"])
def test_select_plans_with_the_class_count_it_was_built_for(hip, layout, fillers, classes):
    c = R.select(fillers)
    p = hip.Plan(c.flat, layouts(hip)[layout])
    assert p.layout == layouts(hip)[layout] and p.C == classes and p.S1 == len(c.dense) + 1
    assert R.fillers_for(hip, layouts(hip)[layout], classes) == fillers


@pytest.mark.parametrize("layout", ["combself", "ldsself"])
def test_more_than_32_classes_are_refused(hip, layout):
    with pytest.raises(OSError) as ei:
        hip.Plan(R.select(5).flat, layouts(hip)[layout])
    assert ei.value.errno == errno.ENOTSUP


@pytest.mark.parametrize("fillers", [0, 3, 4])
def test_select_ranges(hip, fillers):
    c = R.select(fillers)
    got = tuple(rng_of(hip, c, 1 + k) for k in range(R.K))
    assert got == ((48, 57), (0, 127), (128, 255), (1, 127), (0, 0), (127, 127), None, None, None, None, None, None, (65, 65), (0, 126), (2, 255))
    assert got == R.WANT_RNG
    assert rng_of(hip, c, 0) is None and rng_of(hip, c, 1 + R.K) is None           # the start state and ACC loop on nothing


def test_variant_plans(hip):
    for name, L in layouts(hip).items():
        # ACC absorbing: every byte is its loop
        c = R.select(0, acc="absorbing")
        assert hip.Plan(c.flat, L).C == 28
        # the start state with a loop byte of its own: one class more; three fillers fewer... by the plan's own count
        c = R.select(0, start_loop=True)
        assert hip.Plan(c.flat, L).C == 29
        assert R.fillers_for(hip, L, 31, start_loop=True) == 2 and R.fillers_for(hip, L, 32, start_loop=True) == 3
        assert hip.Plan(R.select(0, loops_accept=True).flat, L).C == 28
        p = hip.Plan(R.pingpong().flat, L)
        assert p.layout == L and p.C == 3
    assert rng_of(hip, R.select(0, acc="absorbing"), 1 + R.K) == (0, 255)
    assert rng_of(hip, R.select(0, start_loop=True), 0) == (R.START_LOOP_BYTE, R.START_LOOP_BYTE)
    assert tuple(rng_of(hip, R.select(0, loops_accept=True), 1 + k) for k in range(R.K)) == R.WANT_RNG
    assert tuple(rng_of(hip, R.select(3, start_loop=True), 1 + k) for k in range(R.K)) == R.WANT_RNG
    pp = R.pingpong()
    assert rng_of(hip, pp, 0) == (128, 255) and rng_of(hip, pp, 1) == (1, 127) and rng_of(hip, pp, 2) == (0, 255)
    # eager outputs: both layouts take them, with the ranges and the class count unchanged
    e = R.select(0, eager=True)
    for L in layouts(hip).values():
        p = hip.Plan(e.flat, L)
        assert p.layout == L and p.C == 28
    assert tuple(rng_of(hip, e, 1 + k) for k in range(R.K)) == R.WANT_RNG


# ---- masks ---------------------------------------------------------------------------------------------------------------------

ALL_CASES = [("select", dict(fillers=0)), ("select", dict(fillers=3)), ("select", dict(fillers=4)), ("select", dict(fillers=0, acc="absorbing")),
             ("select", dict(fillers=3, start_loop=True)), ("select", dict(fillers=0, loops_accept=True)), ("pingpong", {})]


def make(kind, kw):
    return R.pingpong() if kind == "pingpong" else R.select(**kw)


@pytest.mark.parametrize("kind,kw", ALL_CASES, ids=[make(k, kw).name for k, kw in ALL_CASES])
@pytest.mark.parametrize("layout", ["combself", "ldsself"])
def test_masks_are_the_self_loops_of_the_dense_table(hip, layout, kind, kw):
    c = make(kind, kw)
    rows = R.rows_of(c, 48)[0][:64]
    m = R.Model(hip, c, layouts(hip)[layout], rows)
    p = m.p
    new2old = p.get("new2old")[:p.S1 - 1].astype(np.int64)
    seen_loop = 0
    for n in range(p.S1):
        mask = int(m.smask[n])
        if p.C <= 31:
            assert mask >> 31, (n, hex(mask))                   # the spare class: a loop of every state
        elif n == p.start:
            assert not mask >> 31, (n, hex(mask))               # 32 classes: bit 31 is class 31's, which no start state here loops on
        if n >= p.abs_min:
            assert mask == 0xFFFFFFFF, (n, hex(mask))
            continue
        for cl in range(p.C):
            by = np.nonzero(m.cls == cl)[0]
            loop = c.loops[new2old[n], by]
            assert loop.all() or not loop.any(), (n, cl)       # (a class never splits a state's loop)
            assert bool((mask >> cl) & 1) == bool(loop.all()), (n, cl, hex(mask))
            seen_loop += int(loop.all())
        if p.C < 31:
            assert (mask >> p.C) & ((1 << (31 - p.C)) - 1) == 0, (n, hex(mask))
    assert seen_loop >= 2
    # DEAD is absorbing; an absorbing ACC too
    assert p.abs_min <= p.S1 - 1 and p.nabsorbing == (3 if kind == "pingpong" else 2 if kw.get("acc") == "absorbing" else 1)


# ---- the inputs reach every branch ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fillers", [0, 3, 4])
@pytest.mark.parametrize("L", R.STRIDES)
def test_whole_chunks_reach_every_branch(hip, fillers, L):
    c = R.select(fillers)
    rows, lens, _ = R.rows_of(c, L)
    if L == 48:                                                # the stride's two batches, one behind the other
        rows = np.concatenate([rows, R.rows_of(c, L, part=1)[0]])
        assert len(rows) % 64 == 0
    assert len(R.rows_of(c, L)[0]) <= 20000
    want = c.ends(rows)
    acc = float((want != NO).mean())
    assert 0.25 <= acc <= 0.75, acc
    m = R.Model(hip, c, hip.LAYOUT_COMBSELF, rows)
    ml = R.Model(hip, c, hip.LAYOUT_LDSSELF, rows)
    assert np.array_equal(m.vote, ml.vote)                     # the two layouts' masks say the same
    raw_w, vote_w = m.waves(m.raw), m.waves(m.vote)            # [c][w][64]
    nbad = (~raw_w).sum(-1)
    first_bad = m.waves(m.raw_first_bad)
    for k in range(R.K):
        in_k = np.stack([m.waves(m.state_k(ch)[None, :])[0] == k for ch in range(m.nch)])     # [c][w][64]
        any_k = in_k.any(-1)
        if k in R.ONE_RUN:
            # whole wavefronts pass the raw test with a lane in L_k ...
            assert int((raw_w.all(-1) & any_k).sum()) >= 16, (k, L)
            # ... and fail it by ONE lane, which is in L_k, at every byte position
            lone = (nbad == 1) & ((~raw_w) & in_k).any(-1)
            pos = {int(first_bad[ci, w][~raw_w[ci, w]][0]) for ci, w in zip(*np.nonzero(lone))}
            assert pos == set(range(16)), (k, L, sorted(pos))
        else:
            # no raw pass where a lane is in a state without a range; the class vote passes all the same
            assert int((raw_w.all(-1) & any_k).sum()) == 0, (k, L)
            assert int(raw_w[in_k].sum()) == 0
            assert int((vote_w.all(-1) & any_k).sum()) >= 16, (k, L)
            lone = ((~vote_w).sum(-1) == 1) & ((~vote_w) & in_k).any(-1)
            assert int(lone.sum()) >= 8, (k, L)
    # wavefronts whose lanes are in DIFFERENT looping states when the vote is taken -- and pass it
    kk = np.stack([m.waves(m.state_k(ch)[None, :])[0] for ch in range(m.nch)])
    mixed = np.array([[len(set(kk[ci, w][kk[ci, w] >= 0].tolist())) >= 9 for w in range(kk.shape[1])] for ci in range(m.nch)])
    assert int((mixed & vote_w.all(-1)).sum()) >= 16 and int((mixed & raw_w.all(-1)).sum()) >= 8
    assert int((mixed & ((~vote_w).sum(-1) == 1)).sum()) >= 16
    # every wavefront has chunks all 64 lanes pass (rows of three chunks: every wavefront of the stride's second batch)
    assert vote_w.all(-1).any(0)[vote_w.shape[1] // 2 if L == 48 else 0:].all()


@pytest.mark.parametrize("fillers", [0, 4])
@pytest.mark.parametrize("L", [128, 256])
def test_tails_reach_every_branch(hip, fillers, L):
    c = R.select(fillers)
    rows, lens, _ = R.rows_of(c, L, True)
    assert int(lens.min()) == 0 and int(lens.max()) == L and set(range(L + 1)) <= set(lens.tolist())
    want = c.ends(rows, lens)
    assert 0.25 <= float((want != NO).mean()) <= 0.75
    # every tail at every start alignment of a packed line
    _, off = R.packed_from(rows, lens, 1)
    pairs = set(zip((off[:-1] % 16).tolist(), (lens % 16).tolist()))
    assert {(a, t) for a in range(16) for t in range(1, 16)} <= pairs
    for layout in (hip.LAYOUT_COMBSELF, hip.LAYOUT_LDSSELF):
        m = R.Model(hip, c, layout, rows, lens)
        for lo_positive in (False, True):
            idx, t, st, ch, valid = m.tails(lo_positive)
            looping = m.smask[st] & 0x7FFFFFFF != 0
            vote = m.vote_pass(st, ch)                         # on the FILLED chunk: the predicated path of 32 classes
            ident = m.vote_pass(st, ch, valid)                 # with the spare class
            assert np.array_equal(vote, ident)                 # (the fill byte is one of the row's own: it changes no answer)
            for tail in range(1, 16):
                sel = (t == tail) & looping & (st < m.p.abs_min)
                assert int((sel & vote).sum()) >= 1 and int((sel & ~vote).sum()) >= 1, (fillers, L, lo_positive, tail)
                if m.rng is not None:
                    raw = m.raw_pass(st, ch)[0]
                    assert int((sel & raw).sum()) >= 1 and int((sel & ~raw & vote).sum()) >= 1, (fillers, L, lo_positive, tail)


def test_pingpong_rows_switch_inside_and_between_chunks(hip):
    c = R.pingpong()
    for L in (128, 256):
        rows, _, _ = R.rows_of(c, L)
        want = c.ends(rows)
        assert (want == 2).mean() >= 0.2 and (want == 3).mean() >= 0.2 and (want == NO).mean() >= 0.25
        m = R.Model(hip, c, hip.LAYOUT_COMBSELF, rows)
        a, b = m.old2new[0], m.old2new[1]
        raw_w = m.waves(m.raw)
        st_w = m.waves(m.st[:m.nch])
        # whole wavefronts pass the raw test in A, in B, and with lanes in both
        for want_states in ({a}, {b}, {a, b}):
            hit = [(ci, w) for ci, w in zip(*np.nonzero(raw_w.all(-1))) if set(st_w[ci, w].tolist()) == want_states]
            assert len(hit) >= 8, (L, want_states, len(hit))
        # a row enters the other looping state in one chunk and the NEXT chunk is whole bytes of the state it left: the chunk
        # a range that was not reloaded would skip
        ch = rows.reshape(len(rows), m.nch, 16)
        stale = 0
        for ci in range(1, m.nch - 1):
            moved = (m.st[ci] != m.st[ci + 1]) & np.isin(m.st[ci], (a, b)) & np.isin(m.st[ci + 1], (a, b))
            lo, hi = (m.rng[m.st[ci]] & 0xff)[:, None], (m.rng[m.st[ci]] >> 8)[:, None]
            old_range = ((ch[:, ci + 1] >= lo) & (ch[:, ci + 1] <= hi)).all(-1)
            stale += int((moved & old_range).sum())
        assert stale >= 64, (L, stale)
        # the switch falls on chunk bytes 0 and 15
        sw = np.nonzero((rows[:, 1:] >= 128) != (rows[:, :-1] >= 128))
        assert {0, 15} <= set(((sw[1] + 1) % 16).tolist())


def test_start_loop_rows_meet_the_start_states_byte_as_a_whole_chunk(hip):
    c = R.select(3, start_loop=True)
    rows, _, _ = R.rows_of(c, 256)
    want = c.ends(rows)
    assert 0.25 <= float((want != NO).mean()) <= 0.75
    m = R.Model(hip, c, hip.LAYOUT_COMBSELF, rows)
    # whole wavefronts skip their FIRST chunk in the start state (its own loop byte): first_noskip()'s other side
    assert int(m.waves(m.raw)[0].all(-1).sum()) >= 32
    # rows in a looping state meet a whole chunk of the start state's byte, which is none of theirs
    ch = rows.reshape(len(rows), m.nch, 16)
    hit = sum(int(((ch[:, ci] == R.START_LOOP_BYTE).all(-1) & (m.state_k(ci) >= 0) & ~m.vote[ci]).sum()) for ci in range(m.nch))
    assert hit >= 16, hit


# ---- the SWAR range test -------------------------------------------------------------------------------------------------------

def swar_pass(w, lo, hi):
    """CombSelfPol::skip16_raw for one lane: w u32 [m][4] -> the lane's vote"""
    w = w.astype(np.uint32)
    LO = np.uint32((lo * 0x01010101) & 0xFFFFFFFF)
    AD = np.uint32(((127 - hi) * 0x01010101) & 0xFFFFFFFF)
    MM = np.uint32(0 if hi == 255 else 0x80808080)
    aL = np.bitwise_or.reduce((w - LO) & ~w, axis=1)
    aM = np.bitwise_or.reduce((w + AD) | w, axis=1)
    return ((aL | (aM & MM)) & np.uint32(0x80808080)) == 0


def adversarial_chunks(lo, hi):
    """16-byte chunks around lo and hi: every byte of {0, lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, 0x7F, 0x80, 0xFF} alone among
    copies of lo, of hi and of a middle value, at every byte position; pairs of them next to each other (borrows and carries
    run from byte to byte inside a dword); and seeded random chunks inside and around the range"""
    edge = sorted({b for b in (0, lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, 0x7F, 0x80, 0xFF) if 0 <= b <= 255})
    base = sorted({lo, hi, (lo + hi) // 2} if lo <= hi else {lo})
    out = []
    for f in base:
        for e in edge:
            for pos in (0, 1, 2, 3, 7, 12, 15):
                r = np.full(16, f, np.uint8)
                r[pos] = e
                out.append(r)
                for e2 in edge:
                    r2 = r.copy()
                    r2[(pos + 1) % 16] = e2
                    out.append(r2)
    rs = np.random.RandomState(lo * 256 + hi)
    if lo <= hi:
        out += list(rs.randint(lo, hi + 1, (16, 16)).astype(np.uint8))
    out += list(rs.randint(max(lo - 2, 0), min(hi + 2, 255) + 1, (16, 16)).astype(np.uint8)) if lo <= hi else []
    return np.array(out, np.uint8)


def test_swar_range_test_is_exact_where_the_planner_uses_it():
    pairs = [(lo, hi) for lo in range(129) for hi in list(range(128)) + [255] if lo <= hi]
    assert len(pairs) == 8385
    pairs.append((0x80, 0x00))                                 # "no range": nothing passes
    bad = []
    for lo, hi in pairs:
        ch = adversarial_chunks(lo, hi)
        want = ((ch >= lo) & (ch <= hi)).all(1)
        got = swar_pass(ch.view("<u4").reshape(-1, 4), lo, hi)
        if not np.array_equal(got, want):
            bad.append((lo, hi, int((got != want).sum())))
    assert not bad, bad[:10]


def test_swar_range_test_never_passes_a_byte_above_127_unless_hi_is_255():
    """why the planner's refusal of 127 < hi < 255 costs speed, not answers: with such a range the test fails on every byte
    >= 0x80, in the range or not -- it can lose a skip, it cannot skip a byte outside the range"""
    for lo, hi in ((100, 200), (128, 128), (0, 128), (0x80, 0xFE), (0, 254), (64, 129)):
        ch = adversarial_chunks(lo, hi)
        want = ((ch >= lo) & (ch <= hi)).all(1)
        got = swar_pass(ch.view("<u4").reshape(-1, 4), lo, hi)
        assert not (got & ~want).any(), (lo, hi)
        assert not got[(ch >= 0x80).any(1)].any(), (lo, hi)
