"""CPU: the case table of tests/test_gpu_column_table.py, checked before anything is launched -- that every member of
column_table_ref.FAMILY but `sixteen` plans as a column table (FSM_HIP_LAYOUT_TINY) under AUTO, on which side of the boundary
between the 5-bit and the 64-bit image it lies, that one state more is refused, and that the judge's answers on the shared
pool are what the pool was made for: rows die, are accepted and stay live throughout a row, every state (DEAD and the sink
included) is where some row stands at every point a test stops a walk, and half the bytes are >= 0x80 -- no GPU test can pass
on trivial rows.  Nothing here needs a GPU: hip.Plan is the host-side planner, the rest is numpy."""
import errno

import numpy as np
import pytest

import global_ref as G
import column_table_ref as R

NO = R.NO
MEMBERS = [n for n in R.FAMILY if n != "sixteen"]


@pytest.fixture(scope="module")
def hip(built):
    import libfsm_amd
    libfsm_amd.load_library()
    return libfsm_amd


def test_pool():
    rows, lens, cut = R.pool()
    assert rows.shape == (R.N, R.L) and R.N % 2 == 1 and R.N % 64 not in (0, 63) and R.N > 1400
    assert lens[:9].tolist() == [0, 1, 15, 16, 17, 2, 31, 32, 33]
    assert {0, 1, 2, 15, 16, 17, R.L - 1, R.L} <= set(cut.tolist())
    assert int(lens.max()) == R.L
    assert R.SUBS == (1, 2, 63, 64, 65, 129, R.N) and R.OFF0 % 2 == 1
    # the bytes: at least 40 % at or above 0x80, and every byte value occurs
    high = float((rows >= 0x80).mean())
    print(f"bytes >= 0x80: {high:.4f}; distinct byte values: {len(np.unique(rows))}")
    assert high >= 0.40 and len(np.unique(rows)) == 256
    for name, b in R.edge_batches().items():
        assert set(R.EDGE_LENS) <= set(b.tolist()), name
        if name != "head":
            assert int(b[-1]) in (0, 1, 33), name
    assert R.edge_batches()["tail_short"][-16:].tolist() == [1, 2, 3, 1, 2] + [1] * 11


def test_the_formula():
    """column(): the hole, the door, the sinks, the end states, and a permutation of the live states on every other class"""
    for name, (S, K, sinks, endids, hole) in R.FAMILY.items():
        flat, dense, cls = R.column(S, K, sinks, endids=endids, hole=hole)
        live = S - sinks
        assert dense.shape == (S, K) and flat.nstates == S and len(np.unique(cls)) == K
        assert (dense[0, K - 1] == -1) == hole and int((dense < 0).sum()) == int(hole)
        for c in range(K):
            col = dense[:live, c]
            into = col[(col >= 0) & (col < live)]
            assert len(set(into.tolist())) == len(into), (name, c)       # injective on the live states: no class merges two
        if sinks:
            assert dense[live - 1, K - 2] == S - 1 and int((dense[:live] >= live).sum()) == 1      # the door, and no other way in
            assert (dense[live:] == np.arange(live, S)[:, None]).all()
        end = flat.is_end.astype(bool)
        assert end[0] and np.array_equal(end[:live], np.arange(live) % 3 == 0) and end[live:].all()
        assert (flat.endid_off[-1] > 0) == endids
    assert {n: R.FAMILY[n][0] + 1 for n in R.FAMILY} == dict(one=2, two=3, five=6, six=7, fifteen=16, complete15=16, sixteen=17)


@pytest.mark.parametrize("name", MEMBERS)
def test_member_plans_as_a_column_table(hip, name):
    S, K = R.FAMILY[name][:2]
    c = R.case(name)
    p = hip.Plan(c.flat, 0)
    assert p.layout == hip.LAYOUT_TINY, (name, p.layout)
    assert p.S1 == S + 1 and 2 <= p.C <= K       # (with so few states several of the K ranges have the same column: the planner merges them)
    col, col5 = p.get("tiny_col"), p.get("tiny5_col")
    assert len(col) == 256
    # the boundary between the two images: five states + DEAD keep the 5-bit form, six + DEAD only the 64-bit one
    assert len(col5) == (256 if name in ("one", "two", "five") else 0), (name, len(col5))
    assert (len(col5) == 256) == (S + 1 <= 6)
    forced = hip.Plan(c.flat, hip.LAYOUT_TINY)
    assert forced.layout == hip.LAYOUT_TINY and np.array_equal(forced.get("tiny_col"), col) and np.array_equal(forced.get("tiny5_col"), col5)
    assert p.nabsorbing == c.sinks + 1 and p.abs_min == S + 1 - p.nabsorbing       # the sinks and DEAD, numbered last
    # every nibble (5-bit field) from abs_min on is its own index in EVERY column: an absorbing lane stays where it is
    # whatever it reads; the fields beyond S1 are identities too
    for s in range(p.abs_min, 16):
        assert (((col >> np.uint64(4 * s)) & np.uint64(15)) == s).all(), (name, s)
    for s in range(p.abs_min, 6 if len(col5) else 0):
        assert (((col5 >> np.uint32(5 * s)) & np.uint32(31)) == 5 * s).all(), (name, s)
    if name in ("fifteen", "complete15"):
        assert p.S1 == 16 and p.abs_min + p.nabsorbing == 16                          # DEAD is nibble 15


def test_one_state_too_many_is_refused(hip):
    S, K, sinks, endids, hole = R.FAMILY["sixteen"]
    flat = R.traced("sixteen")[0]
    assert S + 1 == 17 and flat.nstates == 16
    with pytest.raises(OSError) as ei:
        hip.Plan(flat, hip.LAYOUT_TINY)
    assert ei.value.errno == errno.ENOTSUP
    assert hip.Plan(flat, 0).layout != hip.LAYOUT_TINY


@pytest.mark.parametrize("name", R.COVERED)
def test_pool_dies_is_accepted_and_lives_throughout_a_row(name):
    c = R.case(name)
    s = R.bites(c)                       # dead, accept, live >= 0.15 each; the three bands >= 0.08 each
    print(name, {k: round(v, 3) if isinstance(v, float) else v for k, v in s.items()})
    s = R.bites(c, 129, bands=0.05)      # ... and on the first 129 rows
    print(name, "first 129:", {k: round(v, 3) if isinstance(v, float) else v for k, v in s.items()})


def test_one_and_two():
    s = R.case("one").shares()
    print("one", s)
    assert s["dead"] >= 0.25 and s["live"] >= 0.25 and s["accept"] == 0, s
    s = R.case("two").shares()
    print("two", s)
    assert min(s["dead"], s["accept"], s["live"]) >= 0.10, s


def test_complete15_has_nothing_absorbing():
    c = R.case("complete15")
    s = c.shares()
    print("complete15", s)
    assert not c.absorbing(c.tr).any() and s["distinct"] == 15 and s["live"] == 1.0, s


@pytest.mark.parametrize("name", R.COVERED)
def test_every_state_is_where_some_row_stands(name):
    """after L bytes, after lens[i] bytes and after cut[i] bytes: every state of the automaton, the sink and DEAD"""
    c = R.case(name)
    rows, lens, cut = R.pool()
    for what, at in (("L", np.full(R.N, R.L)), ("lens", lens), ("cut", cut)):
        assert R.missing(name, at) == [], (name, what, R.missing(name, at))
        st, cnt = np.unique(c.at(at), return_counts=True)
        print(name, what, dict(zip(st.tolist(), cnt.tolist())))
        assert st.tolist() == list(range(-1, c.S))
    moved = int((lens != R.drawn()[1]).sum())
    print(name, f"lengths moved from the drawn ones: {moved}")


@pytest.mark.parametrize("name", R.COVERED)
def test_accepted_rows_carry_several_id_sets(name):
    c = R.case(name)
    end = c.ends(c.st_len)
    hit = end != NO
    sets = {tuple(c.ids_of(int(s)).tolist()) for s in end[hit]}
    print(name, f"accepted under lens: {hit.mean():.3f} ({int(hit.sum())} rows), distinct id sets: {len(sets)}")
    assert all(len(s) >= 1 for s in sets) and int(hit.sum()) >= 100 and int((~hit).sum()) >= 100, (name, sets)
    if name == "fifteen":                # (endid_slots() changes its set every seven states: the smaller automata have one set)
        assert len(sets) >= 2, sets


@pytest.mark.parametrize("name", MEMBERS)
def test_judge_agrees_with_itself(name):
    """(Case.__init__ asserts it: walk() against the trace's columns, and the second piece walked from the first piece's state
    ends where the whole row ends) -- here once more for a cut vector of its own, for the clipped lengths of a short stride,
    and from every state handed in: DEAD stays dead and the sink stays the sink, whatever is read"""
    c = R.case(name)
    rows, lens, cut = R.pool()
    for s in R.STRIDES:
        short = np.minimum(lens, s)
        assert np.array_equal(G.walk(c.dense, c.cls, 0, rows[:, :s], short), c.at(short)), (name, s)
        assert np.array_equal(G.walk(c.dense, c.cls, 0, rows[:, :s]), c.tr[:, s]), (name, s)
    half = np.full(R.N, R.L // 2, np.int64)
    mid = c.at(half)
    assert np.array_equal(G.walk(c.dense, c.cls, 0, rows[:, R.L // 2:], state_in=mid), c.st_all), name
    dead = np.full(R.N, -1, np.int64)
    assert (G.walk(c.dense, c.cls, 0, rows, state_in=dead) == -1).all()
    if c.sinks:
        sink = np.full(R.N, c.S - 1, np.int64)
        assert (G.walk(c.dense, c.cls, 0, rows, state_in=sink) == c.S - 1).all()
