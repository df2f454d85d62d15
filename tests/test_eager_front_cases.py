"""CPU: the case table of tests/test_gpu_eager_front.py, checked before anything is launched -- which layout every
(automaton, layout flag) pair gets from the planner, its set width and the three thresholds the eager walks test a state
against (eager_lo_end, eager_hi_begin, abs_min), and that the reference's answers on the shared inputs are what the inputs
were made for.  Nothing here needs a GPU: hip.Plan is the host-side planner, the rest is numpy."""
import errno

import numpy as np
import pytest

import eager_front_ref as R
import global_ref as G


@pytest.fixture(scope="module")
def hip(built):
    import libfsm_amd
    libfsm_amd.load_library()
    return libfsm_amd


@pytest.mark.parametrize("name", list(R.AUTOMATA))
def test_layouts_and_thresholds(hip, name):
    c = R.case(name)
    from libfsm_amd.capi import ALL_LAYOUTS, LAYOUT_NAMES
    for flag in (0,) + tuple(ALL_LAYOUTS):
        lay = LAYOUT_NAMES.get(flag)
        if flag and lay not in R.TAKES[name]:
            with pytest.raises(OSError) as ei:
                hip.Plan(c.flat, flag)
            assert ei.value.errno == errno.ENOTSUP, (name, lay)
            continue
        p = hip.Plan(c.flat, flag)
        assert LAYOUT_NAMES[p.layout] == (lay or R.AUTO[name]), (name, lay)
        assert (p.S1, p.C) == (c.S + 1, c.K)
        ids = p.get("eager_ids")
        assert np.array_equal(ids, c.ids), (name, lay)                   # the bit order: ascending ids
        W = (len(ids) + 63) // 64
        assert W == c.W and (len(p.get("ew_off")) != 0) == (W > 1), (name, lay)
        assert (p.eager_lo_end, p.eager_hi_begin, p.abs_min) == (c.lo_end, c.hi_begin, c.abs_min), (name, lay)
        assert p.nabsorbing == c.sinks + 1
        if lay == "tiny" or (not flag and R.AUTO[name] == "tiny"):
            # an eager automaton gets the 64-bit column form; the 5-bit one (Tiny5Pol) was never emitted for one
            assert len(p.get("tiny_col")) == 256 and len(p.get("tiny5_col")) == 0, name
        # the boundaries sit next to states the walk visits: the renumbering puts the emitting states that are not absorbing
        # below lo_end, the silent ones between, the emitting sinks from hi_begin up, DEAD last
        n2o = p.get("new2old").astype(np.int64)
        assert len(n2o) == p.S1
        old = n2o[:c.S]
        assert sorted(old.tolist()) == list(range(c.S))
        sink = old >= c.S - c.sinks
        assert c.emitting[old[:c.lo_end]].all() and not sink[:c.lo_end].any()
        assert not c.emitting[old[c.lo_end:c.hi_begin]].any()
        assert c.emitting[old[c.hi_begin:]].all() and sink[c.hi_begin:].all() and sink[c.abs_min:].all() and not sink[:c.abs_min].any()
    if c.dying:
        assert c.lo_end < c.abs_min < c.hi_begin < c.S        # absorbing states without outputs, and one with
    else:
        assert c.hi_begin == c.abs_min == c.S


def test_lds2_refuses_eager_outputs(hip):
    for name in ("s15", "s1000"):
        with pytest.raises(OSError) as ei:
            hip.Plan(R.case(name).flat, hip.LAYOUT_LDS2)
        assert ei.value.errno == errno.ENOTSUP


def test_every_layout_is_taken_at_both_widths():
    w1 = {lay for a, lay in R.PAIRS if R.case(a).W == 1}
    assert w1 == set(R.LAYOUT_OF), w1
    w2 = {lay for a, lay in R.PAIRS if a == "s1000"}
    assert R.case("s1000").W == 2 and w2 == set(R.BIG)
    assert len(R.case("s1000").ids) == 94 and len(R.case("s200").ids) == 23
    assert {R.case(a).W for a in R.DYING} == {1, 2}


@pytest.mark.parametrize("name", list(R.AUTOMATA))
def test_reference_side_of_the_inputs(name):
    c = R.case(name)
    rows, lens = R.inputs(c.dying)
    em, st = c.all.em, c.all.st
    used = np.zeros(c.E, bool)
    used[c.cols] = True
    assert not em[:, ~used].any()
    every = em.any(axis=0) | c.len.em.any(axis=0)
    assert every[c.cols].all(), (name, c.cols[~every[c.cols]])           # every id of the automaton is emitted by some input
    two = float((em.sum(axis=1) >= 2).mean())
    print(f"{name}: rows that emit at least two ids: {two:.3f}; distinct ids {len(c.cols)}, W = {c.W}")
    assert (lens[list(R.EMPTY_ROWS)] == 0).all() and lens[0] == 0
    # a zero-length input emits the start state's outputs alone
    assert np.array_equal(np.nonzero(c.len.em[0])[0], np.sort(c.start_cols))
    # the two halves of a resumed walk add up, and the second half adds something the first did not have
    adds = float((c.second.em & ~c.first.em).any(axis=1).mean())
    print(f"{name}: rows whose second half adds an id: {adds:.3f}")
    assert c.S < 200 or adds > (0.0 if c.dying else 0.5)                 # (15 states: every id is out after a few bytes)
    if not c.dying:
        assert two > 0.5 and (st >= 0).all()
        return
    sink = st >= c.S - c.sinks
    loud = sink & c.emitting[np.maximum(st, 0)]
    dead = st < 0
    print(f"{name}: rows ending DEAD {dead.mean():.3f}, in an emitting sink {loud.mean():.3f}, in a silent sink {(sink & ~loud).mean():.3f}")
    assert dead.sum() >= 64 and loud.sum() >= 8 and (sink & ~loud).sum() >= 8
    live = (c.len.st >= 0) & (c.len.st < c.S - c.sinks)
    assert live.sum() >= 8                                               # and, at shorter lengths, rows that are still walking
    # the hand-made tiles: DEAD after byte 0 with the start state's set alone
    t = np.arange(64)
    start_only = np.zeros(c.E, bool)
    start_only[c.start_cols] = True
    for tile, is_dead in ((R.TILE_ALL_DEAD, t >= 0), (R.TILE_ALTERNATE, t % 2 == 0), (R.TILE_LANE63, t != 63)):
        r = tile * 64 + t
        assert (rows[r[is_dead], 0] == 0xFF).all()
        assert (G.trace(c.dense, c.cls, 0, rows[r, :1])[:, 1] < 0).tolist() == is_dead.tolist()
        assert (em[r[is_dead]] == start_only).all() and (c.len.em[r[is_dead]] == start_only).all()
