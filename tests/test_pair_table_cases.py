"""CPU: the case table of tests/test_gpu_pair_table.py, checked before anything is launched -- that every member of
pair_table_ref.FAMILY plans as the pair table (FSM_HIP_LAYOUT_LDS2) under AUTO, on which side of the hand-over to a second
image it lies, where the 16-bit entry ends, and that the judge's answers on the shared pool are what the pool was made for:
no GPU test can pass on trivial rows.  Nothing here needs a GPU: hip.Plan is the host-side planner, the rest is numpy."""
import errno

import numpy as np
import pytest

import global_ref as G
import pair_table_ref as R

NO = R.NO
LDS_LIMIT = 163840                       # all of a workgroup's LDS on the device (fsm_hip.hip caps lds_limit at 160 KiB)
RAGGED_WAVE_LDS = 8192 + 64 * 16 + 1024   # walk_kernels.h FSMHIP_RAGGED_WAVE_LDS: a wavefront's tile + ring + row records
HAND_OVER = LDS_LIMIT - 8 * RAGGED_WAVE_LDS   # 81 920: a pair table above it (with its byte map) keeps a second image


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
    assert 0.4 <= float((lens % 2).mean()) <= 0.6 and 0.4 <= float((cut % 2).mean()) <= 0.6
    assert int(lens.max()) == R.L and len(np.unique(rows)) == 256
    assert R.SUBS == (1, 2, 63, 64, 65, 129, R.N) and R.OFF0 % 2 == 1
    for name, b in R.edge_batches().items():
        assert set(R.EDGE_LENS) <= set(b.tolist()), name


@pytest.mark.parametrize("name", list(R.FAMILY))
def test_member_plans_as_the_pair_table(hip, name):
    S, K, kw, entries = R.FAMILY[name]
    c = R.case(name)
    p = hip.Plan(c.flat, 0)
    assert p.layout == hip.LAYOUT_LDS2, (name, p.layout)
    assert (p.S1, p.C) == (S + 1, K)
    tab = p.get("lds_tab")
    assert len(tab) == entries == (S + 1) * (K + 1) ** 2 <= 61440
    forced = hip.Plan(c.flat, hip.LAYOUT_LDS2)
    assert forced.layout == hip.LAYOUT_LDS2 and np.array_equal(forced.get("lds_tab"), tab)
    assert p.nabsorbing == c.sinks + 1                                  # the sinks and DEAD
    assert int(tab.max()) == S * (K + 1) ** 2 < 65536                    # an entry is a row index in entries: DEAD's is the largest
    # every row from abs_min on sends EVERY pair to itself: whether an absorbing lane's bytes are masked (mask_absorbing) or
    # foreign, and on which side of abs_min itself absorbing() falls, cannot change an answer -- only a live row taken for an
    # absorbing one can (the GPU file's absorbing-lane tests)
    unit = (K + 1) ** 2
    top = tab.reshape(S + 1, unit)[p.abs_min:]
    assert len(top) == c.sinks + 1 and (top == (np.arange(p.abs_min, S + 1) * unit)[:, None]).all()
    # ... and the identity class is the identity: T[s][c * C1 + C] is one step, T[s][C * C1 + C] none
    rows_of = tab.reshape(S + 1, K + 1, K + 1)
    assert (rows_of[:, K, K] == np.arange(S + 1) * unit).all()


def test_hand_over_lies_between_the_two_neighbours():
    assert HAND_OVER == 81920
    one, two = R.case("one_image_max"), R.case("two_images_min")
    assert (one.entries, two.entries) == (40362, 41323) and two.S == one.S + 1 and two.K == one.K
    assert 256 + 2 * one.entries == 80980 and 256 + 2 * two.entries == 82902
    assert R.pair_lds_bytes(one.entries) == 80992 <= HAND_OVER < R.pair_lds_bytes(two.entries) == 82912
    # of the family: which members keep a second image under AUTO
    second = {n: R.pair_lds_bytes(R.FAMILY[n][3]) > HAND_OVER for n in R.FAMILY}
    assert second == dict(small=False, odd_c1=False, one_image_max=False, two_images_min=True, complete=True, full=True)


def test_one_state_beyond_the_largest_table_is_refused(hip):
    S, K, kw = R.BEYOND_FULL
    assert (S + 1) * (K + 1) ** 2 == 61450 > 61440 >= R.case("full").entries == 61425
    flat = G.affine(S, K, **kw)[0]
    with pytest.raises(OSError) as ei:
        hip.Plan(flat, hip.LAYOUT_LDS2)
    assert ei.value.errno == errno.ENOTSUP
    assert hip.Plan(flat, 0).layout != hip.LAYOUT_LDS2


@pytest.mark.parametrize("name", ["small", "full"])
def test_pool_dies_early_late_and_on_either_byte_of_a_pair(name):
    c = R.case(name)
    s = R.bites(c)       # dead, accept, live >= 0.15 each; the three bands >= 0.10 each; 0.3 <= odd <= 0.7; second byte >= 0.10
    print(name, {k: round(v, 3) if isinstance(v, float) else v for k, v in s.items()})
    # ... and for the sub-batches the absorbing-lane tests launch
    for n in (129, R.N):
        R.bites(c, n)


def test_odd_c1_absorbs_quickly():
    c = R.case("odd_c1")
    s = c.shares()
    print("odd_c1", s)
    # (no bound of the issue's: at least 150 of the 1501 rows turn absorbing on either byte of a pair, and as many end either way)
    assert s["dead"] >= 0.10 and s["accept"] >= 0.10 and s["band0"] >= 0.10 and s["odd"] >= 0.10 and s["second"] >= 0.10, s


@pytest.mark.parametrize("name", ["one_image_max", "two_images_min"])
def test_neighbours_of_the_hand_over_die_and_live(name):
    s = R.case(name).shares()
    print(name, s)
    assert s["dead"] >= 0.10 and s["live"] >= 0.5 and s["accept"] == 0, s


def test_complete_has_nothing_absorbing():
    c = R.case("complete")
    s = c.shares()
    print("complete", s)
    assert not c.absorbing(c.tr).any() and s["distinct"] >= 250 and s["live"] == 1.0, s


@pytest.mark.parametrize("name", ["small", "one_image_max", "two_images_min", "full"])
def test_accepted_rows_carry_several_id_sets(name):
    """Under `lens`: accepted rows carry at least two distinct id sets, and at least 20 % of the rows are accepted.

    Lengths drawn at random alone give small 0.205, full 0.201, one_image_max 0.115, two_images_min 0.123: the two neighbours of the
    hand-over have 6 end states of 41 / 42 (affine(): s % 7 == 3), and random bytes spread the walk evenly over the states.  The
    bound stays and the pool changed (pair_table_ref.pool): 209 of the 1 501 lengths moved, by 36 bytes on average, to the nearest
    length at which both neighbours accept the row.  Now: small 0.217 (20 distinct sets), full 0.210 (20), one_image_max 0.239 (6),
    two_images_min 0.249 (6)."""
    c = R.case(name)
    _, lens, _ = R.pool()
    end = c.ends(c.st_len)
    hit = end != NO
    sets = {tuple(c.ids_of(int(s)).tolist()) for s in end[hit]}
    print(name, f"accepted under lens: {hit.mean():.3f} ({int(hit.sum())} rows), distinct id sets: {len(sets)}")
    assert len(sets) >= 2 and all(len(s) >= 1 for s in sets) and int(hit.sum()) >= 100, (name, sets)
    assert float(hit.mean()) >= 0.20, (name, hit.mean())


@pytest.mark.parametrize("name", list(R.FAMILY))
def test_judge_agrees_with_itself(name):
    """(Case.__init__ asserts it: walk() against the trace's columns, and the second piece walked from the first piece's state
    ends where the whole row ends) -- here once more for a cut vector of its own, and for the clipped lengths of a short stride"""
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
