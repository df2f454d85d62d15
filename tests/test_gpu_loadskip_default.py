"""GPU (-m gpu): the per-lane load skip as the DEFAULT of a plain walk.

A dfa created without FSM_HIP_NO_EARLY_RETIRE whose automaton can reach an absorbing state stops fetching a row once
that row's state is absorbing (FSM_HIP_KNOB_EARLY_RETIRE bits 0 and 1), and the LDS-DMA walk asks for a row's second
segment only after it has walked the first 16 bytes.  No knob of that family is touched here: the default is what is
under test, and the same rows go through a dfa created WITH the flag (which streams everything).  The judge is
Oracle.table_walk, bit for bit.

The rows: "dying" at byte k means byte k is the one that takes the row into an absorbing state (for c3.npz, anchored
patterns, the DEAD state; for c1.npz, [Ll]ibf+(sm)*, the absorbing ACCEPT state, which needs four bytes: k < 3 becomes 3),
k in 0, 15, 16, 17, 127, 128, 129, stride - 1, and rows that never do.  After its death a c3 row carries, from the next
128-byte boundary on, a text that one of the patterns accepts when walked from the start state, a c1 row "Libf" over
and over: a lane that reads another row's slot, or walks a slot's stale bytes while alive, ends in another state.
Tiles (64 rows) with 0, 1, 32 alternating, 63 and 64 dead rows, and with 20 dead rows bunched at either end."""
import os

import numpy as np
import pytest

from common import GOLDEN, Golden

pytestmark = pytest.mark.gpu

NO = 0xFFFFFFFF
DIE_AT = (0, 15, 16, 17, 127, 128, 129, -1)      # -1: stride - 1


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


def tile_masks():
    """dead[i] for the 64 rows of each kind of tile"""
    k = np.arange(64)
    return [k < 0, k == 37, k % 2 == 1, k != 0, k >= 0, k < 20, k >= 44, k % 2 == 0, k != 63, k == 0, k == 63]


def c3_rows(n, stride, rng):
    """-> rows, die (byte index at which the row turns absorbing, -1: never)"""
    pats = bytes(np.load(os.path.join(GOLDEN, "c3.npz"))["patterns"]).split(b"\n")
    pres = [p[1:p.index(b"[")] for p in pats if p]
    masks = tile_masks()
    rows = np.zeros((n, stride), np.uint8)
    die = np.full(n, -1, np.int64)
    nd = 0
    for i in range(n):
        dead = masks[(i // 64) % len(masks)][i % 64]
        pre = pres[rng.randint(len(pres))]
        r = rng.randint(48, 58, stride).astype(np.uint8)          # digits: the body of every pattern
        r[:len(pre)] = np.frombuffer(pre, np.uint8)
        if dead:
            k = DIE_AT[nd % len(DIE_AT)]
            nd += 1
            k = stride - 1 if k < 0 or k >= stride else k
            r[k] = ord("!")                                       # no pattern has it: DEAD (at byte 0: instead of the prefix)
            die[i] = k
            at = (k + 128) // 128 * 128                           # the next segment: a whole accepted text to the row's end
            if at < stride:
                p2 = pres[rng.randint(len(pres))]
                r[at:at + len(p2)] = np.frombuffer(p2, np.uint8)
                r[stride - 1] = ord("x")
        else:
            kind = i % 3                                          # accepted by x, accepted by yz, alive and not accepted
            if kind == 0:
                r[stride - 1] = ord("x")
            elif kind == 1:
                r[stride - 2:] = (ord("y"), ord("z"))
        rows[i] = r
    return rows, die


def c1_rows(n, stride, rng):
    alpha = np.frombuffer(b"abcdeghjkmnopqrtuvwxyz 0123456789", np.uint8)      # no l, i, f, s
    masks = tile_masks()
    rows = alpha[rng.randint(0, len(alpha), (n, stride))]
    die = np.full(n, -1, np.int64)
    libf = np.frombuffer(b"Libf", np.uint8)
    nd = 0
    for i in range(n):
        if masks[(i // 64) % len(masks)][i % 64]:
            k = DIE_AT[nd % len(DIE_AT)]
            nd += 1
            k = stride - 1 if k < 0 or k >= stride else max(k, 3)
            rows[i, k - 3:k + 1] = libf
            die[i] = k
            tail = rows[i, k + 1:]
            tail[:] = np.resize(libf, len(tail))
        elif i % 3 == 0:
            rows[i, stride - 3:] = np.frombuffer(b"Lib", np.uint8)       # alive to the end, one byte short
    return rows, die


def check_deaths(hip, dfa, o, rows, die):
    """the rows do what their construction says: not absorbing before byte die[i], absorbing after it"""
    n, stride = rows.shape
    start = np.full(n, hip.STATE_START, np.uint32)
    before = o.state_walk(rows, start.copy(), np.where(die < 0, stride, die).astype(np.uint32))
    after = o.state_walk(rows, start.copy(), np.where(die < 0, stride, die + 1).astype(np.uint32))

    def absorbing(s):
        return s == 0xFFFFFFFC or dfa.state_is_absorbing(int(s))

    for i in range(min(n, 2 * 64 * len(tile_masks()))):
        assert not absorbing(before[i]), (i, die[i])
        assert absorbing(after[i]) == (die[i] >= 0), (i, die[i])


@pytest.mark.parametrize("stride", [128, 256, 1024])
@pytest.mark.parametrize("name", ["c3.npz", "c1.npz"])
def test_default_walk_skips_dead_rows_and_answers_as_the_oracle(hip, name, stride):
    from oracle.pyoracle import Oracle
    g = Golden(os.path.join(GOLDEN, name))
    o = Oracle(g.flat)
    rng = np.random.RandomState(stride + len(name))
    nmax = 4097
    rows_all, die_all = (c3_rows if name == "c3.npz" else c1_rows)(nmax, stride, rng)
    want_all = o.table_walk(rows_all)
    # what the rows are for: dead rows (for c3: all of them rejected although a pattern's text follows), live ones of every kind
    dead = die_all >= 0
    assert dead.sum() > 1500 and (~dead).sum() > 1500
    if name == "c3.npz":
        assert (want_all[dead] == NO).all() and (want_all[~dead] != NO).sum() > 800 and (want_all[~dead] == NO).sum() > 400
        if stride > 128:      # the text after the death of a row that dies in its first segment is an accepted one
            early = dead & (die_all < 128)
            assert (o.table_walk(np.ascontiguousarray(rows_all[early][:, 128:])) != NO).all()
    else:
        assert (want_all[dead] != NO).all() and (want_all[~dead] == NO).all()
    for flags in (0, hip.NO_EARLY_RETIRE):
        for layout in hip.ALL_LAYOUTS:
            try:
                dfa = hip.HipDfa(g.flat, layout | flags)
            except OSError:
                continue
            if flags == 0 and layout == hip.ALL_LAYOUTS[0]:
                check_deaths(hip, dfa, o, rows_all, die_all)
            sets = dfa.ret_sets()
            # the front's own choice of kernel, then the two kernels that have the skip: LDS-DMA at both segment sizes, and per-lane
            # loads without the register double-buffer
            for mode, seg, nb, pre in ((-1, 0, 0, 1), (hip.IN_LDSDMA, 128, 0, 1), (hip.IN_LDSDMA, 64, 0, 1), (hip.IN_DIRECT, 0, 4, 0)):
                if mode >= 0:
                    dfa.tune(hip.KNOB_INPUT_MODE, mode)
                    dfa.tune(hip.KNOB_SEG, seg)
                    dfa.tune(hip.KNOB_NB, nb)
                    dfa.tune(hip.KNOB_PREFETCH, pre)
                for n in (1, 63, 65, nmax):
                    rows, want = np.ascontiguousarray(rows_all[:n]), want_all[:n]
                    end, bm = dfa.exec_batch(rows)
                    bad = np.nonzero(end != want)[0]
                    assert len(bad) == 0, (name, stride, flags, layout, mode, seg, n, bad[:8], die_all[bad[:8]])
                    assert np.array_equal(bits(bm, n), want != NO), (name, stride, flags, layout, mode, seg, n)
                    if seg == 64 or (n != 65 and n != nmax):
                        continue
                    # end-ids from the kernel: the lowest id, and the index of the end state's id set
                    e1, e2 = dfa.exec_batch_ids(rows, 1), dfa.exec_batch_ids(rows, 2)
                    assert np.array_equal(e1 == NO, want == NO) and np.array_equal(e2 == NO, want == NO), (name, stride, flags, layout, mode, n)
                    for s, k1, k2 in set(zip(want[want != NO].tolist(), e1[want != NO].tolist(), e2[want != NO].tolist())):
                        ids = g.flat.endids_of(s)
                        assert k1 == (int(ids[0]) if len(ids) else 0xFFFFFFFE), (name, stride, flags, layout, mode, n, s)
                        assert np.array_equal(sets[k2], ids), (name, stride, flags, layout, mode, n, s)
            dfa.close()
