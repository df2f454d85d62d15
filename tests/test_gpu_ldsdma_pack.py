"""GPU (-m gpu): walk_ldsdma_pack, the LDS-DMA walk that packs the rows which outlive their first segment across tiles.

One wavefront per workgroup and one workgroup per CU (KNOB_WAVES = 1, KNOB_BLOCKS_PER_CU = 1), n = 64 * ncu * 5 + 37 rows: every
wavefront owns five tiles (the first ones a sixth, the last of them partial), tile t is the (t // ncu)-th tile of wavefront
t % ncu, and wavefront w runs tests/ldsdma_pack_ref.SEQUENCES[w % 6] -- tiles with 0, 1, 15, 16, 32 alternating, 49, 63, 64
early-dead rows and 20 bunched at either end, in orders that bring the pending count to exactly 64, from 63 to 111, and to
0, 1 and 63 at the wavefront's end, with in-place tiles between queued ones (tests/test_ldsdma_pack_cases.py holds the queue
arithmetic against the same model on the CPU).  Rows die at byte 0, 15 (early), 16, 17, 127 (first segment), 128, 129, stride - 1
(packed rounds), or never; a row that dies carries from the next 128-byte boundary on a text that a pattern accepts from the
start state (c3) / "Libf" over and over (c1), so a lane that reads another row's slot or walks stale bytes ends elsewhere.

The judge is Oracle.table_walk for c3.npz / c1.npz and tests/global_ref.py for the synthetic tables; the shares of rows dead
after 16 bytes, after 128 bytes, later and never come from the reference's own states before anything is launched."""
import functools
import itertools
import os

import numpy as np
import pytest

import eager_front_ref as R
import global_ref as G
import ldsdma_pack_ref as P
from common import GOLDEN, Golden

pytestmark = pytest.mark.gpu

NO = 0xFFFFFFFF
DEAD = 0xFFFFFFFC
JUNK32, JUNK64 = 0xA5A5A5A5, 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()
    return libfsm_amd


@pytest.fixture(scope="module")
def ncu(hip):
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def bits(bm, n):
    return np.unpackbits(np.ascontiguousarray(bm).view(np.uint8), bitorder="little")[:n].astype(bool)


def c3_rows(die, stride, rng):
    pats = bytes(np.load(os.path.join(GOLDEN, "c3.npz"))["patterns"]).split(b"\n")
    pres = [np.frombuffer(p[1:p.index(b"[")], np.uint8) for p in pats if p][::131]
    n = len(die)
    i = np.arange(n)
    rows = rng.randint(48, 58, (n, stride)).astype(np.uint8)          # digits: the body of every pattern
    pick, pick2 = rng.randint(len(pres), size=n), rng.randint(len(pres), size=n)
    for k, pre in enumerate(pres):
        rows[pick == k, :len(pre)] = pre
    live = die < 0
    rows[live & (i // 3 % 3 == 0), stride - 1] = ord("x")             # accepted by x, accepted by yz, alive and not accepted
    rows[live & (i // 3 % 3 == 1), stride - 2:] = (ord("y"), ord("z"))
    at = (die + 128) // 128 * 128                                     # the segment after the death: a whole accepted text
    for k, pre in enumerate(pres):
        for a in np.unique(at[~live & (at < stride)]):
            sel = ~live & (at == a) & (pick2 == k)
            rows[sel, a:a + len(pre)] = pre
            rows[sel, stride - 1] = ord("x")
    rows[i[~live], die[~live]] = ord("!")                             # no pattern has it: DEAD
    return rows


def c1_rows(die, stride, rng):
    alpha = np.frombuffer(b"abcdeghjkmnopqrtuvwxyz 0123456789", np.uint8)      # no l, i, f, s
    n = len(die)
    i = np.arange(n)
    rows = alpha[rng.randint(0, len(alpha), (n, stride))]
    libf = np.frombuffer(b"Libf", np.uint8)
    live = die < 0
    rows[live & (i // 3 % 3 == 0), stride - 3:] = np.frombuffer(b"Lib", np.uint8)   # alive to the end, one byte short
    for k in np.unique(die[~live]):
        sel = die == k
        kk = max(int(k), 3)                                                    # the absorbing accept state needs four bytes
        rows[sel, kk - 3:kk + 1] = libf
        rows[sel, kk + 1:] = np.resize(libf, stride - kk - 1)
    return rows


def absorbing_states(o, states):
    """which of `states` (the reference's numbering) loop on all 256 bytes: asked of the reference, one byte at a time"""
    every = np.arange(256, dtype=np.uint8).reshape(256, 1)
    out = {DEAD: True}
    for s in np.unique(states):
        if int(s) not in out:
            out[int(s)] = bool((o.state_walk(every, np.full(256, s, np.uint32)) == s).all())
    return np.array([out[int(s)] for s in states], bool)


class Batch:
    """rows of one automaton at one stride with the reference's answers, computed once"""

    def __init__(self, hip, name, stride, ncu, mixed):
        from oracle.pyoracle import Oracle
        self.g = Golden(os.path.join(GOLDEN, name))
        self.o = Oracle(self.g.flat)
        self.n = 64 * ncu * 5 + 37
        self.ncu, self.stride = ncu, stride
        die = P.plan_rows(self.n, ncu, mixed, stride)
        rng = np.random.RandomState(stride + len(name) + mixed)
        self.rows = (c3_rows if name == "c3.npz" else c1_rows)(die, stride, rng)
        self.want = self.o.table_walk(self.rows)
        start = np.full(self.n, hip.STATE_START, np.uint32)
        at = {k: ~absorbing_states(self.o, self.o.state_walk(self.rows, start, np.full(self.n, k, np.uint32))) for k in (16, 128, stride)}
        self.alive16, self.alive128, self.alive_end = at[16], at[128], at[stride]
        self.shares = ((~self.alive16).mean(), (self.alive16 & ~self.alive128).mean(), (self.alive128 & ~self.alive_end).mean(), self.alive_end.mean())
        for a in (self.rows, self.want):
            a.setflags(write=False)

    def waves(self):
        """the model's run of every sixth-of-a-kind wavefront: (events, entries left for the flush)"""
        return [P.model(P.wave_tiles(self.alive16, self.alive128, self.ncu, w)) for w in range(min(self.ncu, 4 * len(P.SEQUENCES)))]


@functools.lru_cache(maxsize=None)
def batch(hip, name, stride, ncu, mixed):
    return Batch(hip, name, stride, ncu, mixed)


def packed_dfa(hip, flat, layout=0):
    dfa = hip.HipDfa(flat, layout)
    dfa.tune(hip.KNOB_WAVES, 1)
    dfa.tune(hip.KNOB_BLOCKS_PER_CU, 1)
    return dfa


def check(dfa, rows, want, *tag, kernel="walk_ldsdma_pack<"):
    end, bm = dfa.exec_batch(np.ascontiguousarray(rows))
    assert kernel in dfa.last_kernel_name(), (dfa.last_kernel_name(),) + tag
    bad = np.nonzero(end != want)[0]
    assert len(bad) == 0, tag + (len(bad), bad[:8], end[bad[:8]], want[bad[:8]])
    assert np.array_equal(bits(bm, len(want)), want != NO), tag


@pytest.mark.parametrize("stride", [256, 384, 1024])
@pytest.mark.parametrize("name", ["c3.npz", "c1.npz"])
def test_early_deaths_only_the_queue_at_its_edges(hip, ncu, name, stride):
    b = batch(hip, name, stride, ncu, False)
    # the reference's own states make the events the sequences are for (c1 turns absorbing at byte 3 where c3 does at byte 0: still
    # early).  Wavefronts 6 .. 11 own exactly five tiles; the first ones a sixth: the batch's partial tile is wavefront 0's
    assert ncu >= 2 * len(P.SEQUENCES)
    runs = b.waves()[len(P.SEQUENCES):2 * len(P.SEQUENCES)]
    assert [left for _, left in runs] == [s[1] for s in P.SEQUENCES]
    pushed = [[t[1] for t in ev if t[0] == "Q"] for ev, _ in runs]
    assert 64 in pushed[0] and pushed[1][:3] == [48, 63, 111] and runs[0][1] == 0 and runs[2][1] == 1 and runs[3][1] == 63
    assert len(b.waves()[0][0]) == 6
    assert b.shares[0] >= 0.1 and b.shares[3] >= 0.1, b.shares
    dfa = packed_dfa(hip, b.g.flat)
    check(dfa, b.rows, b.want, name, stride)
    dfa.close()


@pytest.mark.parametrize("stride", [256, 384, 1024])
@pytest.mark.parametrize("name", ["c3.npz", "c1.npz"])
def test_mixed_deaths_outputs_and_sizes(hip, ncu, name, stride):
    import torch
    b = batch(hip, name, stride, ncu, True)
    assert min(b.shares) >= 0.1, b.shares            # dead after 16 bytes, after 128, later, never: none of them can hide
    if name == "c3.npz":                             # (c1's accepted rows are the dead ones: its absorbing state accepts)
        assert (b.want[b.alive_end] != NO).mean() > 0.2 and (b.want[b.alive_end] == NO).mean() > 0.2
    runs = b.waves()
    assert any(t[0] == "I" for ev, _ in runs for t in ev) and any(t[0] == "Q" and t[2] for ev, _ in runs for t in ev)
    assert any(left > 0 for _, left in runs)
    dfa = packed_dfa(hip, b.g.flat)
    n, want = b.n, b.want
    check(dfa, b.rows, want, name, stride)
    # the sizes at which a wavefront has one tile, full or not, and two; the first wavefront's flush alone
    for m in (1, 63, 64, 65, 129):
        check(dfa, b.rows[:m], want[:m], name, stride, m)
    # outputs: junk in both, junk behind the bitmap's last word; then either output absent
    d_rows = torch.from_numpy(np.array(b.rows)).cuda()
    nw = (n + 63) // 64
    d_end = torch.from_numpy(np.full(n, JUNK32, np.uint32).view(np.int32)).cuda()
    d_bm = torch.from_numpy(np.full(nw + 3, JUNK64, np.uint64).view(np.int64)).cuda()
    dfa.exec_batch_device(d_rows.data_ptr(), stride, n, d_end.data_ptr(), d_bm.data_ptr())
    torch.cuda.synchronize()
    assert "walk_ldsdma_pack<" in dfa.last_kernel_name()
    bm = d_bm.cpu().numpy().view(np.uint64)
    assert np.array_equal(d_end.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(bits(bm[:nw], nw * 64), np.concatenate([want != NO, np.zeros(nw * 64 - n, bool)]))      # spare bits of the last word are 0
    assert (bm[nw:] == JUNK64).all()
    d_bm.fill_(0x1234)
    dfa.exec_batch_device(d_rows.data_ptr(), stride, n, 0, d_bm.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_bm.cpu().numpy().view(np.uint64)[:nw], n), want != NO)
    d_end.fill_(7)
    dfa.exec_batch_device(d_rows.data_ptr(), stride, n, d_end.data_ptr(), 0)
    torch.cuda.synchronize()
    assert np.array_equal(d_end.cpu().numpy().view(np.uint32), want)
    if name == "c3.npz":                             # the ids front: out2 beside the end states
        sets = dfa.ret_sets()
        e1, e2 = dfa.exec_batch_ids(np.ascontiguousarray(b.rows), 1), dfa.exec_batch_ids(np.ascontiguousarray(b.rows), 2)
        assert "walk_ldsdma_pack<" in dfa.last_kernel_name()
        assert np.array_equal(e1 == NO, want == NO) and np.array_equal(e2 == NO, want == NO)
        for s, k1, k2 in set(zip(want[want != NO].tolist(), e1[want != NO].tolist(), e2[want != NO].tolist())):
            ids = b.g.flat.endids_of(s)
            assert k1 == (int(ids[0]) if len(ids) else 0xFFFFFFFE) and np.array_equal(sets[k2], ids), s
    dfa.close()


def test_what_keeps_walk_ldsdma(hip, ncu):
    b = batch(hip, "c3.npz", 256, ncu, True)
    dfa = packed_dfa(hip, b.g.flat)
    dfa.tune(hip.KNOB_PACK, 0)
    check(dfa, b.rows, b.want, "KNOB_PACK = 0", kernel="walk_ldsdma<")
    dfa.tune(hip.KNOB_PACK, -1)
    check(dfa, b.rows, b.want, "KNOB_PACK = -1")
    dfa.tune(hip.KNOB_EARLY_RETIRE, 1)               # the per-lane load skip off: the old default
    check(dfa, b.rows, b.want, "early = 1", kernel="walk_ldsdma<")
    dfa.tune(hip.KNOB_PACK, 1)                       # ... unless the kernel is asked for wherever it exists
    check(dfa, b.rows, b.want, "early = 1, KNOB_PACK = 1")
    dfa.tune(hip.KNOB_EARLY_RETIRE, -1)
    # one-segment rows
    half = np.ascontiguousarray(b.rows[:, :128])
    check(dfa, half, b.o.table_walk(half), "stride 128", kernel="walk_ldsdma<")
    # a resumed call: the second half from the states the first half left
    start = np.full(b.n, hip.STATE_START, np.uint32)
    st, _ = dfa.exec_batch_resume(half, start)
    assert "walk_ldsdma<" in dfa.last_kernel_name()
    st2, end2 = dfa.exec_batch_resume(np.ascontiguousarray(b.rows[:, 128:]), st)
    assert "walk_ldsdma<" in dfa.last_kernel_name()
    assert np.array_equal(end2, b.want)
    dfa.close()
    # an eager automaton: its walks stay where they were
    c = R.case("s200_dying")
    dfa = hip.HipDfa(c.flat, R.LAYOUT_OF["lds"])
    end, _ = dfa.exec_eager_words(R.inputs(True)[0])
    assert "walk_ldsdma<" in dfa.last_kernel_name() and "EagerPol" in dfa.last_kernel_name()
    assert np.array_equal(end, c.all.end)
    dfa.close()


AFFINE = {"tiny": (15, 4, dict(holes=16, sinks=3)), "comb256": (15, 4, dict(holes=16, sinks=3)), "lds": (200, 4, dict(holes=64, sinks=3)),
          "ldsself": (200, 4, dict(holes=64, sinks=3)), "comb": (200, 4, dict(holes=64, sinks=3)), "combself": (200, 4, dict(holes=64, sinks=3)),
          "sparse": (1000, 4, dict(holes=64, sinks=10)), "global": (1000, 4, dict(holes=64, sinks=10))}


@pytest.mark.parametrize("lay", list(AFFINE))
def test_every_layout_behind_lds_dma(hip, ncu, lay):
    """"dying" affine automata (global_ref.affine: the states s % holes == 0, the start state among them, have no edge for the last
    byte class; the last states are absorbing accepts).  A row of 0x80 bytes never dies and is in such a state at every eighth byte:
    one 0xFF there is DEAD.  Rows die at byte 0 (tiles alternating and 63-dead by turns, and some all alive), at 16, 120, 128, 136,
    248 or never (the last three bytes may still take it into a sink); a dead row is 0xFF from the next segment on, which takes a live walk that reads it elsewhere."""
    S, K, kw = AFFINE[lay]
    flat, dense, cls = G.affine(S, K, **kw)
    L, n = 256, 64 * ncu * 5 + 37
    i = np.arange(n)
    rows = np.full((n, L), 0x80, np.uint8)
    ends27 = np.array(list(itertools.product([0x00, 0x40, 0x80], repeat=3)), np.uint8)
    rows[::2, L - 3:] = ends27[i[::2] % 27]                            # 27 ends for every other row, some of them accepted
    early = np.where((i // 64) % 3 == 0, i % 2 == 1, np.where((i // 64) % 3 == 1, i % 64 != 5, False))
    die = np.where(early, 0, np.take([-1, 16, 128, -1, 120, 136, -1, 248], (i // 3) % 8))
    for k in np.unique(die[die >= 0]):
        rows[die == k, k] = 0xFF
        rows[die == k, (k + 128) // 128 * 128:] = 0xFF
    tr = G.trace(dense, cls, 0, rows)
    gone = (tr < 0) | (tr >= S - kw["sinks"])
    assert np.array_equal(gone[:, 16], (die >= 0) & (die < 16)) and np.array_equal(gone[:, 128], (die >= 0) & (die < 128))
    sh = (gone[:, 16].mean(), (gone[:, 128] & ~gone[:, 16]).mean(), (gone[:, L] & ~gone[:, 128]).mean(), (~gone[:, L]).mean())
    assert min(sh) >= 0.1, sh
    want = G.ends(flat, tr[:, L])
    assert (want != NO).sum() > 1000 and (want == NO).sum() > 1000
    dfa = packed_dfa(hip, flat, R.LAYOUT_OF[lay])
    dfa.tune(hip.KNOB_INPUT_MODE, hip.IN_LDSDMA)
    dfa.tune(hip.KNOB_SEG, 128)
    if lay == "sparse":
        dfa.tune(hip.KNOB_SPARSE_FAST, 1)            # the record walk, not the lazy form (which has kernels of its own)
    check(dfa, rows, want, lay)
    dfa.close()
