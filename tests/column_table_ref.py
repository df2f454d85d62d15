"""Automata, inputs and the judge's answers for the column-table (FSM_HIP_LAYOUT_TINY) walks: tests/test_column_table_cases.py
(CPU) and tests/test_gpu_column_table.py (GPU).

The column tables hold automata of up to 15 states (S1 = S + DEAD <= 16): the 5-bit form (Tiny5Pol) for S1 <= 6, the 64-bit
nibble form (TinyPol<uint64_t>) above.  global_ref.affine() does not serve at these sizes: every class is a permutation of the
states, so some state enters an absorbing accept with probability ~1/4 per byte and every row is absorbed within a chunk.
column(S, K, sinks) is a closed formula again: the live states are permuted among themselves, and ONE cell leads to DEAD (the
hole) and ONE to the absorbing accept (the door), so that rows stay live for tens of bytes and die or are accepted throughout
a 256-byte row.

Every expected value is global_ref's judge (trace / walk / ends / carried / endid_slots) on column()'s dense table: ONE trace
of the pool's rows per automaton holds the state before every byte, and every answer -- any stride, any length, any cut -- is
a column of it.  Nothing here goes through the library's planner, its tables or its kernels, and the oracle's table walk is
not used.  The rows are uniformly random bytes: about half of them are >= 0x80, and every byte value occurs."""
import functools
from math import gcd

import numpy as np

import global_ref as G
from libfsm_amd import FlatDfa
from libfsm_amd.capi import RANGE_DTYPE

NO = G.NO
N, L = 1501, 256                         # odd, no multiple of 64 (23 tiles + 29 rows); 384 KiB of rows
SUBS = (1, 2, 63, 64, 65, 129, N)
STRIDES = (256, 192, 80, 100, 37)        # 2 segments of 128; 64 | 192 but not 128; 16 | 80 but not 64; unaligned rows
EDGE_LENS = (0, 1, 2, 15, 16, 17, 31, 32, 33)
OFF0 = 5                                 # the packed forms (walk_buffers.Packed) start here: inputs begin at odd and even addresses

# name -> (S, K, sinks, end-ids, the hole)
FAMILY = {
    "one": (1, 256, 0, False, True),             # S1 = 2, the smallest table there is
    "two": (2, 256, 1, False, True),             # start, sink, DEAD and nothing else
    "five": (5, 80, 1, True, True),              # S1 = 6: the last automaton with the 5-bit form
    "six": (6, 72, 1, True, True),               # S1 = 7: the first with only the 64-bit form
    "fifteen": (15, 24, 1, True, True),          # S1 = 16: every nibble used, DEAD is 15
    "complete15": (15, 24, 0, False, False),     # no absorbing state reachable
    "sixteen": (16, 24, 1, False, True),         # one state too many
}
TABLE_LDS = 65536                        # 256 columns x 64 copies x 4 bytes, or x 32 copies x 8 bytes


def column(S, K, sinks=0, *, endids=False, hole=True):
    """-> (FlatDfa, dense[S][K] int64 with -1 = no edge, cls[256]).  Start state 0.

    live = S - sinks; live state s on class c goes to (a_c * s + b_c) % live, a_c cycling through the first eight odd numbers
    from 3 that are coprime to live, b_c = 1 + 37 c.  The hole: dense[0][K - 1] = -1.  The door (with sinks):
    dense[live - 1][K - 2] = S - 1.  The sinks loop on every class.  End states: the live states with s % 3 == 0 (the start
    state among them: an empty input is a hit) and the sinks."""
    cls, bounds = G.class_map(K)
    live = S - sinks
    assert live >= 1 and K >= 2
    mult = [a for a in range(3, 200, 2) if gcd(a, live) == 1][:8]
    s = np.arange(S, dtype=np.int64)
    c = np.arange(K, dtype=np.int64)
    a = np.array([mult[k % len(mult)] for k in range(K)], np.int64)
    b = 1 + 37 * c
    dense = (s[:, None] * a[None, :] + b[None, :]) % live
    if hole:
        dense[0, K - 1] = -1
    if sinks:
        dense[live - 1, K - 2] = S - 1
        dense[live:, :] = s[live:, None]
    is_end = s % 3 == 0
    is_end[live:] = True
    keep = dense >= 0
    r = np.zeros(int(keep.sum()), RANGE_DTYPE)
    r["lo"] = np.broadcast_to(bounds[:-1][None, :], (S, K))[keep]
    r["hi"] = np.broadcast_to(bounds[1:][None, :] - 1, (S, K))[keep]
    r["to"] = dense[keep]
    edge_off = np.zeros(S + 1, np.uint32)
    edge_off[1:] = np.cumsum(keep.sum(axis=1))
    endid_off, ids = np.zeros(S + 1, np.uint32), np.zeros(0, np.uint32)
    if endids:
        slots = G.endid_slots(S, is_end)
        endid_off[1:] = np.cumsum((slots >= 0).sum(axis=1))
        ids = slots[slots >= 0].astype(np.uint32)
    flat = FlatDfa(S, 0, edge_off, r, is_end.astype(np.uint8), endid_off, ids, None, None)
    return flat, dense, cls


@functools.lru_cache(maxsize=None)
def drawn():
    """(rows [N][L], lens [N], cut [N]) as the random generator gives them: uniformly random bytes, varlens() + 2, 31, 32, 33"""
    rng = np.random.RandomState(5)
    rows = rng.randint(0, 256, (N, L)).astype(np.uint8)
    lens = G.varlens(N, L, rng)                       # 0, 1, 15, 16, 17, then random
    lens[5:9] = (2, 31, 32, 33)
    cut = rng.randint(0, L + 1, N).astype(np.uint32)
    cut[:8] = (0, 1, 2, 15, 16, 17, L - 1, L)
    for a in (rows, lens, cut):
        a.setflags(write=False)
    return rows, lens, cut


@functools.lru_cache(maxsize=None)
def traced(name):
    """(flat, dense, cls, trace [N][L + 1] of the pool's rows: the state before byte t, after the last) of a family member"""
    S, K, sinks, endids, hole = FAMILY[name]
    flat, dense, cls = column(S, K, sinks, endids=endids, hole=hole)
    tr = G.trace(dense, cls, 0, drawn()[0])
    tr.setflags(write=False)
    return flat, dense, cls, tr


COVERED = ("five", "six", "fifteen")     # every state of these is where some row stands after L, lens[i] and cut[i] bytes


def missing(name, at):
    """the states of a member (DEAD = -1 among them) in which no row stands after at[i] bytes"""
    S = FAMILY[name][0]
    tr = traced(name)[3]
    return sorted(set(range(-1, S)) - set(tr[np.arange(N), np.asarray(at, np.int64)].tolist()))


@functools.lru_cache(maxsize=None)
def pool():
    """(rows [N][L], lens [N], cut [N]): the inputs of every test, read-only.

    The bytes and the cut vector stay as drawn.  Where the drawn lengths leave a state of `five`, `six` or `fifteen` without a
    row that ends in it, the length of the first row behind the head's edge lengths that passes through the state (and whose
    length has not been moved yet) moves to the NEAREST length at which it stands there, as pair_table_ref.pool() moves
    lengths: never the bytes."""
    rows, lens0, cut = drawn()
    lens = lens0.copy()
    moved = set()
    for name in COVERED:
        tr = traced(name)[3]
        for q in missing(name, lens):
            for i in range(len(EDGE_LENS), N):
                cols = np.nonzero(tr[i] == q)[0]
                if i not in moved and len(cols):
                    lens[i] = cols[np.abs(cols - int(lens0[i])).argmin()]
                    moved.add(i)
                    break
    lens.setflags(write=False)
    return rows, lens, cut


def edge_batches():
    """batches of lengths for the packed fronts: the edge lengths at the head, and at the very end of the text
    (pair_table_ref.edge_batches() rebuilt on this pool)"""
    _, lens, _ = pool()
    e = np.array(EDGE_LENS, np.uint32)
    head = lens.copy()
    head[:len(e)] = e
    tail = lens.copy()
    tail[-len(e):] = e[::-1]                          # ... the last line has 0 bytes, the one before it 1, ...
    tail2 = lens.copy()
    tail2[-len(e):] = e                               # ... and the last line has 33: its last chunk ends the allocation
    # ... and the text ends in sixteen lines of 1 to 3 bytes, eight of them inside its last 8 bytes: walk_lines32 takes inputs
    # that end there one byte at a time
    tail3 = lens.copy()
    tail3[-16:] = (1, 2, 3, 1, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1)
    return {"head": head, "tail": tail, "tail33": tail2, "tail_short": tail3}


class Case:
    """one automaton and the judge's answers on pool(): computed once, left as they are"""

    def __init__(self, name):
        self.name = name
        self.S, self.K, self.sinks, self.endids, self.hole = FAMILY[name]
        S = self.S
        rows, lens, cut = pool()
        self.ar = np.arange(N)
        self.flat, self.dense, self.cls, self.tr = traced(name)     # tr [N][L + 1]: the state before byte t, after the last
        self.st_all = self.tr[:, L]
        self.st_len = self.at(lens)
        self.st_cut = self.at(cut)
        # self-check of the judge (as pair_table_ref.Case): walk() agrees with the trace's columns, and the second piece
        # walked from the first piece's state ends where the whole row ends
        assert np.array_equal(G.walk(self.dense, self.cls, 0, rows, lens), self.st_len)
        self.rest = np.zeros((N, L), np.uint8)
        for i in range(N):
            self.rest[i, :L - cut[i]] = rows[i, cut[i]:]
        self.rest.setflags(write=False)
        self.rest_lens = (L - cut.astype(np.int64)).astype(np.uint32)
        assert np.array_equal(G.walk(self.dense, self.cls, 0, self.rest, self.rest_lens, state_in=self.st_cut), self.st_all)
        self.slots = G.endid_slots(S, self.flat.is_end.astype(bool)) if self.endids else None

    def at(self, lens):
        """the state of every row after its first lens[i] bytes (-1 = DEAD)"""
        return self.tr[self.ar[:len(lens)], np.asarray(lens, np.int64)]

    def ends(self, states):
        return G.ends(self.flat, states)

    def absorbing(self, states):
        """DEAD or an absorbing accept (the last `sinks` states)"""
        st = np.asarray(states)
        return (st < 0) | (st >= self.S - self.sinks)

    def first_absorbing(self, n=N):
        """per row the index of the byte that made it absorbing, L where none did (full-length rows)"""
        a = self.absorbing(self.tr[:n, 1:])
        return np.where(a.any(axis=1), a.argmax(axis=1), L)

    def shares(self, n=N):
        """what the conditions are asserted on, for the first n full-length rows"""
        st = self.tr[:n, L]
        dead, acc = st < 0, st >= self.S - self.sinks
        fa = self.first_absorbing(n)
        return dict(dead=float(dead.mean()), accept=float(acc.mean()), live=float((~dead & ~acc).mean()),
                    band0=float((fa < 16).mean()), band1=float(((fa >= 16) & (fa < 128)).mean()), band2=float(((fa >= 128) & (fa < L)).mean()),
                    distinct=len(np.unique(st)))

    def ids_of(self, state):
        sl = self.slots[state]
        return sl[sl >= 0].astype(np.uint32)

    def states(self):
        """every state a row can be handed: the automaton's own, then DEAD (-1)"""
        return list(range(self.S)) + [-1]


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def bites(c, n=N, bands=0.08, each=0.15):
    """the conditions that make the absorbing-lane tests bite, on the first n full-length rows of the pool"""
    s = c.shares(n)
    assert min(s["dead"], s["accept"], s["live"]) >= each, (c.name, n, s)
    assert min(s["band0"], s["band1"], s["band2"]) >= bands, (c.name, n, s)
    return s
