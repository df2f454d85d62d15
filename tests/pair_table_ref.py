"""Automata, inputs and the judge's answers for the pair-table (lds2) walks: tests/test_pair_table_cases.py (CPU) and
tests/test_gpu_pair_table.py (GPU).

The automata are global_ref.affine() at sizes the planner gives the pair table (FSM_HIP_LAYOUT_LDS2: (S + 1) * (C + 1)^2
entries of 16 bits, 61 440 at most).  Every expected value is global_ref's closed formula applied byte by byte in numpy
(trace / walk / ends / carried / endid_slots): ONE trace of the pool's rows per automaton holds the state before every byte,
and every answer -- any stride, any length, any cut -- is a column of it.  Nothing here goes through the library's planner,
its tables or its kernels, and the oracle's table walk is not used.  The rows are uniformly random bytes; a seventh of the lengths
are chosen (pool()) so that the automata with few end states accept enough rows for the end-id tests."""
import functools

import numpy as np

import global_ref as G

NO = G.NO
N, L = 1501, 256                         # odd, no multiple of 64 (23 tiles + 29 rows); 384 KiB of rows
SUBS = (1, 2, 63, 64, 65, 129, N)
STRIDES = (256, 192, 80, 100, 37)        # 2 segments of 128; 64 | 192 but not 128; 16 | 80 but not 64; unaligned rows
EDGE_LENS = (0, 1, 2, 15, 16, 17, 31, 32, 33)
OFF0 = 5                                 # the packed forms start here: inputs begin at odd and even addresses, not at the base

# name -> (S, K, keyword arguments of global_ref.affine, entries of the pair table = (S + 1) * (K + 1)^2)
FAMILY = {
    "small": (400, 4, dict(holes=100, sinks=1, endids=True), 10025),          # every input path fits beside it
    "odd_c1": (120, 7, dict(holes=30, sinks=1), 7744),                        # C1 = 8; quickly absorbing
    "one_image_max": (41, 30, dict(holes=41, endids=True), 40362),            # the largest table with no second image
    "two_images_min": (42, 30, dict(holes=42, endids=True), 41323),           # the smallest with one
    "complete": (300, 12, {}, 50869),                                         # no absorbing state reachable
    "full": (2456, 4, dict(holes=307, sinks=4, endids=True), 61425),          # the largest table there is
}
BEYOND_FULL = (2457, 4, dict(holes=307, sinks=4, endids=True))               # one state more: 61 450 entries, refused


def round16(x):
    return (x + 15) // 16 * 16


def pair_lds_bytes(entries):
    """the LDS the pair table takes in front of any tile: the 256-byte byte -> class map and the table in 16-byte granules"""
    return 256 + round16(2 * entries)


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
    S, K, kw = FAMILY[name][:3]
    flat, dense, cls = G.affine(S, K, **kw)
    tr = G.trace(dense, cls, 0, drawn()[0])
    tr.setflags(write=False)
    return flat, dense, cls, tr


def accepting(name):
    """[N][L + 1] bool: row i cut after t bytes is accepted (the judge's formula, nothing of the library)"""
    flat, _, _, tr = traced(name)
    return (tr >= 0) & flat.is_end.astype(bool)[np.maximum(tr, 0)]


@functools.lru_cache(maxsize=None)
def pool():
    """(rows [N][L], lens [N], cut [N]): the inputs of every test, read-only.

    The lengths are drawn()'s but for every fourth row behind the head's edge lengths: the two neighbours of the hand-over have 6
    end states of 41 and 42 (affine(): s % 7 == 3), so purely random lengths leave 0.115 and 0.123 of the rows accepted, too few
    for the end-id tests (test_pair_table_cases asks for 0.20 of every automaton with end-ids).  Such a row's length moves to the
    NEAREST length at which both neighbours accept it -- unless `small` or `full` accepts the row at its drawn length, so that
    neither of those loses a row.  The rows' bytes, the cut vector and three lengths of four stay as drawn."""
    rows, lens0, cut = drawn()
    ar = np.arange(N)
    both = accepting("one_image_max") & accepting("two_images_min")
    keep = accepting("small")[ar, lens0] | accepting("full")[ar, lens0]
    lens = lens0.copy()
    for i in range(len(EDGE_LENS), N):
        cols = np.nonzero(both[i])[0]
        if i % 4 == 3 and not keep[i] and len(cols):
            lens[i] = cols[np.abs(cols - int(lens0[i])).argmin()]
    lens.setflags(write=False)
    return rows, lens, cut


def edge_batches():
    """batches of lengths for the packed fronts: the edge lengths at the head, and at the very end of the text"""
    _, lens, _ = pool()
    e = np.array(EDGE_LENS, np.uint32)
    head = lens.copy()
    head[:len(e)] = e
    tail = lens.copy()
    tail[-len(e):] = e[::-1]                          # ... the last line has 0 bytes, the one before it 1, ...
    tail2 = lens.copy()
    tail2[-len(e):] = e                               # ... and the last line has 33: its last chunk ends the allocation
    # ... and the text ends in sixteen lines of 1 to 3 bytes, eight of them inside its last 8 bytes: walk_lines32 takes inputs
    # that end there one byte at a time (the policy's next(): for the pair table a lone byte paired with the identity class)
    tail3 = lens.copy()
    tail3[-16:] = (1, 2, 3, 1, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1)
    return {"head": head, "tail": tail, "tail33": tail2, "tail_short": tail3}


def packed_from(rows, lens, off0=OFF0):
    """G.packed with off0 bytes of 0xFF in front: (bytes, u64 offsets [n + 1] starting at off0)"""
    base, off = G.packed(rows, lens)
    return np.concatenate([np.full(off0, 0xFF, np.uint8), base]), off + np.uint64(off0)


class Case:
    """one automaton and the judge's answers on pool(): computed once, left as they are"""

    def __init__(self, name, spec=None):
        self.name = name
        S, K, kw = (FAMILY[name][:3] if spec is None else spec)
        self.S, self.K, self.kw = S, K, kw
        self.entries = (S + 1) * (K + 1) ** 2
        self.sinks = kw.get("sinks", 0)
        rows, lens, cut = pool()
        self.ar = np.arange(N)
        if spec is None:
            self.flat, self.dense, self.cls, self.tr = traced(name)     # tr [N][L + 1]: the state before byte t, after the last
        else:
            self.flat, self.dense, self.cls = G.affine(S, K, **kw)
            self.tr = G.trace(self.dense, self.cls, 0, rows)
            self.tr.setflags(write=False)
        self.st_all = self.tr[:, L]
        self.st_len = self.at(lens)
        self.st_cut = self.at(cut)
        # self-check of the judge (as test_gpu_global_table.Case): walk() agrees with the trace's columns, and the second
        # piece walked from the first piece's state ends where the whole row ends
        assert np.array_equal(G.walk(self.dense, self.cls, 0, rows, lens), self.st_len)
        self.rest = np.zeros((N, L), np.uint8)
        for i in range(N):
            self.rest[i, :L - cut[i]] = rows[i, cut[i]:]
        self.rest.setflags(write=False)
        self.rest_lens = (L - cut.astype(np.int64)).astype(np.uint32)
        assert np.array_equal(G.walk(self.dense, self.cls, 0, self.rest, self.rest_lens, state_in=self.st_cut), self.st_all)
        self.slots = G.endid_slots(S, self.flat.is_end.astype(bool)) if kw.get("endids") else None

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
        hit = fa < L
        return dict(dead=float(dead.mean()), accept=float(acc.mean()), live=float((~dead & ~acc).mean()),
                    band0=float((fa < 16).mean()), band1=float(((fa >= 16) & (fa < 128)).mean()), band2=float(((fa >= 128) & hit).mean()),
                    # the first absorbing COLUMN of the trace (column t + 1 = the state after byte t) is odd: the lane turned on the
                    # first byte of a pair; `second`: on the second one.  Both as shares of all rows.
                    odd=float((hit & (fa % 2 == 0)).mean()), second=float((hit & (fa % 2 == 1)).mean()), distinct=len(np.unique(st)))

    def ids_of(self, state):
        sl = self.slots[state]
        return sl[sl >= 0].astype(np.uint32)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def bites(c, n=N, bands=0.10, each=0.15):
    """the conditions that make the absorbing-lane tests bite, on the first n full-length rows of the pool"""
    s = c.shares(n)
    assert min(s["dead"], s["accept"], s["live"]) >= each, (c.name, n, s)
    assert min(s["band0"], s["band1"], s["band2"]) >= bands, (c.name, n, s)
    assert 0.3 <= s["odd"] <= 0.7, (c.name, n, s)
    assert s["second"] >= bands, (c.name, n, s)       # (the start state has a hole: a quarter of the rows die on byte 0)
    return s
