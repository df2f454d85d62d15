"""The automata, inputs and reference answers of tests/test_gpu_eager_front.py and tests/test_eager_front_cases.py: the
single-DFA eager walks (EagerPol / EagerWidePol, plain and resumed) on every layout and input path.

Automata are global_ref.affine at sizes the LDS layouts accept; every answer is global_ref.walk_eager / walk / ends / carried,
the closed formula byte by byte in numpy.  Id sets are compared as uint64 word arrays built from emitted[n][E] and the
automaton's own bit order (bit b holds the b-th smallest id: HipDfa.eager_id(b), the planner's eager_ids)."""
import functools

import numpy as np

import global_ref as G

NO = 0xFFFFFFFF
N, L, HALF = 4099, 256, 128             # odd, no multiple of 64 or 128: 65 tiles, the last one of three rows
SUBS = (1, 63, 64, 65, 129, N)
# the dying cases' hand-made tiles: rows whose first byte takes state 0's missing edge (DEAD after byte 0)
TILE_ALL_DEAD, TILE_ALTERNATE, TILE_LANE63 = 4, 5, 6
EMPTY_ROWS = (63, 64, 127, 128, 129, N - 1)     # zero-length inputs at tile boundaries (lens[0] is 0 already)

# name -> (S, K, keyword arguments of global_ref.affine)
AUTOMATA = {
    "s15": (15, 4, dict(eager=40, every=3)),                                   # 5 emitting states, 7 ids: the column table
    "s15_dying": (15, 4, dict(eager=40, every=3, holes=16, sinks=3)),          # sink 12 emits, 13 and 14 do not; comb256 takes it
    "s200": (200, 4, dict(eager=40)),                                          # 23 ids, W = 1
    "s200_dying": (200, 4, dict(eager=40, holes=64, sinks=3)),                 # sink 198 = 11 * 18 emits, 197 and 199 do not
    "s200_k29": (200, 29, dict(eager=40)),                                     # the planner's own choice is combself
    "s1000": (1000, 4, dict(eager=100)),                                       # 94 ids, W = 2
    "s1000_dying": (1000, 4, dict(eager=100, holes=64, sinks=10)),             # sink 990 = 11 * 90 emits, 991 .. 999 do not
    "s1000_k29": (1000, 29, dict(eager=40)),                                   # 40 ids on 58-byte rows: W = 1 at 1 000 states
}
DYING = tuple(n for n in AUTOMATA if n.endswith("_dying"))
LAYOUT_OF = {"tiny": 1, "lds": 2, "comb": 3, "global": 4, "comb256": 5, "combself": 6, "sparse": 7, "ldsself": 8}
BIG = ("lds", "ldsself", "comb", "combself", "sparse", "global")             # what can hold 1 000 states of 4 classes
# automaton -> the layouts it is asked for (by flag) and gets; every other flag is refused with ENOTSUP
TAKES = {
    "s15": ("tiny",) + BIG,
    "s15_dying": ("tiny", "comb256") + BIG,
    "s200": BIG,
    "s200_dying": BIG,
    "s200_k29": BIG,
    "s1000": BIG,
    "s1000_dying": BIG,
    "s1000_k29": ("lds", "ldsself", "comb", "sparse", "global"),              # 1 001 x 29: no class comb with self-loop masks
}
AUTO = {"s15": "tiny", "s15_dying": "tiny", "s200": "lds", "s200_dying": "lds", "s200_k29": "combself", "s1000": "lds",
        "s1000_dying": "lds", "s1000_k29": "lds"}                             # what the planner picks with no flag
PAIRS = tuple((a, lay) for a in AUTOMATA for lay in TAKES[a])


def words_of(emitted, cols, W):
    """emitted[n][E] bool, cols[b] = the column of bit b -> [n][W] uint64, bit b of a row = emitted[row][cols[b]]"""
    bits = np.zeros((emitted.shape[0], W * 64), np.uint8)
    bits[:, :len(cols)] = emitted[:, cols]
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(emitted.shape[0], W)


@functools.lru_cache(maxsize=None)
def inputs(dying):
    """the rows every test walks, their lengths for the variable-length fronts (zero-length inputs at tile boundaries); the
    dying cases get three hand-made tiles: every row DEAD after byte 0, such rows alternating with live ones, one live row at
    lane 63 (all of them at least one byte long)"""
    rows = np.random.RandomState(4099).randint(0, 256, (N, L)).astype(np.uint8)
    lens = G.varlens(N, L, np.random.RandomState(7))
    lens[list(EMPTY_ROWS)] = 0
    if dying:
        t = np.arange(64)
        for tile, dead in ((TILE_ALL_DEAD, t >= 0), (TILE_ALTERNATE, t % 2 == 0), (TILE_LANE63, t != 63)):
            r = tile * 64 + t
            rows[r[dead], 0] = 0xFF
            rows[r[~dead], 0] = 0x00
            lens[r] = np.maximum(lens[r], 1)
    rows.setflags(write=False)
    lens.setflags(write=False)
    return rows, lens


class Ref:
    """the reference's answers for one walk: end states as the fronts report them, carried states, emitted[n][E]"""

    def __init__(self, c, rows, lens=None, state_in=None):
        self.st, self.em = G.walk_eager(c.dense, c.cls, 0, rows, c.E, lens, state_in, every=c.every)
        self.end = G.ends(c.flat, self.st)
        self.carried = G.carried(self.st)
        self.words = c.words(self.em)
        for a in (self.st, self.em, self.end, self.carried, self.words):
            a.setflags(write=False)


class Piece(Ref):
    """a later piece of a resumed walk, from the states an earlier piece carried.  Over the whole stream the set is defined (what
    fsm_exec's callback receives over the concatenation) and .words is this piece's share of it by fsm_exec's rule, under which a
    byte that keeps the state it was handed enters it again.  The header leaves that one case open for a piece taken alone ("that
    state's outputs do NOT fire again (they fired when it was entered)", "re-entering a state adds nothing"): sets of the piece's
    own must hold .changed (the outputs of every state entered by a step that changes the state) and nothing outside .words."""

    def __init__(self, c, rows, lens, state_in):
        Ref.__init__(self, c, rows, lens, state_in)
        tr = G.trace(c.dense, c.cls, 0, rows, lens, state_in)
        n, L1 = tr.shape
        lens = np.full(n, L1 - 1, np.int64) if lens is None else np.asarray(lens, np.int64)
        ek = np.vstack([G.eager_ids_of_states(c.S, c.E, c.every), [[-1, -1]]])
        em = np.zeros((n, c.E + 1), bool)
        ar = np.arange(n)
        for t in range(1, L1):
            moved = (t <= lens) & (tr[:, t] != tr[:, t - 1])
            for j in (0, 1):
                em[ar[moved], ek[tr[moved, t], j]] = True
        self.changed = c.words(em[:, :c.E])
        assert not (self.changed & ~self.words).any()
        self.changed.setflags(write=False)

    def holds(self, got):
        """rows of got[n][W] outside the two bounds"""
        got = np.asarray(got, np.uint64).reshape(-1, self.words.shape[1])
        k = len(got)
        return np.nonzero(((self.changed[:k] & ~got) | (got & ~self.words[:k])).any(axis=1))[0]


class Case:
    """one automaton and the reference's answers on inputs(), computed once and left as they are"""

    def __init__(self, name):
        self.name = name
        self.S, self.K, self.kw = AUTOMATA[name]
        self.dying = name in DYING
        self.E, self.every = self.kw["eager"], self.kw.get("every", 11)
        self.sinks = self.kw.get("sinks", 0)
        self.flat, self.dense, self.cls = G.affine(self.S, self.K, **self.kw)
        ek = G.eager_ids_of_states(self.S, self.E, self.every)
        self.emitting = (ek >= 0).any(axis=1)
        self.cols = np.unique(ek[ek >= 0])                 # ids ascend with their index: bit b is column cols[b]
        self.ids = (5 + 3 * self.cols).astype(np.uint32)
        self.W = (len(self.cols) + 63) // 64
        self.start_cols = ek[0][ek[0] >= 0]
        # the planner's numbering: emitting states that are not absorbing first, emitting absorbing ones last but for DEAD
        sink = np.arange(self.S) >= self.S - self.sinks
        self.lo_end = int((self.emitting & ~sink).sum())
        self.hi_begin = self.S - int((self.emitting & sink).sum())
        self.abs_min = self.S - self.sinks

    def words(self, emitted):
        return words_of(emitted, self.cols, self.W)

    @functools.cached_property
    def all(self):
        return Ref(self, inputs(self.dying)[0])

    @functools.cached_property
    def len(self):
        return Ref(self, *inputs(self.dying))

    @functools.cached_property
    def first(self):
        return Ref(self, inputs(self.dying)[0][:, :HALF])

    @functools.cached_property
    def second(self):
        """the second half alone, from the state the first half carried: what a resumed piece adds to the sets"""
        r = Piece(self, inputs(self.dying)[0][:, HALF:], None, self.first.st)
        assert np.array_equal(r.st, self.all.st) and np.array_equal(self.first.em | r.em, self.all.em)
        return r

    @functools.cached_property
    def packed(self):
        return G.packed(*inputs(self.dying))


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


# ---- the lane-refill batch: many short packed lines, every wavefront owns at least three tiles ---------------------------

REFILL_L = 160


@functools.lru_cache(maxsize=None)
def refill_inputs(n):
    """n lines of 0 to 160 bytes as rows + lengths, and the byte every line is cut at for the resumed form (0 for every 7th
    line: an empty first piece, which carries the start state's own id); every 5th line begins with 0xFF"""
    rng = np.random.RandomState(n)
    rows = rng.randint(0, 256, (n, REFILL_L)).astype(np.uint8)
    rows[::5, 0] = 0xFF                       # (the dying automata: DEAD after byte 0, so a first piece that ends DEAD)
    lens = rng.randint(0, REFILL_L + 1, n).astype(np.uint32)
    cut = (rng.randint(0, REFILL_L + 1, n) % (lens + 1)).astype(np.uint32)
    cut[::7] = 0
    for a in (rows, lens, cut):
        a.setflags(write=False)
    return rows, lens, cut


class Refill:
    def __init__(self, name, n):
        c = self.c = case(name)
        rows, lens, cut = refill_inputs(n)
        self.whole = Ref(c, rows, lens)
        self.first = Ref(c, rows, cut)
        rest = np.zeros_like(rows)
        m = np.arange(REFILL_L)[None, :] < (lens - cut)[:, None]
        rest[m] = rows[(np.arange(REFILL_L)[None, :] >= cut[:, None]) & (np.arange(REFILL_L)[None, :] < lens[:, None])]
        self.rest_rows, self.rest_lens = rest, (lens - cut).astype(np.uint32)
        self.second = Piece(c, rest, self.rest_lens, self.first.st)
        assert np.array_equal(self.second.st, self.whole.st) and np.array_equal(self.first.em | self.second.em, self.whole.em)
        self.packed = G.packed(rows, lens)
        self.packed_first = G.packed(rows, cut)
        self.packed_rest = G.packed(rest, self.rest_lens)


@functools.lru_cache(maxsize=None)
def refill(name, n):
    return Refill(name, n)
