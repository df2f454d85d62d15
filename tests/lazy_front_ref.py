"""The automata, inputs and reference answers of tests/test_gpu_lazy_front.py and tests/test_lazy_front_cases.py: the lazy
walks of the sparse layout (walk_lazy, walk_lazy_lines: walk_lazy.h) on absorbing and non-trie automata, at line edges.

Every answer is a plain numpy walk of FlatDfa.dense() in the caller's numbering with the identity byte map
(global_ref.trace / ends / carried): nothing here goes through the planner, a layout, a knob or a front.  States are the
caller's; -1 is DEAD (a missing edge was taken; sticky).

Automata (all below 20 000 states):
  trie_ids       literal set with end-ids, anchored right: no absorbing state is reachable (the control: ABS = false)
  abs_accept16   unanchored literal sets WITHOUT end-ids: the accept state is absorbing, and reachable (ABS = true);
  abs_accept64   what a caller gets for a re_strings-style set on lines; both meet fsm_hip's auto-lazy rule
  rewired_a      literal sets whose dense table has a share of its transitions redirected to random states (3 % / 0.2 %) and a
  rewired_b      smaller share removed, plus single missing edges: no longer tries (states entered with two carried records,
                 exceptions that are no progression, DEAD reachable).  rewired_b carries end-ids (from_dense).  The states
                 within two bytes of the start state keep their rows, or the planner makes no lazy image.
Lines, per automaton (one pool, the reference walked over it once):
  hand    lines of HAND_LENS bytes in which the byte that makes the line absorbing sits at a chosen index (or nowhere), built
          by walking the reference; behind it text that would change the answer if walked from a live state
  shape   all-tail lines (0-15 bytes), lines without a tail (multiples of 16), 16k - 1 / 16k / 16k + 1 bytes
  random  0-160 bytes, every third line with a word planted; 2 % foreign bytes on the trie
A batch of n lines takes lines of the shuffled pool, puts empty lines at indexes 0, 191, 192, 255, 256 and makes its last line
one whose tail of 1, 7 or 15 bytes ends at the text's last byte (or an empty one)."""
import functools

import numpy as np

import global_ref as G
from libfsm_amd import FlatDfa

NO = 0xFFFFFFFF
NO_ID = 0xFFFFFFFE
IDENT = np.arange(256, dtype=np.int64)
WIDTH = 304                                  # the pool's row width: the longest hand-made line is 300 bytes
HAND_LENS = (16, 17, 31, 32, 47, 48, 49, 64, 96, 97, 145, 300)
HAND_AT = (0, 15, 16, 17, 31, 32, 47, 48)    # ... and len - 1, len - len % 16 (the tail's first byte), nowhere (None)
SIZES = (1, 63, 64, 65, 191, 192, 193, 255, 256, 257, 511, 513)
EMPTY_AT = (0, 191, 192, 255, 256)
TAILS = (0, 1, 7, 15)                        # bytes the batch's last line leaves in the text's last 16 (0: an empty last line)
NRANDOM = 1800
CUTS = ("random", 16, 32, 48, 0)

A8, A16 = b"abcdefgh", b"abcdefghijklmnop"
A64 = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_-"
# name -> how it is made, and what tests/test_lazy_front_cases.py holds the planner to (abs_reach: lazy_img[11]; auto: fsm_hip's
# auto-lazy rule, (nz + nsent) * 10 <= abs_min - H)
SPEC = {
    "trie_ids": dict(alpha=A8, nwords=3000, lo=4, hi=10, flags=2, seed=8 * 13 + 3000, ids=True, abs_reach=0, auto=True),
    "abs_accept16": dict(alpha=A16, nwords=2000, lo=5, hi=9, flags=0, seed=16, ids=False, abs_reach=1, auto=True),
    "abs_accept64": dict(alpha=A64, nwords=5000, lo=4, hi=8, flags=0, seed=66, ids=False, abs_reach=1, auto=True),
    "rewired_a": dict(alpha=A8, nwords=3000, lo=4, hi=10, flags=2, seed=104, ids=False, abs_reach=1, auto=False, rewire=0.03, remove=0.006),
    "rewired_b": dict(alpha=A8, nwords=3000, lo=4, hi=10, flags=2, seed=108, ids=True, abs_reach=1, auto=False, rewire=0.002, remove=0.008),
}
START_HOLE = 0x7A          # 'z': the rewired pair's start state has no edge on it -- a line can be DEAD after byte 0.  (A byte of a class without
                           # a bit: the exact path.  A hole on a letter of the alphabet in the start state's row leaves no lazy image.)
NAMES = tuple(SPEC)
ABSORBING = tuple(n for n in NAMES if SPEC[n]["abs_reach"])
REWIRED = ("rewired_a", "rewired_b")
WITH_IDS = tuple(n for n in NAMES if SPEC[n]["ids"])


def rewired_ids(s):
    """the end-ids rewired_b gives end state s: two per state, one of them above 255, few distinct sets"""
    return [s % 7, 300 + s % 3]


def walk1(dense, s, data):
    """the states after each byte of one line, from state s (-1: DEAD)"""
    out = []
    for b in data:
        s = int(dense[s, b]) if s >= 0 else -1
        out.append(s)
    return out


class Case:
    def __init__(self, name):
        self.name = name
        sp = self.spec = SPEC[name]
        rng = np.random.RandomState(sp["seed"])
        self.alpha = alpha = np.frombuffer(sp["alpha"], np.uint8)
        self.words = sorted(set(bytes(alpha[rng.randint(0, len(alpha), rng.randint(sp["lo"], sp["hi"] + 1))]) for _ in range(sp["nwords"])))
        ac = FlatDfa.from_strings(self.words, sp["flags"], list(range(len(self.words))) if sp["ids"] or "rewire" in sp else None)
        self.idsets = None
        if "rewire" in sp:
            nt = ac.dense().astype(np.int64)
            nt[nt == NO] = -1
            S = ac.nstates
            # the states within two bytes of the start state keep their rows: whether the planner makes a lazy image at all hangs on
            # them (its LDS set is a breadth-first prefix whose exceptions lead to consecutive ids: plan.cpp build_lazy)
            depth = np.full(S, 99, np.int64)
            depth[ac.start] = 0
            for d in (1, 2):
                t = nt[depth == d - 1][:, alpha].ravel()
                depth[t[(t >= 0) & (depth[np.maximum(t, 0)] > d)]] = d
            deep = depth > 2
            k = int(S * len(alpha) * sp["rewire"])
            ss, cc = rng.randint(0, S, k), alpha[rng.randint(0, len(alpha), k)]
            to = rng.randint(0, S, k)
            nt[ss[deep[ss]], cc[deep[ss]]] = to[deep[ss]]
            k = int(S * len(alpha) * sp["remove"])
            ss, cc = rng.randint(0, S, k), alpha[rng.randint(0, len(alpha), k)]
            nt[ss[deep[ss]], cc[deep[ss]]] = -1
            nt[ac.start, START_HOLE] = -1                            # single missing edges: the start state's on a foreign byte, ...
            for s in np.nonzero(deep)[0][rng.randint(0, int(deep.sum()), 8)]:      # ... and eight states' on the alphabet's first letter
                nt[s, alpha[0]] = -1
            if sp["ids"]:
                self.idsets = {s: rewired_ids(s) for s in np.nonzero(ac.is_end)[0].tolist()}
            self.flat = FlatDfa.from_dense(nt, ac.start, ac.is_end, self.idsets)
            self.dense = nt
        else:
            self.flat = ac
            self.dense = ac.dense().astype(np.int64)
            self.dense[self.dense == NO] = -1
        self.dense.setflags(write=False)
        self.S, self.start = self.flat.nstates, self.flat.start
        self.is_end = self.flat.is_end.astype(bool)
        self.absorbing = (self.dense == np.arange(self.S)[:, None]).all(axis=1)      # every byte keeps the state
        self.has_abs = bool(sp["abs_reach"])
        self._lines(np.random.RandomState(sp["seed"] + 1000))

    # ---- text ----------------------------------------------------------------------------------------------------------------
    def text(self, rng, n, plant=False, foreign=0.0):
        """n bytes over the alphabet; plant: a word at the end (the sets anchored right: every other time) or at a random place"""
        b = self.alpha[rng.randint(0, len(self.alpha), n)]
        if foreign > 0 and n:
            m = rng.rand(n) < foreign
            b[m] = rng.randint(0, 256, int(m.sum())).astype(np.uint8)
        if plant:
            w = self.words[rng.randint(len(self.words))]
            if len(w) <= n:
                at = n - len(w) if (self.spec["flags"] & 2 and rng.rand() < 0.5) else int(rng.randint(0, n - len(w) + 1))
                b[at:at + len(w)] = np.frombuffer(w, np.uint8)
        return bytes(b)

    def first_absorbing(self, data, s=None):
        """the index of the byte after which the line is in an absorbing state or DEAD, None if it never is"""
        for t, s in enumerate(walk1(self.dense, self.start if s is None else s, data)):
            if s < 0 or self.absorbing[s]:
                return t
        return None

    def accepts_from_start(self, data):
        st = walk1(self.dense, self.start, data)
        s = st[-1] if st else self.start
        return s >= 0 and bool(self.is_end[s])

    def _hand_accept(self, rng, ln, k):
        """the last byte of a planted word at index k, no word before it; behind it text that holds no word"""
        for _ in range(400):
            if k is None:
                body = self.text(rng, ln)
            else:
                w = self.words[rng.randint(len(self.words))]
                if len(w) > k + 1:
                    continue
                body = self.text(rng, k + 1 - len(w)) + w + self.text(rng, ln - k - 1)
            if self.first_absorbing(body) == k and (k is None or not self.accepts_from_start(body[k + 1:])):
                return body
        return None

    def _hand_dead(self, rng, ln, k):
        """a byte with no edge from the state reached at index k, none before it; behind it, where there is room, text that ends
        in an end state if walked from the start state (a whole word at its end)"""
        al = self.alpha.tolist()
        if k is not None and not self.can[k][self.start]:
            return None
        for _ in range(400):
            s, body = self.start, []
            for t in range(ln if k is None else k):
                ok = [b for b in al if self.dense[s, b] >= 0 and (self.safe if k is None else self.can[k - t - 1])[self.dense[s, b]]]
                if not ok:
                    break
                body.append(ok[rng.randint(len(ok))])
                s = int(self.dense[s, body[-1]])
            else:
                if k is None:
                    if self.first_absorbing(bytes(body)) is None:
                        return bytes(body)
                    continue
                holes = [b for b in al + [START_HOLE] if self.dense[s, b] < 0]
                rest = self.text(rng, ln - k - 1, plant=True)
                w = self.words[rng.randint(len(self.words))]
                if len(w) <= len(rest):
                    rest = rest[:len(rest) - len(w)] + w
                body = bytes(body) + bytes([holes[rng.randint(len(holes))]]) + rest
                if self.first_absorbing(body) == k and (len(rest) < 10 or self.accepts_from_start(rest)):
                    return body
        return None

    def _lines(self, rng):
        sp = self.spec
        lines, kind, self.hand = [], [], []                  # hand: (pool index, length, index of the absorbing byte or None)
        if self.has_abs:
            if self.name in REWIRED:
                # can[r][s]: a walk of exactly r bytes of the alphabet leads from s, through states that are not absorbing, to one with
                # a missing edge; safe[s]: a walk of any length from s stays clear of DEAD and of absorbing states
                al = self.alpha
                sub = self.dense[:, al]
                hole = (self.dense[:, al.tolist() + [START_HOLE]] < 0).any(axis=1) & ~self.absorbing
                self.can = [hole]
                for _ in range(max(HAND_LENS)):
                    self.can.append(~self.absorbing & ((sub >= 0) & self.can[-1][np.maximum(sub, 0)]).any(axis=1))
                self.safe = ~self.absorbing
                for _ in range(self.S):
                    nxt = self.safe & ((sub >= 0) & self.safe[np.maximum(sub, 0)]).any(axis=1)
                    if (nxt == self.safe).all():
                        break
                    self.safe = nxt
            for ln in HAND_LENS:
                ks = sorted(set(k for k in HAND_AT + (ln - 1,) + ((ln - ln % 16,) if ln % 16 else ()) if k < ln))
                for k in ks + [None]:
                    body = (self._hand_dead if self.name in REWIRED else self._hand_accept)(rng, ln, k)
                    if body is not None:
                        self.hand.append((len(lines), ln, k))
                        lines.append(body)
                        kind.append("hand")
        nshape = len(lines)
        for ln in rng.randint(0, 16, 400).tolist() + (16 * rng.randint(0, 11, 400)).tolist() + [16 * k + d for k in (1, 2, 3, 4) for d in (-1, 0, 1)]:
            lines.append(self.text(rng, ln, plant=len(lines) % 3 == 0))
            kind.append("shape")
        self.shape = (nshape, len(lines))
        for i in range(NRANDOM):
            lines.append(self.text(rng, int(rng.randint(0, 161)), plant=i % 3 == 0, foreign=0.02 if self.name == "trie_ids" else 0.0))
            kind.append("random")
        self.random = (len(lines) - NRANDOM, len(lines))
        self.nfull = len(lines)
        self.EMPTY = len(lines)
        lines.append(b"")
        self.tail_idx = {0: self.EMPTY}
        for t in TAILS[1:]:
            self.tail_idx[t] = len(lines)
            lines.append(self.text(rng, 32 + t, plant=True))
        self.lines = lines
        self.kind = np.array(kind + ["extra"] * (len(lines) - len(kind)))
        self.lens = np.array([len(x) for x in lines], np.uint32)
        self.rows = np.zeros((len(lines), WIDTH), np.uint8)
        for i, x in enumerate(lines):
            self.rows[i, :len(x)] = np.frombuffer(x, np.uint8)
        self.order = np.random.RandomState(sp["seed"] + 2000).permutation(self.nfull)
        self.FULL = self.nfull + len(EMPTY_AT) + 1
        # ---- the reference, once ----
        self.tr = G.trace(self.dense, IDENT, self.start, self.rows, self.lens)      # [pool][WIDTH + 1]
        self.st = self.tr[:, -1].copy()
        self.end = G.ends(self.flat, self.st)
        self.cut = {}
        cr = np.random.RandomState(sp["seed"] + 3000)
        for c in CUTS:
            self.cut[c] = (cr.randint(0, WIDTH + 1, len(lines)) % (self.lens + 1) if c == "random" else np.minimum(c, self.lens)).astype(np.uint32)
        for a in (self.rows, self.lens, self.tr, self.st, self.end, self.order) + tuple(self.cut.values()):
            a.setflags(write=False)

    # ---- batches -------------------------------------------------------------------------------------------------------------
    @functools.lru_cache(maxsize=None)
    def batch(self, n, tail=0):
        """pool indexes of a batch of n lines: the shuffled pool from a place of the batch's own, empty lines at EMPTY_AT, the last
        line one with a tail of `tail` bytes (0: empty).  n = FULL takes every line of the three blocks."""
        src = iter(np.roll(self.order, -7 * n if n != self.FULL else 0).tolist())
        idx = [self.tail_idx[tail] if i == n - 1 else self.EMPTY if i in EMPTY_AT else next(src) for i in range(n)]
        idx = np.array(idx, np.int64)
        idx.setflags(write=False)
        return idx

    def packed(self, idx, lens=None):
        """(bytes, u64 offsets[n + 1]) of the lines idx (their first lens[i] bytes)"""
        return G.packed(self.rows[idx], self.lens[idx] if lens is None else lens)

    def rest(self, idx, cut):
        """rows + lengths of what is left of the lines idx behind their first cut[i] bytes"""
        lens = self.lens[idx] - cut
        col = np.arange(WIDTH)[None, :]
        out = np.zeros((len(idx), WIDTH), np.uint8)
        out[col < lens[:, None]] = self.rows[idx][(col >= cut[:, None]) & (col < self.lens[idx][:, None])]
        return out, lens.astype(np.uint32)

    @functools.lru_cache(maxsize=None)
    def fixed(self, stride):
        """rows of exactly `stride` bytes for the fronts without lengths -- every pool line cut at, or padded with live text to,
        the stride, the hand-made ones first, then the shuffled rest -- and the reference's answers on them: (rows, states, ends)"""
        rng = np.random.RandomState(self.spec["seed"] + 4000 + stride)
        rows = self.alpha[rng.randint(0, len(self.alpha), (self.nfull, stride))]
        col = np.arange(min(stride, WIDTH))[None, :]
        keep = col < self.lens[:self.nfull, None]
        rows[:, :col.shape[1]][keep] = self.rows[:self.nfull, :col.shape[1]][keep]
        if self.name in REWIRED:
            # live text behind a line that is alive at its end: bytes that lead to states from which a walk can stay alive
            sub = self.dense[:, self.alpha]
            ok = (sub >= 0) & self.safe[np.maximum(sub, 0)]
            rank, cnt = np.cumsum(ok, axis=1), ok.sum(axis=1)
            cur = np.full(self.nfull, self.start, np.int64)
            for t in range(stride):
                s_ = np.maximum(cur, 0)
                pick = (rank[s_] > (rng.randint(0, 1 << 30, self.nfull) % np.maximum(cnt[s_], 1))[:, None]).argmax(axis=1)
                pad = (t >= self.lens[:self.nfull]) & (cur >= 0) & (cnt[s_] > 0)
                rows[pad, t] = self.alpha[pick[pad]]
                cur = np.where(cur >= 0, self.dense[s_, rows[:, t]], -1)
        hand = [i for i, _, _ in self.hand]
        rows = rows[np.array(hand + [i for i in self.order.tolist() if self.kind[i] != "hand"], np.int64)]
        st = G.walk(self.dense, IDENT, self.start, rows)
        end = G.ends(self.flat, st)
        for a in (rows, st, end):
            a.setflags(write=False)
        return rows, st, end

    def state_at(self, idx, cut):
        """the reference's state of every line idx after its first cut[i] bytes"""
        return self.tr[idx, cut]

    def ids_of(self, s):
        """the end-ids of end state s, ascending: rewired_b's are rewired_ids(); trie_ids' are the description's own arrays (word i
        carries id i; an end state holds the ids of the words that END in it, not of the shorter words that end the same text --
        tests/test_lazy_front_cases.py holds the arrays to that)"""
        return sorted(self.idsets[s]) if self.idsets is not None else self.flat.endids_of(s).tolist()

    def lowest_id(self, states):
        """FSM_HIP_IDS_EARLIEST of walks that ended in `states`: the lowest id, NO_ID for an end state without one, NO_MATCH"""
        out = np.full(len(states), NO, np.uint32)
        for i, s in enumerate(np.asarray(states, np.int64).tolist()):
            if s >= 0 and self.is_end[s]:
                ids = self.ids_of(s)
                out[i] = ids[0] if ids else NO_ID
        return out


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)
