"""The judge of the tokeniser (include/fsm_hip.h, "tokens"): the definition restated in plain Python / numpy over the
automaton's own dense[S][K], cls[256] and is_end, with the ids from a formula (global_ref.endids_of) or from the caller.
Nothing here goes through the library's planner, its tables or its kernels; from the library only the description's container
(FlatDfa) is used.

An automaton is (flat, dense[S][K] int64 with -1 = no edge, cls[256]) as global_ref.affine returns it; start = flat.start.
A state is absorbing when every byte leads back to it."""
import numpy as np

from global_ref import endids_of

NO_POS = 0xFFFFFFFFFFFFFFFF
NO_MATCH = 0xFFFFFFFF
NO_ID = 0xFFFFFFFE
NO_BACKTRACK, SKIP_BAD = 1, 2
EARLIEST, RET, ERROR = 1, 2, 3


def id_sets(auto, sets=None):
    """per state its ascending end-ids (None for a state that is no end state); sets: {state: ids} instead of the formula"""
    flat = auto[0]
    out = []
    for s in range(flat.nstates):
        if not flat.is_end[s]:
            out.append(None)
        elif sets is not None:
            out.append(tuple(sorted(set(int(x) for x in sets.get(s, ())))))
        else:
            out.append(tuple(int(x) for x in endids_of(flat, s)) if int(flat.endid_off[-1]) else ())
    return out


def state_ids(auto, mode, sets=None):
    """id(q) for every state q (NO_MATCH where q is no end state): EARLIEST the lowest id, NO_ID without one; RET the index of
    the id set among the distinct sets of the end states, ordered by count, then by their bytes as u32 little-endian arrays"""
    per = id_sets(auto, sets)
    if mode == RET:
        order = sorted({x for x in per if x is not None}, key=lambda x: (len(x), np.array(x, "<u4").tobytes()))
        index = {x: k for k, x in enumerate(order)}
        return np.array([NO_MATCH if x is None else index[x] for x in per], np.int64)
    return np.array([NO_MATCH if x is None else (x[0] if x else NO_ID) for x in per], np.int64)


def conflict(auto, sets=None):
    """some end state carries more than one id"""
    return any(x is not None and len(x) > 1 for x in id_sets(auto, sets))


class Judge:
    """tokens of lines under both rules and both modes; the walks from a cursor are remembered, so the four combinations of
    one automaton over the same lines share them"""

    def __init__(self, auto, rows, lens):
        flat, dense, cls = auto
        self.dense = np.asarray(dense, np.int64)
        self.cls = np.asarray(cls, np.int64)
        self.start = int(flat.start)
        self.is_end = np.asarray(flat.is_end).astype(bool)
        S = self.dense.shape[0]
        used = np.unique(self.cls)
        self.absorbing = (self.dense[:, used] == np.arange(S)[:, None]).all(axis=1)
        self.rows = np.asarray(rows, np.uint8)
        self.lens = np.asarray(lens, np.int64)
        self.crow = self.cls[self.rows] if self.rows.size else np.zeros(self.rows.shape, np.int64)
        self.tab = [list(map(int, r)) for r in self.dense]     # plain lists: the inner loop is Python
        self.memo = {}

    def walk(self, i, p):
        """from cursor p of line i -> (stop, state at stop, e, q, walked): e the largest position in (p, len] with an end
        state (0: none) and q the state there; walked: the bytes looked at, the one with the missing edge included"""
        key = (i, p)
        got = self.memo.get(key)
        if got is not None:
            return got
        L = int(self.lens[i])
        c = self.crow[i]
        s, k, e, q, walked = self.start, p, 0, -1, 0
        while k < L:
            walked += 1
            nx = self.tab[s][int(c[k])]
            if nx < 0:
                break                         # DEAD: the byte is not consumed
            s = nx
            k += 1
            if self.is_end[s]:
                e, q = k, s
            if self.absorbing[s]:
                if self.is_end[s]:
                    e = L                     # it accepts at every later position
                break
        got = (k, s, e, q, walked)
        self.memo[key] = got
        return got

    def line(self, i, flags):
        """-> ([(end, state)], err, [overrun of every real token], bytes walked)"""
        L = int(self.lens[i])
        p, toks, err, over, walked_all = 0, [], NO_POS, [], 0
        while p < L:
            stop, s_stop, e, q, walked = self.walk(i, p)
            walked_all += walked
            if flags & NO_BACKTRACK:
                e, q = (stop, s_stop) if stop > p and self.is_end[s_stop] else (0, -1)
            if e:
                toks.append((e, q))
                over.append(p + walked - e if e <= p + walked else 0)
                p = e
                continue
            if err == NO_POS:
                err = p
            if not flags & SKIP_BAD:
                break
            toks.append((p + 1, -1))
            p += 1
        return toks, err, over, walked_all

    def run(self, flags, ids, n=None):
        """all lines (the first n) -> dict(off u64 [n + 1], end u64 [total], id u32 [total], err u64 [n], state int64 [total]
        (-1: a bad byte), overrun int64 [real tokens], length int64 [total], walked int)"""
        n = len(self.lens) if n is None else n
        off, end, state, err, over, length, walked = [0], [], [], [], [], [], 0
        for i in range(n):
            toks, e, ov, w = self.line(i, flags)
            end += [t[0] for t in toks]
            length += [t[0] - (toks[k - 1][0] if k else 0) for k, t in enumerate(toks)]
            state += [t[1] for t in toks]
            off.append(len(end))
            err.append(e)
            over += ov
            walked += w
        state = np.array(state, np.int64)
        off = np.array(off, np.uint64)
        end = np.array(end, np.uint64)
        ids = np.asarray(ids, np.int64)
        idv = np.where(state < 0, NO_MATCH, ids[np.maximum(state, 0)]).astype(np.uint32) if len(state) else np.zeros(0, np.uint32)
        return dict(off=off, end=end, id=idv, err=np.array(err, np.uint64), state=state, overrun=np.array(over, np.int64),
                    length=np.array(length, np.int64),
                    walked=walked)


def select(res, pick):
    """the result for inputs pick[j] of a result over all lines: (off, end, id, err)"""
    off, end, idv, err = res["off"].astype(np.int64), res["end"], res["id"], res["err"]
    pick = np.asarray(pick, np.int64)
    cnt = off[pick + 1] - off[pick] if len(pick) else np.zeros(0, np.int64)
    o = np.zeros(len(pick) + 1, np.uint64)
    o[1:] = np.cumsum(cnt)
    idx = np.concatenate([np.arange(off[i], off[i + 1]) for i in pick]).astype(np.int64) if len(pick) else np.zeros(0, np.int64)
    return o, end[idx], idv[idx], err[pick] if len(pick) else np.zeros(0, np.uint64)


def trie_lexer(words):
    """a trie with DEAD on every missing edge and the word's index as its end-id: (auto, {state: [index]})"""
    from libfsm_amd import FlatDfa
    nxt, ids = [dict()], {}
    for w_i, w in enumerate(words):
        s = 0
        for b in w:
            if b not in nxt[s]:
                nxt[s][b] = len(nxt)
                nxt.append(dict())
            s = nxt[s][b]
        ids[s] = [w_i]
    dense = np.full((len(nxt), 256), -1, np.int64)
    for s, d in enumerate(nxt):
        for b, t in d.items():
            dense[s, b] = t
    is_end = np.zeros(len(nxt), np.uint8)
    is_end[list(ids)] = 1
    flat = FlatDfa.from_dense(dense, 0, is_end, endids=ids)
    return (flat, dense, np.arange(256, dtype=np.int64)), ids
