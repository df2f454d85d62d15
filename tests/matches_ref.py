"""The judge of the matches (include/fsm_hip.h, "matches"): the definition restated in plain Python / numpy over the two
automata's own dense[S][K], cls[256] and is_end.  Nothing here goes through the library's planner, its tables or its kernels,
and nothing through the rounds of span_ref.spans_rounds either (tests/test_matches_abi.py holds the two against each other).

An automaton is (flat, dense[S][K] int64 with -1 = no edge, cls[256]) as global_ref.affine returns it; start = flat.start.
Neither walk needs to know which states are absorbing: a walk that goes on in an absorbing state stays in it, so "every smaller
s has M(s)" and "end = len" are what walking on gives."""
import numpy as np

NO_MATCH = 0xFFFFFFFF
DROP_EMPTY = 1


def _table(auto):
    """(tab[S + 1][K] with DEAD = S as a state of its own, is_end[S + 1], cls, start)"""
    flat, dense, cls = auto
    dense = np.asarray(dense, np.int64)
    S, K = dense.shape
    tab = np.vstack([np.where(dense < 0, S, dense), np.full((1, K), S, np.int64)])
    is_end = np.append(np.asarray(flat.is_end).astype(bool), False)
    return tab, is_end, np.asarray(cls, np.int64), int(flat.start)


def _rows(rows):
    rows = np.asarray(rows, np.uint8)
    if rows.ndim != 2 or rows.shape[1] == 0:
        rows = np.zeros((rows.shape[0], 1), np.uint8)
    return rows


def marks(starts, rows, lens):
    """M[n][L + 1] bool: M[i][s] for s in 0 .. len_i (False beyond): the state of `starts` after bytes len - 1 down to s, from
    its start state, is an end state; s = len is the start state before any byte"""
    tab, is_end, cls, start = _table(starts)
    rows = _rows(rows)
    n, L = rows.shape
    lens = np.asarray(lens, np.int64)
    crow = cls[rows]
    M = np.zeros((n, L + 1), bool)
    st = np.full(n, start, np.int64)
    idx = np.arange(n)
    M[idx, lens] = is_end[st]
    for t in range(L):
        s = lens - 1 - t                            # the byte walked now, and the position reached
        ok = s >= 0
        if not ok.any():
            break
        st = np.where(ok, tab[st, crow[idx, np.maximum(s, 0)]], st)
        M[idx[ok], s[ok]] = is_end[st[ok]]
    return M


def longest_from(ends, rows, lens):
    """(E[n][L + 1], Q[n][L + 1]) int64: for every start s in 0 .. len_i, E the largest e in [s, len] at which `ends`, walked
    from its start state over bytes s, s + 1, ..., is in an end state (-1: none; DEAD is sticky), Q the state there"""
    tab, is_end, cls, start = _table(ends)
    rows = _rows(rows)
    n, L = rows.shape
    lens = np.asarray(lens, np.int64)
    crow = cls[rows]
    pos = np.broadcast_to(np.arange(L + 1, dtype=np.int64)[None, :], (n, L + 1))
    st = np.full((n, L + 1), start, np.int64)
    hit = (pos <= lens[:, None]) & is_end[st]
    E = np.where(hit, pos, -1)
    Q = np.where(hit, st, -1)
    line = np.arange(n)[:, None]
    for t in range(L):
        at = pos + t                                # the byte the walk from s takes now
        ok = at < lens[:, None]
        if not ok.any():
            break
        st = np.where(ok, tab[st, crow[line, np.minimum(at, L - 1)]], st)
        hit = ok & is_end[st]
        E = np.where(hit, at + 1, E)
        Q = np.where(hit, st, Q)
    return E, Q


def line_matches(M_i, E_i, Q_i, L, flags=0):
    """the cursor loop of the definition for one line: [(start, end, state at end)]"""
    marked = np.flatnonzero(M_i[:L + 1])
    out, p = [], 0
    while p <= L:
        k = int(np.searchsorted(marked, p))
        if k == len(marked):
            break                                   # 1. no marked position at or after p
        s = int(marked[k])
        e = int(E_i[s])
        if e < 0:
            break                                   # 4. a hit without a span stays without one
        if not (flags & DROP_EMPTY and e == s):
            out.append((s, e, int(Q_i[s])))
        p = e if e > s else e + 1
    return out


def matches(starts, ends, rows, lens, flags=0, ids=None, tables=None):
    """all lines -> dict(off u64 [n + 1], start u64 [total], end u64 [total], state int64 [total], id u32 [total] (ids: the id of
    every state of `ends`, e.g. tokens_ref.state_ids; without: NO_MATCH)); tables: (M, E, Q) computed before"""
    lens = np.asarray(lens, np.int64)
    M, E, Q = tables if tables is not None else (marks(starts, rows, lens),) + longest_from(ends, rows, lens)
    off, start, end, state = [0], [], [], []
    for i in range(len(lens)):
        for s, e, q in line_matches(M[i], E[i], Q[i], int(lens[i]), flags):
            start.append(s)
            end.append(e)
            state.append(q)
        off.append(len(start))
    state = np.array(state, np.int64)
    idv = np.full(len(state), NO_MATCH, np.uint32) if ids is None else np.asarray(ids, np.int64)[state].astype(np.uint32)
    return dict(off=np.array(off, np.uint64), start=np.array(start, np.uint64), end=np.array(end, np.uint64), state=state, id=idv)


def select(res, pick, nlines=None):
    """the result for inputs pick[j] of a result over all lines: (off, start, end, id); a pick[j] >= nlines has no match"""
    off = res["off"].astype(np.int64)
    nlines = len(off) - 1 if nlines is None else nlines
    idx, o = [], [0]
    for i in pick:
        i = int(i)
        if i < nlines:
            idx.append(np.arange(off[i], off[i + 1]))
        o.append(o[-1] + (int(off[i + 1] - off[i]) if i < nlines else 0))
    idx = np.concatenate(idx).astype(np.int64) if idx else np.zeros(0, np.int64)
    return np.array(o, np.uint64), res["start"][idx], res["end"][idx], res["id"][idx]


def head(res, n):
    """the result for the first n inputs: (off, start, end, id)"""
    total = int(res["off"][n])
    return res["off"][:n + 1], res["start"][:total], res["end"][:total], res["id"][:total]
