"""The judge of the accept-position walks and of the spans (include/fsm_hip.h, "match positions"): plain numpy over
global_ref.trace() and the description's own is_end.  Nothing here goes through the library's planner, its tables or its
kernels; from the library only the description's container (FlatDfa) is used.

An automaton is (flat, dense[S][K] int64 with -1 = no edge, cls[256]) as global_ref.affine returns it; start = flat.start.
A backward walk is trace() over the reversed range.

Also here: a Python Aho-Corasick builder (outputs propagated along failure links) that yields such automata for a set of
words -- `starts` (anything, then a reversed word), `ends` (exactly a word), the line matcher (.*(w).*) -- and the brute-force
leftmost-longest matcher they are held against.  (FlatDfa.from_strings is not used: see NOTES.md, "from_strings and words inside
prefixes".)"""
import numpy as np

from global_ref import trace
from libfsm_amd import FlatDfa

NO_POS = 0xFFFFFFFFFFFFFFFF


def rows_of(lines):
    """list of bytes -> (rows[n][L] uint8 zero padded, L >= 1, lens int64)"""
    lens = np.array([len(x) for x in lines], np.int64)
    rows = np.zeros((len(lines), max(int(lens.max()) if len(lines) else 0, 1)), np.uint8)
    for i, x in enumerate(lines):
        rows[i, :len(x)] = np.frombuffer(x, np.uint8)
    return rows, lens


def accept_pos(auto, rows, lens, frm=None, to=None, back=False, detail=False):
    """-> (first, last) u64 [n]: the definition.  rows[n][L], lens: the (already trimmed) lengths; frm / to: u64 [n] or None.
    detail: also the state every walked input stopped in (-1 DEAD; -2 not walked)."""
    flat, dense, cls = auto
    rows = np.asarray(rows, np.uint8)
    if rows.shape[1] == 0:
        rows = np.zeros((rows.shape[0], 1), np.uint8)
    n, L = rows.shape
    lens = np.asarray(lens, np.int64)
    is_end = np.asarray(flat.is_end).astype(bool)
    hi = lens.copy() if to is None else np.minimum(np.asarray(to, np.uint64), lens.astype(np.uint64)).astype(np.int64)
    f = np.zeros(n, np.uint64) if frm is None else np.asarray(frm, np.uint64)
    walked = f <= hi.astype(np.uint64)
    lo = np.where(walked, f, 0).astype(np.int64)
    total = np.where(walked, hi - lo, 0)
    c = np.arange(L, dtype=np.int64)[None, :]
    src = (hi[:, None] - 1 - c) if back else (lo[:, None] + c)
    sub = rows[np.arange(n)[:, None], np.clip(src, 0, L - 1)]
    tr = trace(dense, cls, flat.start, sub, total)                      # [n][L + 1]; beyond total the state stays
    k = np.arange(L + 1, dtype=np.int64)[None, :]
    A = (tr >= 0) & is_end[np.maximum(tr, 0)] & (k <= total[:, None]) & walked[:, None]
    some = A.any(axis=1)
    c_first, c_last = A.argmax(axis=1), L - A[:, ::-1].argmax(axis=1)
    pos = (lambda cc: hi - cc) if back else (lambda cc: lo + cc)
    first = np.where(some, pos(c_first), 0).astype(np.uint64)
    last = np.where(some, pos(c_last), 0).astype(np.uint64)
    first[~some] = NO_POS
    last[~some] = NO_POS
    if detail:
        return first, last, np.where(walked, tr[np.arange(n), total], -2)
    return first, last


def spans_rounds(starts, ends, rows, lens, max_rounds=10000):
    """the composed definition, round by round until no input has a span: [(start, end)] u64 [n] each, the last round (all
    NO_POS) included"""
    n = len(lens)
    p = np.zeros(n, np.uint64)
    out = []
    for _ in range(max_rounds):
        _, st = accept_pos(starts, rows, lens, frm=p, back=True)
        _, en = accept_pos(ends, rows, lens, frm=st)
        st = np.where(en == NO_POS, np.uint64(NO_POS), st)
        out.append((st, en))
        if not (st != NO_POS).any():
            return out
        with np.errstate(over="ignore"):
            p = np.where(st == NO_POS, np.uint64(NO_POS), np.where(en > st, en, en + np.uint64(1)))
    raise AssertionError("the rounds do not end")


def leftmost_longest(words, line):
    """brute force: the non-overlapping leftmost-longest matches of a set of non-empty words in line, [(start, end)]"""
    out, p = [], 0
    while p <= len(line):
        best = None
        for q in range(p, len(line) + 1):
            fit = [len(w) for w in words if line[q:q + len(w)] == w]
            if fit:
                best = (q, q + max(fit))
                break
        if best is None:
            break
        out.append(best)
        p = best[1] if best[1] > best[0] else best[1] + 1
    return out


# ---- Aho-Corasick, in Python ----------------------------------------------------------------------------------------

def _trie(words):
    nxt, out = [dict()], [False]
    for w in words:
        s = 0
        for b in w:
            if b not in nxt[s]:
                nxt[s][b] = len(nxt)
                nxt.append(dict())
                out.append(False)
            s = nxt[s][b]
        out[s] = True
    return nxt, out


def _auto(dense, is_end):
    dense = np.asarray(dense, np.int64)
    flat = FlatDfa.from_dense(dense, 0, np.asarray(is_end, np.uint8))
    return flat, dense, np.arange(256, dtype=np.int64)


def ac_goto(words):
    """the full goto function of the Aho-Corasick automaton of `words`: (dense[S][256], out[S]) -- out[s]: some word is a
    suffix of what has been read (outputs propagated along failure links)"""
    nxt, out = _trie(words)
    S = len(nxt)
    dense = np.zeros((S, 256), np.int64)
    fail = [0] * S
    queue = []
    for b in range(256):
        t = nxt[0].get(b)
        if t is not None:
            dense[0, b] = t
            queue.append(t)
    while queue:
        s = queue.pop(0)
        out[s] = out[s] or out[fail[s]]
        for b in range(256):
            t = nxt[s].get(b)
            if t is None:
                dense[s, b] = dense[fail[s], b]
            else:
                dense[s, b] = t
                fail[t] = int(dense[fail[s], b])
                queue.append(t)
    return dense, np.array(out, bool)


def starts_of(words):
    """accepts anything followed by a reversed word: walked backward from a line's end, it is in an end state at q iff a word
    begins at q"""
    dense, out = ac_goto([w[::-1] for w in words])
    return _auto(dense, out)


def ends_of(words, empty=False):
    """accepts exactly the words (a missing edge is DEAD); empty: the empty string as well"""
    nxt, out = _trie(words)
    dense = np.full((len(nxt), 256), -1, np.int64)
    for s, d in enumerate(nxt):
        for b, t in d.items():
            dense[s, b] = t
    out[0] = out[0] or empty
    return _auto(dense, out)


def line_matcher_of(words):
    """.*(w).*: the Aho-Corasick automaton with every end state absorbing"""
    dense, out = ac_goto(words)
    dense[out, :] = np.flatnonzero(out)[:, None]
    return _auto(dense, out)


def start_accepting_of(auto):
    """the same automaton with the start state an end state too"""
    flat, dense, cls = auto
    is_end = np.asarray(flat.is_end).copy()
    is_end[flat.start] = 1
    return with_is_end(auto, is_end)


def everywhere_of(auto):
    """the same automaton with every state an end state: it accepts at every position"""
    return with_is_end(auto, np.ones(auto[0].nstates, np.uint8))


def with_is_end(auto, is_end):
    flat, dense, cls = auto
    f2 = FlatDfa(flat.nstates, flat.start, flat.edge_off, flat.ranges, np.asarray(is_end, np.uint8), np.zeros(flat.nstates + 1, np.uint32),
                 np.zeros(0, np.uint32))
    return f2, dense, cls
