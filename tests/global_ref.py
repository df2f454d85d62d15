"""Automata of a chosen shape for the global-table walks, and an independent judge for them (plain numpy).

affine(S, K, ...) builds a DFA over K byte classes (contiguous byte ranges) in which class c sends state s to
(a_c * s + b_c) % S, every a_c odd, small and coprime to S: each class is a permutation of the states, so under
uniformly random bytes the walk is (but for holes and sinks) uniformly spread over ALL states whatever its history --
no row order can keep such a walk in the part of a table that fits LDS.  Its transition function is a closed formula,
kept beside the flat description as dense[S][K], and walk() / walk_eager() below apply it byte by byte: nothing here
goes through the library's planner, its tables or its kernels.  From the library only the description's containers
(FlatDfa, RANGE_DTYPE) are used.

States are the caller's (original) numbering throughout; -1 is DEAD (a missing edge was taken; sticky)."""
from math import gcd

import numpy as np

from libfsm_amd import FlatDfa
from libfsm_amd.capi import RANGE_DTYPE

NO = 0xFFFFFFFF
LIB_DEAD = 0xFFFFFFFC      # fsm_hip.h FSM_HIP_STATE_DEAD: what the resumed fronts carry for a dead input
LIB_START = 0xFFFFFFFD


def class_map(K):
    """cls[256]: K contiguous byte ranges, bounds np.linspace(0, 256, K + 1)"""
    assert 1 <= K <= 256
    bounds = np.linspace(0, 256, K + 1).astype(np.int64)
    cls = np.zeros(256, np.int64)
    for c in range(K):
        cls[bounds[c]:bounds[c + 1]] = c
    return cls, bounds


def eager_ids_of_states(S, E, every=11):
    """[S][2] index (0 .. E - 1) of the eager outputs of every state, -1 = none: every `every`-th state (every 11th unless
    asked otherwise) emits one or two.  The id of index k is 5 + 3 * k: ids are not bit numbers."""
    s = np.arange(S, dtype=np.int64)
    q = s // every
    has = s % every == 0
    k1 = np.where(has, q % E, -1)
    k2 = np.where(has & (q % 2 == 1), (q * 7 + 3) % E, -1)
    k2[k2 == k1] = -1
    return np.stack([k1, k2], axis=1)


def endid_slots(S, is_end):
    """[S][3] end-ids of every state, -1 = unused slot; ascending within a state, 1 to 3 per end state, some >= 256,
    few distinct sets (many states share one)."""
    s = np.arange(S, dtype=np.int64)
    q = s // 7
    cnt = np.where(is_end, 1 + q % 3, 0)
    ids = np.stack([q % 5, 300 + q % 3, 1000 + q % 2], axis=1)
    ids[np.arange(3)[None, :] >= cnt[:, None]] = -1
    return ids


def affine(S, K, *, holes=0, sinks=0, endids=False, eager=0, every=11):
    """-> (FlatDfa, dense[S][K] int64 with -1 = no edge, cls[256]).  Start state 0."""
    cls, bounds = class_map(K)
    mult = [a for a in range(3, 200, 2) if gcd(a, S) == 1][:8]
    s = np.arange(S, dtype=np.int64)
    c = np.arange(K, dtype=np.int64)
    a = np.array([mult[k % len(mult)] for k in range(K)], np.int64)
    b = 1 + 37 * c
    dense = (s[:, None] * a[None, :] + b[None, :]) % S
    is_end = s % 7 == 3
    if holes:
        dense[s % holes == 0, K - 1] = -1            # DEAD is one step of the last class away from every such state
    if sinks:
        dense[S - sinks:, :] = s[S - sinks:, None]   # absorbing accepts
        is_end[S - sinks:] = True
    keep = dense >= 0
    r = np.zeros(int(keep.sum()), RANGE_DTYPE)
    r["lo"] = np.broadcast_to(bounds[:-1][None, :], (S, K))[keep]
    r["hi"] = np.broadcast_to(bounds[1:][None, :] - 1, (S, K))[keep]
    r["to"] = dense[keep]
    edge_off = np.zeros(S + 1, np.uint32)
    edge_off[1:] = np.cumsum(keep.sum(axis=1))
    endid_off, ids = np.zeros(S + 1, np.uint32), np.zeros(0, np.uint32)
    if endids:
        slots = endid_slots(S, is_end)
        endid_off[1:] = np.cumsum((slots >= 0).sum(axis=1))
        ids = slots[slots >= 0].astype(np.uint32)
    eo = ei = None
    if eager:
        ek = eager_ids_of_states(S, eager, every)
        eo = np.zeros(S + 1, np.uint32)
        eo[1:] = np.cumsum((ek >= 0).sum(axis=1))
        lo, hi = np.minimum(ek[:, 0], ek[:, 1]), np.maximum(ek[:, 0], ek[:, 1])      # ascending within a state
        two = ek[:, 1] >= 0
        srt = np.where(two[:, None], np.stack([lo, hi], axis=1), ek)
        ei = (5 + 3 * srt[srt >= 0]).astype(np.uint32)
    flat = FlatDfa(S, 0, edge_off, r, is_end.astype(np.uint8), endid_off, ids, eo, ei)
    return flat, dense, cls


# the automata of tests/test_gpu_global_table.py and tests/test_plan.py: name -> (S, K, keyword arguments)
FAMILY = {
    "last16": (65534, 4, {}),                               # S1 = 65535: the largest table of 2-byte entries
    "first32": (65535, 4, {}),                              # S1 = 65536: the first that needs 4-byte entries
    "odd_rows": (3000, 29, {}),                             # 58-byte rows: the head's boundary is no multiple of 16
    "all_hot": (3000, 4, {}),                               # 24 KB: all of it in LDS by default
    "bytewise_reordered": (8000, 256, {}),                  # 512-byte rows, still re-ordered (S1 * C <= 4 Mi)
    "bytewise_plain": (20000, 256, {}),                     # S1 * C > 4 Mi: rows keep the renumbered order
    "dying": (65534, 4, dict(holes=64, sinks=8, endids=True)),
    "eager40": (65534, 4, dict(eager=40)),
    "eager100": (65534, 4, dict(eager=100)),
}


def family(name):
    S, K, kw = FAMILY[name]
    return affine(S, K, **kw)


def trace(dense, cls, start, rows, lens=None, state_in=None):
    """[n][L + 1] int64: the state of row i before byte t (column t) and after the last one (column L); -1 = DEAD.
    Bytes at or beyond lens[i] leave the state as it is."""
    rows = np.asarray(rows, np.uint8)
    n, L = rows.shape
    S, K = dense.shape
    tab = np.vstack([dense, np.full((1, K), -1, np.int64)])      # row S (= index -1): DEAD stays DEAD
    cur = np.full(n, start, np.int64) if state_in is None else np.asarray(state_in, np.int64).copy()
    out = np.empty((n, L + 1), np.int64)
    out[:, 0] = cur
    lens = np.full(n, L, np.int64) if lens is None else np.asarray(lens, np.int64)
    for t in range(L):
        nxt = tab[cur, cls[rows[:, t]]]
        cur = np.where(t < lens, nxt, cur)
        out[:, t + 1] = cur
    return out


def walk(dense, cls, start, rows, lens=None, state_in=None):
    """-> the state every row ends in (caller's numbering, -1 = DEAD)"""
    return trace(dense, cls, start, rows, lens, state_in)[:, -1]


def ends(flat, states):
    """what the fronts report for a walk that stopped in `states`: the state where it is an end state, else NO_MATCH"""
    st = np.asarray(states, np.int64)
    ok = (st >= 0) & flat.is_end.astype(bool)[np.maximum(st, 0)]
    return np.where(ok, st, NO).astype(np.uint32)


def carried(states):
    """a walk's states as the resumed fronts carry them: the state's id, the library's DEAD code for -1"""
    st = np.asarray(states, np.int64)
    return np.where(st < 0, LIB_DEAD, st).astype(np.uint32)


def walk_eager(dense, cls, start, rows, E, lens=None, state_in=None, every=11):
    """-> (end states as walk(), emitted[n][E] bool by id INDEX): the outputs of the start state (a walk from the start
    only: a resumed piece emits nothing for the state it is handed) and of every state entered; DEAD emits nothing."""
    tr = trace(dense, cls, start, rows, lens, state_in)
    n, L1 = tr.shape
    ek = np.vstack([eager_ids_of_states(dense.shape[0], E, every), [[-1, -1]]])
    lens = np.full(n, L1 - 1, np.int64) if lens is None else np.asarray(lens, np.int64)
    emitted = np.zeros((n, E + 1), bool)                           # column E takes the "none" writes
    ar = np.arange(n)
    for t in range(0 if state_in is None else 1, L1):
        live = (t <= lens)
        for j in (0, 1):
            k = ek[tr[:, t], j]
            emitted[ar[live], k[live]] = True
    return tr[:, -1], emitted[:, :E]


def eager_sets(emitted):
    """emitted[n][E] -> per row the ascending ids (5 + 3 * index), as HipDfa.decode_eager lists them"""
    return [(5 + 3 * np.nonzero(r)[0]).astype(np.uint32) for r in emitted]


def endids_of(flat, state):
    """the end-ids of one state, from the formula (not from the description's arrays)"""
    sl = endid_slots(flat.nstates, flat.is_end.astype(bool))[state]
    return sl[sl >= 0].astype(np.uint32)


def packed(rows, lens):
    """the first lens[i] bytes of every row back to back -> (bytes, u64 offsets[n + 1])"""
    rows = np.asarray(rows, np.uint8)
    lens = np.asarray(lens, np.int64)
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    mask = np.arange(rows.shape[1])[None, :] < lens[:, None]
    return np.ascontiguousarray(rows[mask]), off


def varlens(n, L, rng):
    """lengths 0, 1, 15, 16, 17, then random up to L"""
    lens = rng.randint(0, L + 1, n).astype(np.uint32)
    head = np.array([0, 1, 15, 16, 17], np.uint32)[:n]
    lens[:len(head)] = np.minimum(head, L)
    return lens
