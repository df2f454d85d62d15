"""Automata, inputs and a CPU model of the chunk skip for the self-loop-mask layouts (FSM_HIP_LAYOUT_COMBSELF / _LDSSELF:
walk_kernels.h CombSelfPol / LdsSelfPol).  tests/test_selfloop_cases.py holds the conditions on them, tests/test_gpu_selfloop.py
launches them.  Nothing here calls a walk of the library: the automata are dense tables, the expected answers the oracle's,
and the model restates the three layers of the skip decision from the PLAN's own arrays (cls, comb_rng, comb_smask, the
LDSSELF row masks) -- so that the case tests can prove that the inputs reach every branch.

Family "select": start state 0; byte 0x01 + k enters the looping state L_k (state 1 + k), which loops on SETS[k]; LEAVE[k]
goes on to ACC; every other byte has no edge.  A literal 0xC0 0xC1 ... off the start state ("fillers") raises the class count
by one per byte: 28 classes without, 31 with three, 32 with four, and five are refused by both layouts.

LEAVE[k] is the first of 0x21, 0x00, 0x01, 0xFF outside the set (0x21 for eleven sets, 0x00 for 1..127 and 2..255, 0xFF for
0..127 and 0..126 -- 0x01 lies inside both, so leaving by it would cut the loop into two runs).

"ping-pong": A (the start state) loops on 128..255, B on 1..127, a byte of the other's set moves between them; 0x00 leaves A
to one absorbing accepting state and B to another, so that a row left in the wrong one of the two ends in the wrong state
(any later byte of the other's set would mend it: the 0x00 falls on chunk byte 0 behind whole chunks of such bytes)."""
import functools

import numpy as np

from libfsm_amd import FlatDfa

NO = 0xFFFFFFFF
START, DEAD = 0xFFFFFFFD, 0xFFFFFFFC
RNG_NONE = 0x0080                         # plan.cpp emit_combself: lo 128, hi 0 -- no byte passes

SETS = (((48, 57),), ((0, 127),), ((128, 255),), ((1, 127),), ((0, 0),), ((127, 127),), ((128, 128),), ((129, 255),), ((100, 200),),
        ((0x80, 0xFE),), ((48, 57), (97, 102)), ((0, 0x20), (0x22, 255)), ((65, 65),), ((0, 126),), ((2, 255),))
K = len(SETS)
# what the planner must make of them (lo, hi), None = "no range" (RNG_NONE)
WANT_RNG = ((48, 57), (0, 127), (128, 255), (1, 127), (0, 0), (127, 127), None, None, None, None, None, None, (65, 65), (0, 126), (2, 255))
ONE_RUN = tuple(k for k in range(K) if WANT_RNG[k] is not None)
REFUSED = tuple(k for k in range(K) if WANT_RNG[k] is None)
START_LOOP_BYTE = 0x10                    # the start state's own loop byte in the "startloop" variant: one class more
ACC_ID = 100

STRIDES = (128, 256, 48)
SUBS = (1, 63, 64, 65, 3 * 64 + 1)
LANES = (0, 31, 32, 63, 17)


def members(k):
    m = np.zeros(256, bool)
    for lo, hi in SETS[k]:
        m[lo:hi + 1] = True
    return m


def leave_byte(k):
    m = members(k)
    return next(b for b in (0x21, 0x00, 0x01, 0xFF) if not m[b])


def fillers_of(k):
    """the bytes a row idles on in L_k: lo, hi and a middle value of every run"""
    out = []
    for lo, hi in SETS[k]:
        out += [lo, hi, (lo + hi) // 2]
    return np.array(out, np.uint8)


def outliers_of(k):
    """bytes outside the set that end the loop: lo - 1 and hi + 1 of every run, 0x00, 0x7F, 0x80, 0xFF, the leave byte itself"""
    m = members(k)
    c = []
    for lo, hi in SETS[k]:
        c += [lo - 1, hi + 1]
    c += [0x00, 0x7F, 0x80, 0xFF, leave_byte(k)]
    out = []
    for b in c:
        if 0 <= b <= 255 and not m[b] and b not in out:
            out.append(b)
    return out


class Case:
    """one automaton: the dense table, its FlatDfa, and what the row builders need to know about its looping states"""

    def __init__(self, name, dense, is_end, endids=None, eager=None, kind="select", start_loop=False):
        self.name, self.kind, self.start_loop = name, kind, start_loop
        self.dense = dense
        S = len(dense)
        eo = ei = None
        if eager is not None:
            eo, ei = np.zeros(S + 1, np.uint32), []
            for s in range(S):
                ei += eager.get(s, [])
                eo[s + 1] = len(ei)
            ei = np.array(ei, np.uint32)
        self.flat = FlatDfa.from_dense(dense, 0, is_end, endids, eo, ei)
        self.is_end = np.asarray(is_end, bool)
        self.loops = dense == np.arange(S)[:, None]          # [S][256]: byte b is a self-loop of state s

    @functools.cached_property
    def oracle(self):
        from oracle.pyoracle import Oracle
        return Oracle(self.flat)

    def ends(self, rows, lens=None):
        return self.oracle.table_walk(rows, lens)

    def states(self, rows, lens=None, state_in=None):
        """the state every row is in after its bytes: a state id, or DEAD"""
        st = np.full(len(rows), START, np.uint32) if state_in is None else state_in
        out = self.oracle.state_walk(rows, st, lens)
        return np.where(out == START, np.uint32(0), out).astype(np.uint32)

    def end_of_states(self, st):
        ok = st < len(self.dense)
        return np.where(ok & self.is_end[np.minimum(st, len(self.dense) - 1)], st, np.uint32(NO)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def select(fillers=0, acc="none", start_loop=False, loops_accept=False, eager=False):
    S = 2 + K + fillers
    ACC = 1 + K
    d = np.full((S, 256), -1, np.int64)
    for k in range(K):
        d[0, 0x01 + k] = 1 + k
        d[1 + k, members(k)] = 1 + k
        d[1 + k, leave_byte(k)] = ACC
    if acc == "absorbing":
        d[ACC, :] = ACC
    if start_loop:
        d[0, START_LOOP_BYTE] = 0
    at = 0
    for j in range(fillers):                                  # the literal 0xC0 0xC1 ...: its last state accepts
        d[at, 0xC0 + j] = ACC + 1 + j
        at = ACC + 1 + j
    is_end = np.zeros(S, np.uint8)
    is_end[ACC] = 1
    endids = {ACC: [ACC_ID]}
    if fillers:
        is_end[S - 1] = 1
        endids[S - 1] = [ACC_ID + 1]
    if loops_accept:
        is_end[1:1 + K] = 1
        endids.update({1 + k: [k] for k in range(K)})
    name = f"select{'+%d' % fillers if fillers else ''}{' acc=' + acc if acc != 'none' else ''}{' startloop' if start_loop else ''}" \
           f"{' loops accept' if loops_accept else ''}{' eager' if eager else ''}"
    return Case(name, d, is_end, endids, {1 + k: [k] for k in range(K)} if eager else None, start_loop=start_loop)


@functools.lru_cache(maxsize=None)
def pingpong():
    A, B, ACC_A, ACC_B = 0, 1, 2, 3
    d = np.full((4, 256), -1, np.int64)
    d[A, 128:] = A
    d[A, 1:128] = B
    d[B, 1:128] = B
    d[B, 128:] = A
    d[A, 0], d[B, 0] = ACC_A, ACC_B
    d[ACC_A, :], d[ACC_B, :] = ACC_A, ACC_B                  # absorbing: a row that met its 0x00 in the wrong state keeps saying so
    return Case("ping-pong", d, [0, 0, 1, 1], {ACC_A: [1], ACC_B: [2]}, kind="pingpong", start_loop=True)


def fillers_for(hip, layout, want_c, **kw):
    """how many filler states give the variant `want_c` classes: by the class count the plan reports, not by a formula"""
    for f in range(0, 8):
        if hip.Plan(select(f, **kw).flat, layout).C == want_c:
            return f
    raise AssertionError((want_c, kw))


# ---- rows ------------------------------------------------------------------------------------------------------------------------

def slots_of(nch):
    """the chunks that get a lone outlier: the first, the one behind it, a middle one, the last two"""
    return sorted({c for c in (0, 1, nch // 2, nch - 2, nch - 1) if 0 <= c < nch})


def wave_plan(which=ONE_RUN + REFUSED):
    """the wavefronts of a batch as (states of the 64 lanes, byte position 0..15 of its outliers): first those that mix looping
    states lane by lane (all fifteen, then the nine whose loop is one range), then one per state and byte position"""
    waves = []
    for p in range(16):
        waves.append((np.array([(lane + p) % K for lane in range(64)]), p))
        waves.append((np.array([ONE_RUN[(lane + p) % len(ONE_RUN)] for lane in range(64)]), p))
    for k in which:
        for p in range(16):
            waves.append((np.full(64, k), p))
    return waves


def varlens(n, L):
    """lengths 0..L: three rows in four are long (the ragged kernel's tails behind whole chunks), one takes every length in turn"""
    i = np.arange(n)
    return np.where(i % 4 == 0, (i // 4 * 37) % (L + 1), L - (i * 11) % min(33, L)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def select_rows(L, varlen=False, start_loop=False, interior=True):
    """-> (rows u8 [n][L], lens u32 [n], state k of every row).  A row: [START_LOOP_BYTE prefix] selector, fillers of its set,
    at most one outlier, fillers, the leave byte last (at its length).  Every wavefront has one lone outlier in each chunk of
    slots_of(), each in another lane; a third of the rows without one end badly (an outlier, or a filler, for the leave byte).
    The rows are the same for every variant of the family but the one whose start state loops: there the selector stands behind
    0, 16, 32 or 7 bytes of that loop, and two wavefronts in sixteen meet a whole chunk of its byte in every lane.
    interior=False: outliers in the first and the last chunk only --
    rows of three chunks have ONE chunk that can be skipped, which the same wavefront cannot both pass and fail."""
    waves = wave_plan()
    n = 64 * len(waves)
    lens = varlens(n, L) if varlen else np.full(n, L, np.uint32)
    rows = np.zeros((n, L), np.uint8)
    state = np.zeros(n, np.int64)
    for w, (ks, p) in enumerate(waves):
        # the start state's own loop: whole chunks of it before the selector (0, 1, 2 chunks) or 7 bytes, by wavefront
        pre = (0, 16, 32, 7)[w % 4] if start_loop and L >= 128 else 0
        nch = (L - pre) // 16
        slots = [c for c in slots_of(nch) if interior or c in (0, nch - 1)]
        for lane in range(64):
            i, k = 64 * w + lane, int(ks[lane])
            n_i = int(lens[i])
            state[i] = k
            f, out = fillers_of(k), outliers_of(k)
            r = rows[i]
            r[:pre] = START_LOOP_BYTE
            r[pre:] = f[(np.arange(L - pre) + lane) % len(f)]
            if pre < L:
                r[pre] = 0x01 + k
            has = False
            for si, c in enumerate(slots):
                if lane != LANES[(si + p) % len(LANES)]:
                    continue
                pos = pre + 16 * c + p
                if pos == pre or pos >= n_i - 1:
                    continue                                   # the selector's and the leave byte's places
                j = (p + si + k) % len(out)
                if out[j] == leave_byte(k) and c + 1 < nch - 1 and (c + 1 in slots or not interior):
                    # (a row in ACC fails the NEXT chunk too: not where that has its own lone lane, or is the one that is to pass;
                    # the last chunk holds every row's leave byte and passes for nobody)
                    if len(out) == 1:
                        continue
                    j = (j + 1) % len(out)
                r[pos] = out[j]
                has = True
            # the byte the START state loops on, as a whole chunk in EVERY lane of the wavefront: lanes that kept the start state's
            # range would pass it together (it ends ten of the fifteen loops)
            cx = pre + 16 * (nch // 2 + 1)
            if start_loop and p in (3, 11) and pre % 16 == 0 and nch // 2 + 1 < nch - 2 and cx + 16 <= n_i - 1:
                r[cx:cx + 16] = START_LOOP_BYTE
            if n_i >= pre + 2:
                r[n_i - 1] = leave_byte(k)
                if not has and (lane * 5 + w) % 3 == 0:
                    bad = [b for b in out if b != leave_byte(k)]
                    r[n_i - 1] = bad[(lane + w) % len(bad)] if bad and w % 2 == 0 else f[lane % len(f)]
    return rows, lens, state


@functools.lru_cache(maxsize=None)
def pingpong_rows(L, varlen=False):
    """rows of bytes from A's and B's sets by turns, 0x00 last.  Wavefront w, lane l: the byte that leads to the other state
    falls on chunk bytes 0, 15 and 16 (= byte 0 of the next chunk) of the first, a middle and the last chunks, and whole chunks
    of either set lie behind it; a lone lane (0, 31, 32, 63) switches where the other 63 stay."""
    nch = L // 16
    nw = 64
    n = 64 * nw
    lens = varlens(n, L) if varlen else np.full(n, L, np.uint32)
    rows = np.zeros((n, L), np.uint8)
    a_f, b_f = np.array([128, 255, 200], np.uint8), np.array([1, 127, 64], np.uint8)
    for w in range(nw):
        c = slots_of(nch)[w % len(slots_of(nch))]
        at = 16 * c + (0, 15, 16)[(w // 5) % 3]                # where the switch falls
        lone = w % 2 == 0
        for lane in range(64):
            i = 64 * w + lane
            n_i = int(lens[i])
            side = np.zeros(L, bool)                            # False: a byte of A's set (stay in / go to A), True: of B's
            if w % 4 >= 2:
                side[:] = True
            if not lone or lane == LANES[(w // 2) % 4]:
                side[at:] ^= True
                # ... and back, at the same byte in every lane that switches: whole chunks of the other set lie between, which a
                # wavefront that kept the range of the state it left would pass together
                back = at + (16, 17, 31, 32, 1)[(w // 3) % 5]
                if w % 3 and back < L:
                    side[back:] ^= True
            r = rows[i]
            r[:] = np.where(side, b_f[(np.arange(L) + lane) % 3], a_f[(np.arange(L) + lane) % 3])
            if n_i >= 1 and (lane + w) % 3:
                r[n_i - 1] = 0
            if (lane * 3 + w) % 11 == 0 and n_i >= 20:
                r[n_i // 2] = 0                                 # accepted early, for good: on chunk byte 0 where the row is whole
    return rows, lens, None


BATCHES = ((128, 0), (256, 0), (48, 0), (48, 1))     # (stride, part): rows of three chunks come as two batches


def rows_of(case, L, varlen=False, part=0):
    """part 1 (stride 48): the same rows without the outliers of the middle chunk"""
    if case.kind == "pingpong":
        return pingpong_rows(L, varlen)
    return select_rows(L, varlen, case.start_loop, part == 0)


def packed_from(rows, lens, off0=0):
    """rows cut to their lengths, back to back behind off0 bytes that belong to no line -> (bytes, u64 offsets [n + 1])"""
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    off += np.uint64(off0)
    keep = np.arange(rows.shape[1])[None, :] < np.asarray(lens)[:, None]
    return np.concatenate([np.full(off0, 0x21, np.uint8), rows[keep]]), off


# ---- the model of the skip -----------------------------------------------------------------------------------------------------

class Model:
    """what the three layers of the chunk skip would answer for a batch, from the plan's own arrays.

    st[c][i]: row i's state (plan numbering; S1 - 1 = DEAD) before chunk c, by the oracle's walk of the prefix.
    raw[c][i] / vote[c][i]: would lane i pass the range test on the raw bytes (the plan's comb_rng, byte by byte) / the class
    vote (cls + comb_smask, or the LDSSELF row masks) on chunk c -- whole chunks only; tails: tail_pass()."""

    def __init__(self, hip, case, layout, rows, lens=None):
        self.case, self.rows = case, rows
        n, L = rows.shape
        self.n, self.L, self.nch = n, L, L // 16
        self.lens = np.full(n, L, np.uint32) if lens is None else np.asarray(lens, np.uint32)
        p = hip.Plan(case.flat, layout)
        self.p = p
        self.C, self.cls = p.C, p.get("cls").astype(np.int64)
        new2old = p.get("new2old").astype(np.int64)
        self.old2new = np.full(len(case.dense) + 1, p.S1 - 1, np.int64)
        self.old2new[new2old[:p.S1 - 1]] = np.arange(p.S1 - 1)
        if layout == hip.LAYOUT_COMBSELF:
            off = p.get("comb_off").astype(np.int64)
            self.smask = p.get("comb_smask")[off[:p.S1]].astype(np.uint32)
            self.rng = p.get("comb_rng")[off[:p.S1]].astype(np.int64)
        else:
            tab = p.get("lds_tab").reshape(p.S1, p.row_bytes // 2)
            cpad = (p.C + 1) & ~1
            self.smask = tab[:, cpad].astype(np.uint32) | (tab[:, cpad + 1].astype(np.uint32) << 16)
            self.rng = None
        self.st = np.stack([self.plan_state(case.states(rows, np.minimum(self.lens, 16 * c))) for c in range(self.nch + 1)])
        ch = rows[:, :self.nch * 16].reshape(n, self.nch, 16).transpose(1, 0, 2)       # [c][i][16]
        self.whole = (16 * (np.arange(self.nch)[:, None] + 1) <= self.lens[None, :])   # [c][i]: the chunk lies inside the row
        self.raw, self.raw_first_bad = self.raw_pass(self.st[:self.nch], ch)
        self.vote = self.vote_pass(self.st[:self.nch], ch)

    def plan_state(self, st):
        return self.old2new[np.minimum(st.astype(np.int64), len(self.case.dense))]

    def raw_pass(self, st, ch):
        """-> (all 16 bytes inside the state's range, the first byte position outside it or 16)"""
        if self.rng is None:
            z = np.zeros(st.shape, bool)
            return z, np.zeros(st.shape, np.int64)
        lo, hi = (self.rng[st] & 0xff)[..., None], (self.rng[st] >> 8)[..., None]
        inside = (ch >= lo) & (ch <= hi)
        return inside.all(-1), np.where(inside.all(-1), 16, np.argmin(inside, -1))

    def vote_pass(self, st, ch, valid=None):
        """all classes of the chunk's (valid) bytes are self-loops of the state; bytes that are not valid count as the spare class"""
        bit = ((self.smask[st][..., None] >> self.cls[ch].astype(np.uint32)) & 1).astype(bool)
        if valid is not None:
            bit = bit | ~valid
        return bit.all(-1)

    def state_k(self, c):
        """[i]: the looping state L_k row i is in before chunk c, or -1 (select family)"""
        old = np.full(self.p.S1, -1, np.int64)
        new2old = self.p.get("new2old").astype(np.int64)
        old[:self.p.S1 - 1] = new2old[:self.p.S1 - 1]
        s = old[self.st[c]]
        return np.where((s >= 1) & (s <= K), s - 1, -1)

    def waves(self, a):
        """[c][i] -> [c][w][64] over the batch's whole wavefronts"""
        nw = self.n // 64
        return a[:, :nw * 64].reshape(a.shape[0], nw, 64)

    def tails(self, lo_positive):
        """the partial chunk of every row with a tail (1..15 bytes behind its whole chunks), as the kernels see it after
        fill_invalid.  lo == 0 (the per-lane kernels, LDS-DMA, direct): the chunk starts where the tail starts, bytes
        [0, tail) are the row's, the rest copies of byte 0.  lo > 0 (walk_ragged, rows of 16 bytes and more): the chunk is the
        row's LAST 16 bytes, bytes [16 - tail, 16) are still to walk, the rest copies of byte 16 - tail.
        -> (row indexes, tail, state before the tail, filled chunk [m][16], valid [m][16])"""
        tail = self.lens % 16
        nfull = self.lens // 16
        idx = np.nonzero((tail > 0) & ((nfull > 0) if lo_positive else True))[0]
        t, nf = tail[idx].astype(np.int64), nfull[idx].astype(np.int64)
        st = self.st[nf, idx]
        pad = np.concatenate([self.rows, np.zeros((self.n, 16), np.uint8)], 1)
        k = np.arange(16)[None, :]
        if lo_positive:
            lo = 16 - t
            ch = pad[idx[:, None], (nf * 16 + t - 16)[:, None] + k]
            valid = k >= lo[:, None]
            rep = ch[np.arange(len(idx)), lo]
        else:
            ch = pad[idx[:, None], (nf * 16)[:, None] + k]
            valid = k < t[:, None]
            rep = ch[:, 0]
        return idx, t, st, np.where(valid, ch, rep[:, None]), valid
