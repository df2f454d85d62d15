"""GPU (-m gpu): the many-DFA front (libfsm_amd/csrc/multi.hip: walk_multi, walk_multi_eager and the planner around them) at
its edges -- every table form (the u16 LDS copy at exactly 16 384 entries, the global-table form one row beyond, a plain table
of exactly 1 MiB and one row more), ragged lines of up to 300 bytes (whole chunks, partial chunks, finished, dead and absorbed
lanes in one wavefront), the fuse limits at n = 65 536 / 65 537, 1 MiB / 1 MiB + 1 byte and the staging cap, the 256-line tile,
exactly sized device text, outputs left out, refusals, and the staging context behind a device launch and under two threads.

The automata are tests/global_ref.py's affine family (start state 0).  Every answer is judged by global_ref's closed formulas
(walk, ends, walk_eager, eager_sets' numbering, endids_of): no answer is compared with a HipDfa front or with another many-DFA
call.  The shape of every automaton (S1 = S + 1, C = K, the plain table's size, abs_min, the eager thresholds) is asserted from
the CPU planner before the automaton's first launch, and what the lines are for (the share of dead, absorbed and live lanes, the
ids that fire) from the reference alone."""
import errno
import functools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import global_ref as G

pytestmark = pytest.mark.gpu

NO, NO_ID = 0xFFFFFFFF, 0xFFFFFFFE
EARLIEST, RET, IDS_ERROR = 1, 2, 3
JUNK32, JUNK64 = 0x77777777, 0x7777777777777777     # what every output holds before a launch
LDS_ENTRIES = 16384                                  # multi.hip MULTI_LDS_ENTRIES
N, L = 1500, 300
SPARE = 2                                            # bitmap words behind (n + 63) / 64: they keep their junk

SPEC = {
    "lds_full": (1023, 16, {}),                                           # 16 384 entries: the largest LDS table, 1 024 rows of 32 bytes
    "lds_wide": (63, 256, {}),                                            # 16 384: 512-byte rows, every byte a class of its own
    "lds_mid": (511, 32, {}),                                             # 16 384
    "glob_first": (1024, 16, {}),                                         # 16 400: the first table off LDS
    "glob_1mib": (1023, 256, {}),                                         # 262 144 entries: exactly MULTI_FUSE_TABLE
    "glob_over": (1024, 256, {}),                                         # one row too many: never fused
    "dying": (1023, 16, dict(holes=8, sinks=4, endids=True)),             # DEAD and absorbing accepts reachable
    "dying_glob": (1024, 16, dict(holes=64, sinks=8, endids=True)),       # the same off LDS
    "eager40": (1023, 16, dict(eager=40)),                                # W = 1
    "eager100": (1023, 16, dict(eager=100)),                              # W = 2
    "eager100_glob": (1024, 16, dict(eager=100)),                         # W = 2, global-table form on the host front
}
ALL = tuple(SPEC)
LDS = tuple(k for k in ALL if (SPEC[k][0] + 1) * SPEC[k][1] <= LDS_ENTRIES)
OFF_LDS = tuple(k for k in ALL if k not in LDS)
assert len(LDS) == 6 and len(OFF_LDS) == 5


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()   # raises if the HIP extension is missing: no silent fallback
    return libfsm_amd


# ---- automata ----------------------------------------------------------------------------------------------------------

class Auto:
    def __init__(self, name):
        self.name = name
        self.S, self.K, self.kw = SPEC[name]
        self.flat, self.dense, self.cls = G.affine(self.S, self.K, **self.kw)
        self.E = self.kw.get("eager", 0)
        self.sinks = self.kw.get("sinks", 0)


@functools.lru_cache(maxsize=None)
def auto(name):
    return Auto(name)


def assert_shape(hip, name):
    """what the planner makes of the automaton, before its first launch"""
    a = auto(name)
    p = hip.Plan(a.flat, 0)
    assert p.S1 == a.S + 1 and p.C == a.K and len(p.get("dense")) == p.S1 * p.C, name
    assert (p.S1 * p.C <= LDS_ENTRIES) == (name in LDS), name
    assert p.S1 * p.C == {"lds_full": 16384, "lds_wide": 16384, "lds_mid": 16384, "glob_first": 16400, "glob_1mib": 262144, "glob_over": 262400,
                          "dying": 16384, "dying_glob": 16400, "eager40": 16384, "eager100": 16384, "eager100_glob": 16400}[name]
    if name == "dying":
        assert p.abs_min == 1019 and p.nabsorbing == 5            # four sinks and DEAD
    elif name == "dying_glob":
        assert p.nabsorbing == 9 and p.abs_min == p.S1 - 9
    else:
        assert p.nabsorbing == 1 and p.abs_min == p.S1 - 1        # DEAD alone (unreachable)
    if name in ("eager40", "eager100"):
        assert p.eager_lo_end == 93 and p.eager_hi_begin == 1023
    return p


_dfas = {}


def dfa(hip, name):
    """ONE handle per automaton for the whole file, DEFER_UPLOAD (the fused launch never needs the dfa's own image)"""
    if name not in _dfas:
        assert_shape(hip, name)
        d = hip.HipDfa(auto(name).flat, hip.DEFER_UPLOAD)
        flat = auto(name).flat          # (ids that no state carries are not counted: 93 emitting states make 95 of eager100's)
        E = len(np.unique(flat.eager_ids)) if flat.eager_ids is not None else 0
        assert d.eager_id_count() == E and (not E or d.eager_words() == (E + 63) // 64)
        _dfas[name] = d
    return _dfas[name]


@pytest.fixture(scope="module", autouse=True)
def _close_dfas():
    yield
    for d in _dfas.values():
        d.close()
    _dfas.clear()


# ---- lines and the reference's answers ---------------------------------------------------------------------------------

def ragged(n, seed, L=L, blocks=True):
    """random bytes; lengths 0, 1, 15, 16, 17, then random up to L.  blocks: lines 64 .. 127 have exactly 48 bytes (a wavefront
    that takes the whole-chunk loop for its whole walk), lines 128 .. 191 alternate 48 and 41 (it leaves that loop at its last chunk)"""
    rng = np.random.RandomState(seed)
    rows = rng.randint(0, 256, (n, L)).astype(np.uint8)
    lens = G.varlens(n, L, rng).astype(np.int64)
    if blocks:
        assert n >= 192 and L >= 48
        lens[64:128] = 48
        lens[128:192:2] = 48
        lens[129:192:2] = 41
    return rows, lens


class Job:
    """an automaton, its packed lines and the reference's answers (computed once, left as they are)"""

    def __init__(self, name, rows, lens, lead=0, eager=False):
        a = auto(name)
        self.name, self.a = name, a
        lens = np.asarray(lens, np.int64)
        self.n, self.lens = len(lens), lens
        rows = np.ascontiguousarray(np.asarray(rows, np.uint8)[:, :int(lens.max()) if len(lens) else 0])
        self.st = G.walk(a.dense, a.cls, 0, rows, lens)
        self.end = G.ends(a.flat, self.st)
        self.em = None
        if eager and a.E:
            st, self.em = G.walk_eager(a.dense, a.cls, 0, rows, a.E, lens)
            assert np.array_equal(st, self.st)
        text, off = G.packed(rows, lens)
        if lead:                                       # bytes in front of the first line that are no text: off[0] = lead
            text = np.concatenate([np.full(lead, 0xC3, np.uint8), text])
            off = off + np.uint64(lead)
        self.text, self.off = np.ascontiguousarray(text), np.ascontiguousarray(off, np.uint64)
        for x in (self.st, self.end, self.text, self.off):
            x.setflags(write=False)

    def bitmap(self):
        w = (self.n + 63) // 64
        bits = np.zeros(w * 64, np.uint8)
        bits[:self.n] = self.end != NO
        return np.packbits(bits, bitorder="little").view(np.uint64)       # (spare bits of the last word: zero)

    @functools.lru_cache(maxsize=None)
    def earliest(self):
        """FSM_HIP_IDS_EARLIEST: the lowest id of the end state, NO_ID for an end state without ids, NO_MATCH for a reject"""
        out = np.full(self.n, NO, np.uint32)
        for s in set(self.end[self.end != NO].tolist()):
            ids = G.endids_of(self.a.flat, s) if self.a.kw.get("endids") else np.zeros(0, np.uint32)
            out[self.end == s] = int(ids.min()) if len(ids) else NO_ID
        return out

    def set_words(self, d):
        """the eager sets as the device writes them: W words a line, bit b = the id d.eager_id(b); the reference numbers its
        ids 5 + 3 * index.  An automaton without eager outputs (or a job that the reference walked without): zero words."""
        W = max(d.eager_words(), 1)
        bits = np.zeros((self.n, W * 64), np.uint8)
        if self.em is not None:
            for b in range(d.eager_id_count()):
                k, r = divmod(d.eager_id(b) - 5, 3)
                assert r == 0 and 0 <= k < self.a.E
                bits[:, b] = self.em[:, k]
        return np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(-1)


@functools.lru_cache(maxsize=None)
def job1500(name, rep=0, eager=False):
    """the N ragged lines of an automaton; rep = 1: other bytes in the same lines (the same offsets)"""
    k = ALL.index(name)
    rows, lens = ragged(N, 1500 + k)
    if rep:
        rows = np.random.RandomState(9000 + k).randint(0, 256, rows.shape).astype(np.uint8)
    j = Job(name, rows, lens, eager=eager)
    if name == "dying":        # what the lines are for, from the reference alone
        dead, sink = j.st < 0, j.st >= auto(name).S - auto(name).sinks
        shares = float(dead.mean()), float(sink.mean()), float((~dead & ~sink).mean())
        print("dying, n = %d: DEAD %.2f, absorbing accept %.2f, neither %.2f" % ((N,) + shares))
        assert min(shares) >= 0.1, shares
        assert (j.end[sink] != NO).all() and (j.end[dead] == NO).all()
    if name.startswith("eager100") and eager:
        fired, most = int(j.em.any(axis=0).sum()), int(j.em.sum(axis=1).max())
        print("%s: %d of 100 ids fire, one line carries %d" % (name, fired, most))
        assert fired >= 90 and most >= 20
    assert 0 < int((j.end != NO).sum()) < N
    return j


# ---- buffers and submissions -------------------------------------------------------------------------------------------

KEYS = ("end", "bm", "ids", "sets")


class Bufs:
    """one job's memory, host (numpy) or device (torch): the text EXACTLY sized (off[n] bytes, nothing behind the last line),
    every output filled with junk, the bitmap SPARE words longer than needed"""

    def __init__(self, hip, job, device):
        self.job, self.device = job, device
        self.W = max(dfa(hip, job.name).eager_words(), 1)
        n = job.n
        self.host = dict(end=np.empty(max(n, 1), np.uint32), ids=np.empty(max(n, 1), np.uint32),
                         bm=np.empty((n + 63) // 64 + SPARE, np.uint64), sets=np.empty(max(n * self.W, 1), np.uint64))
        assert n == 0 or len(job.text) == int(job.off[n])
        self.text, self.off = job.text, job.off
        if device:
            import torch
            self.torch = torch
            self.d_text = torch.empty(len(job.text), dtype=torch.uint8, device="cuda")
            self.d_off = torch.from_numpy(job.off.view(np.int64).copy()).cuda()
            self.dev = {k: torch.empty(len(v), dtype=torch.int32 if v.dtype == np.uint32 else torch.int64, device="cuda") for k, v in self.host.items()}
            self.put_text(job)
        self.junk()

    def put_text(self, job):
        assert np.array_equal(job.off, self.off)
        self.job = job
        if self.device and len(job.text):
            self.d_text.copy_(self.torch.from_numpy(job.text.copy()))
        self.text = job.text

    def junk(self):
        for k, v in self.host.items():
            v.fill(JUNK32 if v.dtype == np.uint32 else JUNK64)
            if self.device:
                self.dev[k].fill_(JUNK32 if v.dtype == np.uint32 else JUNK64)

    def addr(self, k):
        if k == "text":
            return (self.d_text.data_ptr() if self.device else self.text.ctypes.data) if len(self.text) else 0
        if k == "off":
            return self.d_off.data_ptr() if self.device else self.off.ctypes.data
        return self.dev[k].data_ptr() if self.device else self.host[k].ctypes.data

    def read(self, k):
        if self.device:
            return self.dev[k].cpu().numpy().view(self.host[k].dtype)
        return self.host[k]


def tuples(bufs, ask, width):
    out = []
    for b, a in zip(bufs, ask):
        assert set(a) <= set(KEYS[:width - 3])
        out.append((b.addr("text"), b.addr("off"), b.job.n) + tuple(b.addr(k) if k in a else 0 for k in KEYS[:width - 3]))
    return out


def submit(hip, jobs, device, ask=("end", "bm"), width=None, ids_mode=0, stream=0, bufs=None):
    """ONE submission of the jobs, host or device form; ask: the outputs every job asks for, or one such tuple per job.
    width: 5, 6 (the ids entry point) or 7 (the eager one); default: the narrowest that holds what is asked for.
    -> (bufs, asked, (launches, fused jobs))"""
    ask = [tuple(ask)] * len(jobs) if (not ask or isinstance(ask[0], str)) else [tuple(a) for a in ask]
    if width is None:
        width = 7 if any("sets" in a for a in ask) else 6 if any("ids" in a for a in ask) else 5
    dfas = [dfa(hip, j.name) for j in jobs]
    if bufs is None:
        bufs = [Bufs(hip, j, device) for j in jobs]
    hip.exec_multi_ptrs(dfas, tuples(bufs, ask, width), ids_mode, device, stream)
    return bufs, ask, (hip.multi_last_launches(), hip.multi_last_fused_jobs())


def first_bad(got, want, job):
    bad = np.nonzero(got != want)[0][:6]
    return bad.tolist(), job.lens[bad].tolist(), got[bad].tolist(), want[bad].tolist()


def check(hip, what, bufs, ask, ids_mode=EARLIEST):
    """every output asked for against the reference; every output not asked for, and every bitmap word behind the job's, still junk"""
    if bufs and bufs[0].device:
        bufs[0].torch.cuda.synchronize()
    for q, (b, a) in enumerate(zip(bufs, ask)):
        j, tag = b.job, (what, q, b.job.name, b.job.n)
        n, w = j.n, (j.n + 63) // 64
        got = {k: b.read(k) for k in KEYS}
        for k in KEYS:
            if k not in a:
                assert (got[k] == (JUNK32 if got[k].dtype == np.uint32 else JUNK64)).all(), tag + (k, "not asked for, yet written")
        if n == 0:
            assert all((got[k] == (JUNK32 if got[k].dtype == np.uint32 else JUNK64)).all() for k in KEYS), tag
            continue
        if "end" in a:
            assert np.array_equal(got["end"][:n], j.end), tag + ("end",) + first_bad(got["end"][:n], j.end, j)
        if "bm" in a:
            want = j.bitmap()
            assert np.array_equal(got["bm"][:w], want), tag + ("bitmap", np.nonzero(got["bm"][:w] != want)[0][:6].tolist())
            assert (got["bm"][w:] == JUNK64).all(), tag + ("bitmap words behind the job's were written",)
        if "ids" in a:
            ids = got["ids"][:n]
            if ids_mode == EARLIEST:
                assert np.array_equal(ids, j.earliest()), tag + ("ids",) + first_bad(ids, j.earliest(), j)
            else:   # RET: the index of the end state's id set in the dfa's own list of sets
                sets = dfa(hip, j.name).ret_sets()
                hit = j.end != NO
                assert (ids[~hit] == NO).all() and (ids[hit] != NO).all(), tag
                for s, k2 in set(zip(j.end[hit].tolist(), ids[hit].tolist())):
                    assert k2 < len(sets) and np.array_equal(sets[k2], G.endids_of(j.a.flat, s)), tag + ("ret", s, k2)
        if "sets" in a:
            want = j.set_words(dfa(hip, j.name))
            gs = got["sets"][:n * b.W]
            if not np.array_equal(gs, want):
                bad = np.nonzero((gs != want).reshape(n, b.W).any(axis=1))[0][:6]
                raise AssertionError(tag + ("sets", bad.tolist(), j.lens[bad].tolist(), [hex(x) for x in gs.reshape(n, b.W)[bad[0]]],
                                            [hex(x) for x in want.reshape(n, b.W)[bad[0]]]))


def refused(fn, err=errno.EINVAL):
    with pytest.raises(OSError) as e:
        fn()
    assert e.value.errno == err, e.value


# ---- 0. shapes, before anything is launched ----------------------------------------------------------------------------

def test_shapes_of_automata_and_lines(hip):
    for name in ALL:
        p = assert_shape(hip, name)
        print("%s: S1 = %d, C = %d, %d entries, abs_min = %d" % (name, p.S1, p.C, p.S1 * p.C, p.abs_min))
    j = job1500("dying")
    assert (j.lens[64:128] == 48).all() and set(j.lens[128:192].tolist()) == {48, 41} and j.lens[:5].tolist() == [0, 1, 15, 16, 17]
    assert int(j.lens.max()) > 280 and int((j.lens % 16 != 0).sum()) > 1000
    job1500("eager100", 0, True)
    job1500("eager100_glob", 0, True)


# ---- 1. every table form, ragged long lines, host front ----------------------------------------------------------------

def test_every_table_form_on_ragged_long_lines_host(hip):
    """the eleven automata, N ragged lines each, ONE fsm_hip_exec_multi: only glob_over (a plain table of more than 1 MiB) goes
    through its dfa's own walk; then in reversed order without the bitmap"""
    jobs = [job1500(name) for name in ALL]
    bufs, ask, counts = submit(hip, jobs, False)
    assert counts == (2, 10), counts
    check(hip, "host", bufs, ask)
    bufs, ask, counts = submit(hip, jobs[::-1], False, ask=("end",))
    assert counts == (2, 10), counts
    check(hip, "host reversed, no bitmap", bufs, ask)


# ---- 2. the same through the device and the prepared fronts ------------------------------------------------------------

def test_every_table_form_on_ragged_long_lines_device_and_prepared(hip):
    """exactly sized text, junk in every output: the six LDS-form automata fuse, each of the five others is a launch of its own;
    the prepared form twice, the second launch on new bytes in the same buffers"""
    jobs = [job1500(name) for name in ALL]
    bufs, ask, counts = submit(hip, jobs, True)
    check(hip, "device", bufs, ask)
    assert counts == (6, 6), counts
    for b in bufs:
        b.junk()
    pr = hip.MultiPrepared([dfa(hip, j.name) for j in jobs], tuples(bufs, ask, 6), 0)
    pr.launch()
    check(hip, "prepared", bufs, ask)
    assert (hip.multi_last_launches(), hip.multi_last_fused_jobs()) == (6, 6)
    again = [job1500(name, 1) for name in ALL]
    assert not np.array_equal(again[0].end, jobs[0].end)
    for b, j in zip(bufs, again):
        b.put_text(j)
        b.junk()
    pr.launch()
    check(hip, "prepared, new bytes", bufs, ask)
    pr.close()


# ---- 3. job sizes ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def size_jobs():
    jobs = []
    for name in ("lds_full", "dying"):
        for k, n in enumerate((1, 63, 64, 65, 255, 256, 257, 511, 513)):
            rows, lens = ragged(n, 300 + k, blocks=False)
            if n == 1:
                lens[0] = 37                                      # (varlens' first line is empty)
            jobs.append(Job(name, rows, lens))
        jobs.append(Job(name, np.zeros((300, 0), np.uint8), np.zeros(300, np.int64)))       # empty lines only
        rows, lens = ragged(600, 600, blocks=False)
        lens[[255, 256, 599]] = 0
        lens[[254, 257, 598]] = 299
        jobs.append(Job(name, rows, lens))
    return jobs


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_job_sizes_around_the_wavefront_and_the_tile(hip, device):
    """n = 1 .. 513, empty lines only, empty lines on both sides of a tile's edge and at the job's end, on lds_full and dying in
    one submission; the bitmap words behind (n + 63) / 64 keep their junk, the spare bits of the last word are zero (check())"""
    jobs = size_jobs()
    assert len(jobs) == 22 and jobs[9].n == 300 and (jobs[9].end == NO).all() and jobs[10].lens[[255, 256, 599]].tolist() == [0, 0, 0]
    bufs, ask, counts = submit(hip, jobs, device)
    check(hip, "sizes", bufs, ask)
    assert counts == (1, len(jobs)), counts


# ---- 4. device tails and bases -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tail_jobs():
    jobs = []
    for name in ("lds_full", "dying", "glob_first"):
        rows, lens = ragged(200, 41, blocks=False)                # the last line ends 13 bytes past a 16-byte boundary
        lens[199] = 40
        lens[199] += (13 - int(lens.sum())) % 16
        assert int(lens.sum()) % 16 == 13
        jobs.append(Job(name, rows, lens))
        rows, lens = ragged(300, 42, blocks=False)                # the last 40 lines are 0 .. 3 bytes: lanes on both load paths
        lens[256:260] = 250
        lens[260:] = np.arange(40) % 4
        assert int(lens[260:].sum()) > 16
        jobs.append(Job(name, rows, lens))
        rows, lens = ragged(300, 43, blocks=False)                # off[0] = 5: the first five bytes are no text
        jobs.append(Job(name, rows, lens, lead=5))
        assert int(jobs[-1].off[0]) == 5
    return jobs


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_tails_of_exactly_sized_text_and_a_base_offset(hip, device):
    jobs = tail_jobs()
    bufs, ask, counts = submit(hip, jobs, device)
    check(hip, "tails", bufs, ask)
    assert counts == ((1, 9) if not device else (4, 6)), counts


# ---- 5. outputs absent, ids -------------------------------------------------------------------------------------------

def test_outputs_left_out(hip):
    """device form: end_out absent, then the bitmap absent, each beside a job that asks for both; host form without bitmaps"""
    jobs = [job1500(k) for k in ("lds_full", "dying", "lds_mid", "dying", "glob_first")]
    ask = [("end", "bm"), ("bm",), ("end", "bm"), ("end",), ("bm",)]
    bufs, ask, counts = submit(hip, jobs, True, ask=ask)
    check(hip, "device, outputs absent", bufs, ask)
    assert counts == (2, 4), counts
    bufs, ask, counts = submit(hip, jobs, False, ask=("end",))
    check(hip, "host, no bitmap", bufs, ask)
    assert counts == (1, 5), counts
    bufs, ask, counts = submit(hip, jobs, False, ask=[("end", "bm"), ("bm",), ("end",), ("end", "bm"), ("bm",)])
    check(hip, "host, outputs absent", bufs, ask)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_end_ids_in_every_mode(hip, device):
    """dying has one to three ids per end state, so EARLIEST and RET differ; lds_full has none (NO_ID under EARLIEST);
    FSM_HIP_IDS_ERROR refuses a submission that holds dying before anything is written, and the next call answers"""
    dy = job1500("dying")
    assert {len(G.endids_of(dy.a.flat, s)) for s in set(dy.end[dy.end != NO].tolist())} == {1, 2, 3}
    jobs = [job1500("lds_full"), dy, job1500("dying_glob")]
    everything = ("end", "bm", "ids")
    bufs, ask, counts = submit(hip, jobs, device, ask=everything, ids_mode=EARLIEST)
    check(hip, "earliest", bufs, ask, EARLIEST)
    assert counts == ((1, 3) if not device else (2, 2)), counts
    bufs, ask, _ = submit(hip, jobs[1:], device, ask=[everything, ("ids",)], ids_mode=RET)
    check(hip, "ret", bufs, ask, RET)
    bufs = [Bufs(hip, j, device) for j in jobs]
    refused(lambda: submit(hip, jobs, device, ask=everything, ids_mode=IDS_ERROR, bufs=bufs))
    check(hip, "refused: IDS_ERROR", bufs, [()] * 3)
    refused(lambda: submit(hip, jobs, device, ask=everything, ids_mode=7, bufs=bufs))
    check(hip, "refused: no such mode", bufs, [()] * 3)
    bufs, ask, _ = submit(hip, jobs, device, ask=everything, ids_mode=EARLIEST, bufs=bufs)
    check(hip, "the call after", bufs, ask, EARLIEST)
    # IDS_ERROR is EARLIEST where no automaton that is asked for ids has a conflict
    bufs, ask, _ = submit(hip, jobs[:2], device, ask=[everything, ("end", "bm")], ids_mode=IDS_ERROR)
    check(hip, "IDS_ERROR without a conflict", bufs, ask, EARLIEST)


# ---- 6. fuse limits, host front ----------------------------------------------------------------------------------------

def test_fuse_limit_lines(hip):
    """65 536 lines ride in the fused launch, 65 537 go through the dfa's own walk"""
    rng = np.random.RandomState(65536)
    rows = rng.randint(0, 256, (65537, 3)).astype(np.uint8)
    lens = rng.randint(0, 4, 65537)
    for n, fused in ((65536, 1), (65537, 0)):
        j = Job("lds_full", rows[:n], lens[:n])
        assert 100 < int((j.end != NO).sum()) < n - 100
        bufs, ask, counts = submit(hip, [j], False)
        check(hip, "n = %d" % n, bufs, ask)
        assert counts == (1, fused), (n, counts)


@functools.lru_cache(maxsize=None)
def mib_jobs():
    rows = np.random.RandomState(1024).randint(0, 256, (1025, 1024)).astype(np.uint8)
    lens = np.full(1025, 1024)
    lens[1024] = 1
    return Job("lds_full", rows[:1024], lens[:1024]), Job("lds_full", rows, lens)


def test_fuse_limit_bytes_and_table(hip):
    """1 MiB of lines fuses, one byte more does not; a plain table of 1 MiB fuses, one row more does not"""
    exact, over = mib_jobs()
    assert int(exact.off[-1]) == 1 << 20 and int(over.off[-1]) == (1 << 20) + 1
    for j, fused in ((exact, 1), (over, 0)):
        bufs, ask, counts = submit(hip, [j], False)
        check(hip, "%d bytes" % int(j.off[-1]), bufs, ask)
        assert counts == (1, fused), counts
    jobs = [job1500("glob_1mib"), job1500("glob_over")]
    p = assert_shape(hip, "glob_1mib")
    assert p.S1 * p.C * 4 == 1 << 20
    for order in (jobs, jobs[::-1]):
        bufs, ask, counts = submit(hip, order, False)
        check(hip, "1 MiB table", bufs, ask)
        assert counts == (2, 1), counts
    bufs, ask, counts = submit(hip, jobs[:1], False)
    assert counts == (1, 1), counts
    bufs, ask, counts = submit(hip, jobs[1:], False)
    assert counts == (1, 0), counts
    check(hip, "glob_over alone", bufs, ask)


def test_staging_cap(hip):
    """66 jobs on ONE glob_1mib handle stage 1 MiB of table each: what does not fit 64 MiB goes the per-dfa way.  (The split
    itself is the planner's arithmetic and is not asserted.)  32 such jobs fuse; the eleven automata right behind, with the
    block at its largest, are right again"""
    K = 66
    rng = np.random.RandomState(66)
    jobs = [Job("glob_1mib", rng.randint(0, 256, (3, 40)).astype(np.uint8), rng.randint(1, 41, 3)) for _ in range(K)]
    assert len({tuple(j.end.tolist()) for j in jobs}) > 4
    bufs, ask, (launches, fused) = submit(hip, jobs, False)
    print("staging cap: %d of %d jobs fused, %d launches" % (fused, K, launches))
    check(hip, "66 x 1 MiB", bufs, ask)
    assert 1 <= fused < K and launches == 1 + (K - fused), (launches, fused)
    bufs, ask, counts = submit(hip, jobs[:32], False)
    check(hip, "32 x 1 MiB", bufs, ask)
    assert counts == (1, 32), counts
    small = [job1500(name) for name in ALL]
    bufs, ask, counts = submit(hip, small, False)
    check(hip, "the eleven behind the largest block", bufs, ask)
    assert counts == (2, 10), counts


# ---- 7. eager on long lines --------------------------------------------------------------------------------------------

EAGER = ("eager40", "eager100", "eager100_glob", "dying")


def test_eager_sets_on_ragged_long_lines(hip):
    """W = 1, W = 2 in the LDS form, W = 2 in the global-table form and an automaton that emits nothing (eager_out given), in one
    submission with end states, bitmaps and ids: host, device, prepared (twice, new bytes)"""
    jobs = [job1500(name, 0, True) for name in EAGER]
    assert all(j.em is not None for j in jobs[:3]) and jobs[3].em is None
    assert float((jobs[0].em.sum(axis=1) >= 2).mean()) > 0.5
    everything = KEYS
    bufs, ask, counts = submit(hip, jobs, False, ask=everything, ids_mode=EARLIEST)
    check(hip, "eager host", bufs, ask)
    assert counts == (1, 4), counts
    bufs, ask, counts = submit(hip, jobs, True, ask=everything, ids_mode=EARLIEST)
    check(hip, "eager device", bufs, ask)
    assert counts == (2, 3), counts
    for b in bufs:
        b.junk()
    pr = hip.MultiPrepared([dfa(hip, j.name) for j in jobs], tuples(bufs, ask, 7), EARLIEST)
    pr.launch()
    check(hip, "eager prepared", bufs, ask)
    assert (hip.multi_last_launches(), hip.multi_last_fused_jobs()) == (2, 3)
    for b, name in zip(bufs, EAGER):
        b.put_text(job1500(name, 1, True))
        b.junk()
    pr.launch()
    check(hip, "eager prepared, new bytes", bufs, ask)
    pr.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_two_kernels_agree_with_the_reference_on_the_same_jobs(hip, device):
    """the eleven plain jobs through the eager entry point: no job asking (walk_multi runs) and exactly one job asking
    (walk_multi_eager runs for all of them).  Both against the reference: this is what holds the two kernels together"""
    jobs = [job1500(name, 0, name == "eager40") for name in ALL]
    counts_want = (2, 10) if not device else (6, 6)
    bufs, ask, counts = submit(hip, jobs, device, ask=("end", "bm"), width=7)
    check(hip, "no job asks", bufs, ask)
    assert counts == counts_want, counts
    ask = [("end", "bm", "sets") if j.name == "eager40" else ("end", "bm") for j in jobs]
    bufs, ask, counts = submit(hip, jobs, device, ask=ask)
    check(hip, "one job asks", bufs, ask)
    assert counts == counts_want, counts


# ---- 8. the context ----------------------------------------------------------------------------------------------------

def _regrow_behind_a_device_launch():
    """(a fresh process: the staging block is still small)  a device submission of the six LDS automata on a stream and, with no
    synchronise in between, a host submission of 1 MiB of lines, which must free and reallocate the block the launch reads"""
    import torch
    import libfsm_amd as hip
    torch.cuda.set_device(0)
    hip.load_library()
    big = []
    for k, name in enumerate(LDS):
        rows, lens = ragged(20000, 800 + k)
        big.append(Job(name, rows, lens))
    exact, _ = mib_jobs()
    bufs = [Bufs(hip, j, True) for j in big]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    _, ask, counts = submit(hip, big, True, stream=st.cuda_stream, bufs=bufs)
    hbufs, hask, hcounts = submit(hip, [exact], False)
    assert counts == (1, 6) and hcounts == (1, 1), (counts, hcounts)
    check(hip, "host behind device", hbufs, hask)
    check(hip, "device before host", bufs, ask)
    for d in _dfas.values():
        d.close()
    print("regrow ok")


def test_host_submission_regrows_the_block_behind_a_device_launch(hip):
    env = dict(os.environ)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "regrow"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "regrow ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_two_threads_submit_at_once(hip):
    """two host threads, twenty submissions each, different automata: one staging block behind a mutex"""
    names = (("lds_full", "dying", "eager40", "glob_1mib"), ("lds_wide", "lds_mid", "glob_first", "dying_glob"))
    for t in names:
        for name in t:
            dfa(hip, name)
            job1500(name)
    errors = []

    def work(mine):
        try:
            for r in range(20):
                jobs = [job1500(mine[(r + k) % 4]) for k in range(1 + r % 4)]
                bufs, ask, _ = submit(hip, jobs, False)          # (the counters are the process's: not read here)
                check(hip, "thread, round %d" % r, bufs, ask)
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    ts = [threading.Thread(target=work, args=(m,)) for m in names]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


# ---- 9. refusals, host front ------------------------------------------------------------------------------------------

def test_refusals(hip):
    import ctypes as C
    good, other = job1500("lds_full"), job1500("dying")
    d = [dfa(hip, "lds_full"), dfa(hip, "dying")]

    def fresh():
        return [Bufs(hip, good, False), Bufs(hip, other, False)]

    def call(bufs, dfas=d, patch=None):
        t = tuples(bufs, [("end", "bm")] * 2, 5)
        if patch:
            t[1] = patch(t[1])
        hip.exec_multi_ptrs(dfas, t, 0, False)

    def answers():
        bufs, ask, counts = submit(hip, [good, other], False)
        check(hip, "the call after", bufs, ask)
        assert counts == (1, 2)

    # a decreasing offset in the second job
    bufs = fresh()
    off = other.off.copy()
    off[700] = off[699] - np.uint64(1)
    refused(lambda: call(bufs, patch=lambda t: (t[0], off.ctypes.data) + t[2:]))
    check(hip, "decreasing offset", bufs, [()] * 2)
    answers()
    # base NULL with off[n] != 0
    bufs = fresh()
    refused(lambda: call(bufs, patch=lambda t: (0,) + t[1:]))
    check(hip, "no base", bufs, [()] * 2)
    answers()
    # a NULL dfa in the array
    bufs = fresh()
    refused(lambda: call(bufs, dfas=[d[0], None]))
    check(hip, "NULL dfa", bufs, [()] * 2)
    answers()
    # k = 0
    assert hip.multi_last_launches() == 1 and hip.multi_last_fused_jobs() == 2
    hip.exec_multi_ptrs([], [], 0, False)
    assert (hip.multi_last_launches(), hip.multi_last_fused_jobs()) == (0, 0)
    answers()
    # fsm_hip_multi_launch(NULL)
    lib = hip.load_library()
    C.set_errno(0)
    assert lib.fsm_hip_multi_launch(None, None) == -1 and C.get_errno() == errno.EINVAL
    # a prepared submission of jobs without lines launches nothing
    pr = hip.MultiPrepared(d, [(0, 0, 0, 0, 0, 0)] * 2, 0)
    pr.launch()
    assert (hip.multi_last_launches(), hip.multi_last_fused_jobs()) == (0, 0)
    pr.close()
    answers()


if __name__ == "__main__":
    assert sys.argv[1:] == ["regrow"]
    _regrow_behind_a_device_launch()
