"""GPU (-m gpu): eager-output sets from the many-DFA front's fused launch (fsm_hip_exec_multi_eager[_device],
fsm_hip_multi_prepare_eager).  Every set and end state is compared with the reference's own frozen answers (tests/golden/eager)
or with the oracle's fsm_exec + callback (oracle.pyoracle.Oracle.exec_eager) directly, never with another HIP front; end-ids
with the contract of FSM_HIP_IDS_EARLIEST worked out from the flat description."""
import os

import numpy as np
import pytest

from common import GOLDEN, Golden, all_golden_paths, eager_golden_paths

pytestmark = pytest.mark.gpu
NO = 0xFFFFFFFF
NO_ID = 0xFFFFFFFE
EARLIEST = 1
LOWER = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)
JUNK32, JUNK64 = 0x77777777, 0x7777777777777777     # what the outputs hold before a launch: every word must be overwritten


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()   # raises if the HIP extension is missing: no silent fallback
    return libfsm_amd


def _eager40(hip):
    z = np.load(os.path.join(GOLDEN, "bench", "eager40.npz"))
    return hip.FlatDfa.load(z), bytes(z["patterns"]).split(b"\n")


def _union150(hip):
    """fsm_union_repeated_pattern_group over 150 unanchored literals of 6-8 letters: 150 eager ids, W = 3 (the automaton of
    tests/test_gpu_eager_stream.py:_union150).  oracle/_ref is made by build(); without it this case is not covered."""
    from oracle.pyoracle import RefFsm, have_ref
    assert have_ref(), "oracle/_ref is missing: build() makes it where the reference tree is, and it travels with the tree"
    rng = np.random.RandomState(150)
    words = []
    while len(words) < 150:
        w = bytes(LOWER[rng.randint(0, 26, rng.randint(6, 9))])
        if w not in words:
            words.append(w)
    return RefFsm.union_repeated("pcre", words, 1, False).flatten(), words


def _wide_small(hip):
    """107 eager ids (W = 2) on a table that fits the fused kernel's LDS copy (101 states x 101 classes): byte v of 32..131 leads
    from every state to state v - 31, which emits 1000 + v and 2000 + v % 7; any other byte is a missing edge"""
    nt = np.full((101, 256), -1, np.int64)
    nt[:, 32:132] = np.arange(1, 101)
    eo = np.zeros(102, np.uint32)
    eo[2:] = 2 * np.arange(1, 101)
    ei = np.array([[2000 + v % 7, 1000 + v] if 2000 + v % 7 < 1000 + v else [1000 + v, 2000 + v % 7] for v in range(32, 132)], np.uint32).reshape(-1)
    return hip.FlatDfa.from_dense(nt, 0, [0] + [1] * 100, eager_off=eo, eager_ids=ei)


def _want_ids(flat, end):
    """FSM_HIP_IDS_EARLIEST: the lowest id of the end state, NO_ID for an end state without ids, NO_MATCH for a rejected input"""
    out = np.full(len(end), NO, np.uint32)
    for i, e in enumerate(end):
        if e != NO:
            ids = flat.endids_of(int(e))
            out[i] = int(ids.min()) if len(ids) else NO_ID
    return out


def _random_planted(g, rng, n=500, L=64):
    """random lines over the patterns' own letters, a whole pattern planted in one line of five (tests/test_gpu_parity.py:556-562)"""
    alpha = np.frombuffer((" ".join(g.meta["patterns"]) + " xyz$^").encode("latin1"), np.uint8)
    rnd = alpha[rng.randint(0, len(alpha), (n, L))]
    for i in range(0, n, 5):
        p = g.meta["patterns"][rng.randint(len(g.meta["patterns"]))].encode("latin1").strip(b"^$")
        if 0 < len(p) <= 40 and not any(c in p for c in b"[]()*+?|\\."):
            at = rng.randint(0, L - len(p))
            rnd[i, at:at + len(p)] = np.frombuffer(p, np.uint8)
    return rnd


class Case:
    """one job: an automaton, its lines (rows + lengths), whether it asks for eager_out; the oracle's answers"""

    def __init__(self, name, flat, rows, lens=None, eager=True, cap=256):
        from oracle.pyoracle import Oracle
        self.name, self.flat, self.eager = name, flat, eager
        rows = np.ascontiguousarray(rows, np.uint8)
        self.n = len(rows)
        self.lens = np.full(self.n, rows.shape[1], np.uint32) if lens is None else np.asarray(lens, np.uint32)
        self.strs = [bytes(rows[i, :self.lens[i]]) for i in range(self.n)]
        if self.n:
            _, self.end, self.sets = Oracle(flat).exec_eager(rows, self.lens, cap=cap)
        else:
            self.end, self.sets = np.zeros(0, np.uint32), []
        self.ids = _want_ids(flat, self.end)
        self.off = np.zeros(self.n + 1, np.uint64)
        self.off[1:] = np.cumsum(self.lens)
        self.base = np.frombuffer(b"".join(self.strs), np.uint8)

    def check(self, what, end, bitmap, ids, sets):
        assert np.array_equal(end, self.end), (what, self.name, "end")
        bits = np.unpackbits(np.ascontiguousarray(bitmap).view(np.uint8), bitorder="little")[:self.n].astype(bool)
        assert np.array_equal(bits, self.end != NO), (what, self.name, "bitmap")
        assert np.array_equal(ids, self.ids), (what, self.name, "ids")
        if self.eager:
            assert len(sets) == self.n
            for i in range(self.n):
                assert np.array_equal(sets[i], self.sets[i]), (what, self.name, i, sets[i], self.sets[i])
        else:
            assert sets is None


class DeviceJobs:
    """the cases as device-pointer jobs: exactly-sized text buffers (no padding behind the last line), outputs filled with junk"""

    def __init__(self, hip, cases):
        import torch
        self.torch, self.cases = torch, cases
        self.dfas = [hip.HipDfa(c.flat, hip.DEFER_UPLOAD) for c in cases]
        self.buf, self.jobs = [], []
        for c, d in zip(cases, self.dfas):
            W = d.eager_words()
            tb = torch.from_numpy(c.base.copy()).cuda() if len(c.base) else torch.zeros(1, dtype=torch.uint8, device="cuda")
            to = torch.from_numpy(c.off.astype(np.int64)).cuda()
            te = torch.empty(max(c.n, 1), dtype=torch.int32, device="cuda")
            ti = torch.empty(max(c.n, 1), dtype=torch.int32, device="cuda")
            tm = torch.empty(max((c.n + 63) // 64, 1), dtype=torch.int64, device="cuda")
            ts = torch.empty(max(c.n * W, 1), dtype=torch.int64, device="cuda") if c.eager else None
            self.buf.append((tb, to, te, ti, tm, ts))
            self.jobs.append((tb.data_ptr(), to.data_ptr(), c.n, te.data_ptr(), tm.data_ptr(), ti.data_ptr(), ts.data_ptr() if c.eager else 0))
        self.junk()

    def junk(self):
        for tb, to, te, ti, tm, ts in self.buf:
            te.fill_(JUNK32)
            ti.fill_(JUNK32)
            tm.fill_(JUNK64)
            if ts is not None:
                ts.fill_(JUNK64)

    def check(self, what):
        self.torch.cuda.synchronize()
        for c, d, (tb, to, te, ti, tm, ts) in zip(self.cases, self.dfas, self.buf):
            W = d.eager_words()
            sets = d.decode_eager(ts.cpu().numpy().view(np.uint64)[:c.n * W]) if c.eager else None
            c.check(what, te.cpu().numpy().view(np.uint32)[:c.n], tm.cpu().numpy().view(np.uint64)[:(c.n + 63) // 64],
                    ti.cpu().numpy().view(np.uint32)[:c.n], sets)

    def close(self):
        for d in self.dfas:
            d.close()


def _host(hip, cases, what):
    dfas = [hip.HipDfa(c.flat, hip.DEFER_UPLOAD) for c in cases]
    outs = hip.exec_multi_eager(dfas, [c.strs for c in cases], EARLIEST, want_eager=[c.eager for c in cases])
    launches, fused = hip.multi_last_launches(), hip.multi_last_fused_jobs()
    for c, (end, bm, ids, sets) in zip(cases, outs):
        c.check(what, end, bm, ids, sets)
    for d in dfas:
        d.close()
    return launches, fused


def test_reference_eager_corpus_in_one_submission(hip):
    """the 22 automata of the reference's tests/eager_output programs with their own 89 lines: ONE fsm_hip_exec_multi_eager
    with DEFER_UPLOAD dfas, one fused launch; end states and id sets as the reference froze them"""
    gs = [Golden(p) for p in eager_golden_paths()]
    assert len(gs) == 22 and sum(len(g.strings()) for g in gs) == 89
    dfas = [hip.HipDfa(g.flat, hip.DEFER_UPLOAD) for g in gs]
    outs = hip.exec_multi_eager(dfas, [g.strings() for g in gs], EARLIEST)
    assert hip.multi_last_launches() == 1 and hip.multi_last_fused_jobs() == 22
    for g, (end, bm, ids, sets) in zip(gs, outs):
        assert np.array_equal(end, g.end), g.name
        assert np.array_equal(ids, _want_ids(g.flat, g.end)), g.name
        bits = np.unpackbits(bm.view(np.uint8), bitorder="little")[:len(end)].astype(bool)
        assert np.array_equal(bits, g.end != NO), g.name
        for i in range(len(end)):
            assert np.array_equal(sets[i], np.sort(g.eager_of(i))), (g.name, i)
    for d in dfas:
        d.close()


def _mixed_cases(hip):
    rng = np.random.RandomState(2024)
    gs = [Golden(p) for p in eager_golden_paths()]
    cases = [Case(g.name, g.flat, _random_planted(g, rng)) for g in gs]
    g0, g1, g2 = gs[16], gs[5], gs[6]                           # 3, 10 and 26 eager ids
    assert all(g.flat.eager_off is not None for g in (g0, g1, g2))
    cases.append(Case("n = 0", g0.flat, np.zeros((0, 16), np.uint8)))
    ragged = _random_planted(g1, rng, 300, 64)
    lens = rng.randint(0, 65, 300)
    lens[::7] = 0                                               # empty lines: the start state's outputs alone
    cases.append(Case("empty and ragged lines", g1.flat, ragged, lens))
    cases.append(Case("256 lines", g2.flat, _random_planted(g2, rng, 256, 64)))
    cases.append(Case("257 lines", g2.flat, _random_planted(g2, rng, 257, 64)))
    cases.append(Case("eager_out NULL", g1.flat, _random_planted(g1, rng, 300, 64), eager=False))
    r = Golden([p for p in all_golden_paths() if "/retest/" in p][0])
    assert r.flat.eager_off is None
    seeds = r.strings() or [b"a"]
    rows = rng.randint(97, 123, (200, 24)).astype(np.uint8)
    for i in range(0, 200, 2):
        sd = seeds[rng.randint(len(seeds))][:24]
        rows[i, :len(sd)] = np.frombuffer(sd, np.uint8)
    cases.append(Case("no eager outputs, eager_out given", r.flat, rows))
    # the last job of the submission: its last line ends at the batch's last byte, off a 16-byte boundary
    tail = _random_planted(g0, rng, 100, 64)
    tl = np.full(100, 64)
    tl[-1] = 13
    cases.append(Case("last line ends the buffer", g0.flat, tail, tl))
    return cases


def test_random_and_planted_lines_host_device_prepared(hip):
    """500 random x 64 B lines per eager golden (patterns planted in one of five) beside the edge jobs -- n = 0, empty and ragged
    lines, 256 and 257 lines, a job without eager_out, an automaton without eager outputs, a last line that ends at the buffer's
    last byte -- through the host form, the device form and the prepared form; everything against Oracle.exec_eager"""
    cases = _mixed_cases(hip)
    nz = sum(1 for c in cases if c.n)
    assert sum(len(s) for c in cases if c.eager for s in c.sets) > 1000          # outputs do fire
    launches, fused = _host(hip, cases, "host")
    assert (launches, fused) == (1, nz)
    dj = DeviceJobs(hip, cases)
    hip.exec_multi_eager_device(dj.dfas, dj.jobs, EARLIEST)
    dj.check("device")
    assert hip.multi_last_launches() == 1 and hip.multi_last_fused_jobs() == nz
    dj.junk()
    pr = hip.MultiPrepared(dj.dfas, dj.jobs, EARLIEST)
    pr.launch()
    dj.check("prepared")
    assert hip.multi_last_launches() == 1 and hip.multi_last_fused_jobs() == nz
    pr.close()
    dj.close()


def _lines(rng, pats, n, L=64, every=5):
    rows = LOWER[rng.randint(0, 26, (n, L))]
    for i in range(0, n, every):
        p = pats[rng.randint(len(pats))]
        at = rng.randint(0, L - len(p) + 1)
        rows[i, at:at + len(p)] = np.frombuffer(p, np.uint8)
    return rows


def test_lds_form_at_size(hip):
    """eager40 (354 states x 27 classes: the LDS form) over 30 000 lines of 64 B, a pattern in one line of five: the device
    form, one launch, every set and end state against the oracle"""
    flat, pats = _eager40(hip)
    c = Case("eager40 x 30000", flat, _lines(np.random.RandomState(40), pats, 30000))
    assert sum(1 for s in c.sets if len(s)) >= 6000
    dj = DeviceJobs(hip, [c])
    info = dj.dfas[0].info()
    assert info["nstates"] == 354 and (info["nstates"] + 1) * info["nclasses"] < 10000
    hip.exec_multi_eager_device(dj.dfas, dj.jobs, EARLIEST)
    dj.check("eager40")
    assert hip.multi_last_launches() == 1 and hip.multi_last_fused_jobs() == 1
    dj.close()


def test_wide_sets(hip):
    """More than 64 ids, host form and device form against the oracle.
    - the 150-literal union (W = 3; 1 673 x 27 = 45 171 table entries): the host form fuses it (a table of up to 1 MiB: the
      global-table path of the fused kernel, the sets in the line's own words); the device forms fuse tables of up to 16 384
      entries, so there it goes through its dfa's own walk with eager_out passed through -- a second launch;
    - a 107-id automaton (W = 2) on a 101 x 101 table: fused in both forms (the LDS form with wide sets);
    - the eager40 job beside them rides in the same fused launch with its one-word sets."""
    flat, words = _union150(hip)
    f40, pats = _eager40(hip)
    fs = _wide_small(hip)
    rng = np.random.RandomState(151)
    rows = _lines(rng, words, 2000, 64, 3)
    for i in range(0, 2000, 6):                              # several ids in one line, from different words of the set
        for w in (words[rng.randint(0, 50)], words[rng.randint(100, 150)]):
            at = rng.randint(0, 64 - len(w) + 1)
            rows[i, at:at + len(w)] = np.frombuffer(w, np.uint8)
    lens = np.full(2000, 64)
    lens[1::9] = rng.randint(0, 64, len(lens[1::9]))
    srows = rng.randint(32, 132, (1500, 48)).astype(np.uint8)
    srows[::11, 20] = 7                                      # a missing edge in mid-line: nothing fires after it
    slens = rng.randint(0, 49, 1500)
    cases = [Case("union150", flat, rows, lens), Case("eager40 beside it", f40, _lines(rng, pats, 300)), Case("107 ids, LDS form", fs, srows, slens)]
    assert max(len(s) for s in cases[0].sets) >= 2 and len(set(np.concatenate(cases[0].sets).tolist())) > 128
    assert len(set(np.concatenate(cases[2].sets).tolist())) == 107
    for f, W in ((flat, 3), (fs, 2)):
        d = hip.HipDfa(f, hip.DEFER_UPLOAD)
        assert d.eager_words() == W
        d.close()
    assert _host(hip, cases, "wide host") == (1, 3)
    dj = DeviceJobs(hip, cases)
    hip.exec_multi_eager_device(dj.dfas, dj.jobs, EARLIEST)
    dj.check("wide device")
    assert hip.multi_last_launches() == 2 and hip.multi_last_fused_jobs() == 2
    dj.close()


def test_big_job_beside_the_fused_launch(hip):
    """a 200 000-line job on the eager40 table in a host submission with the 22 small ones: it goes through its dfa's own walk
    with eager_out passed through (two launches), the 22 ride in the fused one; sets right for all"""
    gs = [Golden(p) for p in eager_golden_paths()]
    flat, pats = _eager40(hip)
    cases = []
    for g in gs:
        rows, lens = g.padded_rows()
        cases.append(Case(g.name, g.flat, rows, lens))
    for g, c in zip(gs, cases):                                 # the oracle agrees with what the reference froze
        assert all(np.array_equal(c.sets[i], np.sort(g.eager_of(i))) for i in range(c.n)), g.name
    cases.insert(5, Case("eager40 x 200000", flat, _lines(np.random.RandomState(41), pats, 200000)))
    launches, fused = _host(hip, cases, "big beside small")
    assert (launches, fused) == (2, 22)


def test_prepared_form_replays_from_a_hip_graph(hip):
    """fsm_hip_multi_prepare_eager + fsm_hip_multi_launch captured into a HIP graph and replayed on new bytes in the same
    buffers (as tests/test_gpu_round6.py does for the plain outputs): planted text, then pattern-free text -- whose sets must
    be all zero, W = 1 and W = 2 alike: the result is overwritten, never OR-ed into -- then planted text again"""
    import torch
    f40, pats = _eager40(hip)
    fw = _wide_small(hip)
    g = Golden(eager_golden_paths()[5])
    n, L = 700, 64
    rng = np.random.RandomState(77)

    def rows_for(k, rep):
        if rep == 1:                                            # nothing a pattern could match: '#' (eager40), a byte without an edge
            return np.full((n, L), ord("#") if k == 0 else 200, np.uint8) if k != 2 else rng.randint(0, 10, (n, L)).astype(np.uint8)
        return _lines(rng, pats, n) if k == 0 else rng.randint(32, 132, (n, L)).astype(np.uint8) if k == 1 else _random_planted(g, rng, n, L)

    flats = [f40, fw, g.flat]
    first = [Case("job %d" % k, flats[k], rows_for(k, 0)) for k in range(3)]
    dj = DeviceJobs(hip, first)
    pr = hip.MultiPrepared(dj.dfas, dj.jobs, EARLIEST)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        pr.launch(st.cuda_stream)
        st.synchronize()
        assert hip.multi_last_launches() == 1 and hip.multi_last_fused_jobs() == 3
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            pr.launch(st.cuda_stream)
    dj.check("prepared, before capture")
    for rep in range(3):
        cases = first if rep == 0 else [Case("job %d rep %d" % (k, rep), flats[k], rows_for(k, rep)) for k in range(3)]
        if rep == 1:
            assert all(len(s) == 0 for c in cases[:2] for s in c.sets)
        else:
            assert all(sum(1 for s in c.sets if len(s)) > 100 for c in cases[:2])
        for c, (tb, to, te, ti, tm, ts) in zip(cases, dj.buf):
            tb.copy_(torch.from_numpy(c.base.copy()))
        if rep != 1:
            dj.junk()                                           # rep 1 keeps the sets of rep 0 in the buffers: they must go
        else:
            for tb, to, te, ti, tm, ts in dj.buf:
                te.fill_(JUNK32)
        dj.cases = cases
        torch.cuda.synchronize()
        gr.replay()
        dj.check("replay %d" % rep)
        if rep == 1:
            for tb, to, te, ti, tm, ts in dj.buf[:2]:
                assert int(ts.abs().max()) == 0
    pr.close()
    dj.close()
