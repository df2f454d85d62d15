"""GPU (-m gpu): the lifecycles of the handles whose device memory, pinned memory, events and streams are owned by type
(libfsm_amd/csrc/hip_host.h): a handle is made to build everything it can own, answers, and goes -- again and again.

The suite's other tests create a handle, use one front and let it go.  Here a single-DFA handle walks from host memory (arena
and pinned stage), through the lengths-only device front at growing sizes (the tile-base block is outgrown, so an old block
waits for the handle to go), delivers end-ids in two modes, resumes a walk, delivers eager sets and the eager stream, and is
freed; deferred handles go unused; the pair-table automaton goes with its second image; the file engine, the many-DFA staging
block, a prepared submission and the node come and go likewise.  No call here is made to fail on the device: the failure
paths are tests/c/test_hip_host.cpp's (stand-ins, on the CPU).

Every answer is judged by tests/global_ref.py alone -- the automaton's closed formula byte by byte in numpy -- never by
another front or handle.  What a leak or a double release would show as is the device's or the allocator's complaint, or a
later answer that is wrong; the answers are therefore checked in every cycle."""
import errno
import functools
import time

import numpy as np
import pytest

import global_ref as G
from eager_front_ref import words_of

pytestmark = pytest.mark.gpu

NO = 0xFFFFFFFF
CYCLES = 20
N_SMALL, N_MID, L = 257, 70_000, 64
# tb_bytes_for(70 000) is 8 776 bytes and the tile-base block starts at 64 KiB, so that batch does not outgrow it; one of
# 600 000 lines (75 024 bytes) does, and leaves the first block among the handle's old ones
N_BIG, L_BIG = 600_000, 8
# name -> (S, K, keyword arguments of global_ref.affine): the options tests/eager_front_ref.py uses, with end-ids and sinks
AUTOMATA = {
    "s15": (15, 4, dict(eager=40, every=3, endids=True, sinks=3)),
    "s200": (200, 4, dict(eager=40, endids=True, sinks=3)),
    "s1000": (1000, 4, dict(eager=100, endids=True, sinks=3)),
}


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()
    return libfsm_amd


def bits(bm, n):
    return np.unpackbits(bm.view(np.uint8), bitorder="little")[:n].astype(bool)


@functools.lru_cache(maxsize=None)
def inputs():
    """70 000 rows of 64 random bytes with lengths 0 .. 64 (the first 257 are the small batch), and 600 000 rows of 8"""
    rng = np.random.RandomState(257)
    rows = rng.randint(0, 256, (N_MID, L)).astype(np.uint8)
    lens = G.varlens(N_MID, L, rng)
    big = rng.randint(0, 256, (N_BIG, L_BIG)).astype(np.uint8)
    big_lens = rng.randint(0, L_BIG + 1, N_BIG).astype(np.uint32)
    for a in (rows, lens, big, big_lens):
        a.setflags(write=False)
    return rows, lens, big, big_lens


class Case:
    """one automaton and the reference's answers, computed once and left as they are"""

    def __init__(self, name):
        self.name = name
        self.S, self.K, self.kw = AUTOMATA[name]
        self.flat, self.dense, self.cls = G.affine(self.S, self.K, **self.kw)
        rows, lens, big, big_lens = inputs()
        small, slens = rows[:N_SMALL], lens[:N_SMALL]
        E, every = self.kw["eager"], self.kw.get("every", 11)
        ek = G.eager_ids_of_states(self.S, E, every)
        self.cols = np.unique(ek[ek >= 0])
        self.ids = (5 + 3 * self.cols).astype(np.uint32)        # bit b of a set is the b-th smallest id
        self.W = (len(self.cols) + 63) // 64
        st, em = G.walk_eager(self.dense, self.cls, 0, small, E, slens, every=every)
        self.end_small = G.ends(self.flat, st)
        self.words = words_of(em, self.cols, self.W)
        self.end_mid = G.ends(self.flat, G.walk(self.dense, self.cls, 0, rows, lens))
        self.end_big = G.ends(self.flat, G.walk(self.dense, self.cls, 0, big, big_lens))
        assert np.array_equal(self.end_mid[:N_SMALL], self.end_small)
        # resumed in two pieces of 32 bytes, every row whole
        self.carried_half = G.carried(G.walk(self.dense, self.cls, 0, small[:, :L // 2]))
        st_full = G.walk(self.dense, self.cls, 0, small)
        self.carried_full, self.end_full = G.carried(st_full), G.ends(self.flat, st_full)
        # end-ids: the lowest id of the end state; its whole set
        self.slots = G.endid_slots(self.S, self.flat.is_end.astype(bool))
        # the eager stream: the start state's ids at position 0, then the ids of every state entered, ascending within a state
        tr = G.trace(self.dense, self.cls, 0, small, slens)
        pair = np.sort(np.where(ek >= 0, 5 + 3 * ek, 1 << 40), axis=1)
        self.stream = []
        for i in range(N_SMALL):
            ids, pos = [], []
            for t in range(int(slens[i]) + 1):
                s = int(tr[i, t])
                assert s >= 0                                  # (no holes: nothing dies)
                for v in pair[s]:
                    if v < (1 << 40):
                        ids.append(int(v))
                        pos.append(t)
            self.stream.append((np.array(ids, np.uint32), np.array(pos, np.uint32)))
        self.cap = max(len(s[0]) for s in self.stream)
        assert self.cap >= 8 and (self.end_small != NO).any() and (self.end_small == NO).any() and self.words.any()

    def ids_of(self, s):
        return self.slots[s][self.slots[s] >= 0].astype(np.uint32)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def device_inputs():
    """the packed batches on the device, once: (bytes, lengths) of the 70 000 lines and of the 600 000"""
    import torch
    rows, lens, big, big_lens = inputs()
    out = []
    for r, ln in ((rows, lens), (big, big_lens)):
        base, _ = G.packed(r, ln)
        out.append((torch.from_numpy(np.concatenate([base, np.zeros(64, np.uint8)])).cuda(), torch.from_numpy(ln.astype(np.int32)).cuda()))
    return out


def granted(hip, flat):
    """the layout flags the planner grants this automaton (0 = its own choice); every other one is refused with ENOTSUP"""
    out = []
    for flag in (0,) + tuple(hip.ALL_LAYOUTS):
        try:
            hip.Plan(flat, flag)
        except OSError as e:
            assert e.errno == errno.ENOTSUP, (flag, e)
            continue
        out.append(flag)
    return out


# ---- (a) the full cycle, per layout flag ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(AUTOMATA))
def test_full_cycle_per_layout(hip, name):
    import torch
    c = case(name)
    rows, lens, _, _ = inputs()
    small, slens = np.ascontiguousarray(rows[:N_SMALL]), lens[:N_SMALL]
    (d_mid, d_mid_len), (d_big, d_big_len) = device_inputs()
    d_end = torch.empty(N_BIG, dtype=torch.int32, device="cuda")
    START = np.full(N_SMALL, hip.STATE_START, np.uint32)
    flags = granted(hip, c.flat)
    assert len(flags) >= 6, flags
    t0 = time.perf_counter()
    for flag in flags:
        for cycle in range(CYCLES):
            tag = (name, flag, cycle)
            dfa = hip.HipDfa(c.flat, flag)
            assert [dfa.eager_id(b) for b in range(dfa.eager_id_count())] == c.ids.tolist() and dfa.eager_words() == c.W, tag
            # host walk: the arena and the pinned stage
            end, bm = dfa.exec_batch(small, slens)
            assert np.array_equal(end, c.end_small) and np.array_equal(bits(bm, N_SMALL), c.end_small != NO), tag
            # lengths alone on the device, at growing sizes: the tile-base block, then a bigger one
            for n, base, ln, want in ((N_SMALL, d_mid, d_mid_len, c.end_mid), (N_MID, d_mid, d_mid_len, c.end_mid), (N_BIG, d_big, d_big_len, c.end_big)):
                d_end.fill_(0x5A5A5A5A)
                dfa.exec_batch_lengths_device(base.data_ptr(), ln.data_ptr(), n, d_end.data_ptr())
                torch.cuda.synchronize()
                got = d_end[:n].cpu().numpy().view(np.uint32)
                assert np.array_equal(got, want[:n]), tag + (n,)
            # end-ids, earliest and by set
            e1, e2 = dfa.exec_batch_ids(small, 1, slens), dfa.exec_batch_ids(small, 2, slens)
            hit = c.end_small != NO
            assert np.array_equal(e1 == NO, ~hit) and np.array_equal(e2 == NO, ~hit), tag
            assert np.array_equal(e1[hit], c.slots[c.end_small[hit].astype(np.int64), 0].astype(np.uint32)), tag
            sets = dfa.ret_sets()
            for s, k2 in set(zip(c.end_small[hit].tolist(), e2[hit].tolist())):
                assert k2 < len(sets) and np.array_equal(sets[k2], c.ids_of(s)), tag + (s, k2)
            # a resumed walk in two pieces
            st, _ = dfa.exec_batch_resume(np.ascontiguousarray(small[:, :L // 2]), START)
            assert np.array_equal(st, c.carried_half), tag
            st, end = dfa.exec_batch_resume(np.ascontiguousarray(small[:, L // 2:]), st)
            assert np.array_equal(st, c.carried_full) and np.array_equal(end, c.end_full), tag
            # eager sets, and the eager stream
            end, words = dfa.exec_eager_words(small, slens)
            assert np.array_equal(end, c.end_small) and np.array_equal(words, c.words), tag
            end, cnt, stream = dfa.exec_batch_eager_trace(small, slens, cap=c.cap)
            assert np.array_equal(end, c.end_small) and cnt.tolist() == [len(s[0]) for s in c.stream], tag
            for i, ((gi, gp), (wi, wp)) in enumerate(zip(stream, c.stream)):
                assert np.array_equal(gi, wi) and np.array_equal(gp, wp), tag + (i,)
            dfa.close()
    print(f"{name}: {len(flags)} layout flags x {CYCLES} cycles in {time.perf_counter() - t0:.2f} s")


# ---- (b) deferred upload; the second image --------------------------------------------------------------------------------

def test_deferred_handles_go_unused_and_after_reserve_only(hip):
    for name in AUTOMATA:
        c = case(name)
        for flag in granted(hip, c.flat):
            for _ in range(5):
                hip.HipDfa(c.flat, flag | hip.DEFER_UPLOAD).close()          # nothing was ever uploaded
                dfa = hip.HipDfa(c.flat, flag | hip.DEFER_UPLOAD)
                dfa.reserve(N_MID)                                           # tables, tile-base block, id and resume tables; no walk
                dfa.close()
    # and a deferred handle still answers
    c = case("s200")
    rows, lens, _, _ = inputs()
    dfa = hip.HipDfa(c.flat, hip.DEFER_UPLOAD)
    end, _ = dfa.exec_batch(np.ascontiguousarray(rows[:N_SMALL]), lens[:N_SMALL])
    assert np.array_equal(end, c.end_small)
    dfa.close()


def test_pair_table_handle_goes_with_its_second_image(hip):
    flat, dense, cls = G.affine(2000, 4, endids=True, sinks=3)
    rng = np.random.RandomState(2000)
    rows = rng.randint(0, 256, (N_SMALL, 256)).astype(np.uint8)
    lens = G.varlens(N_SMALL, 256, rng)
    want_rows = G.ends(flat, G.walk(dense, cls, 0, rows))
    want_lens = G.ends(flat, G.walk(dense, cls, 0, rows, lens))
    assert (want_rows != NO).any() and (want_rows == NO).any()
    for cycle in range(5):
        dfa = hip.HipDfa(flat)
        assert dfa.info()["layout_name"] == "lds2", dfa.info()
        end, _ = dfa.exec_batch(rows)                                        # fixed stride: the pair table
        assert np.array_equal(end, want_rows) and "Lds2Pol" in dfa.last_kernel_name(), (cycle, dfa.last_kernel_name())
        end, _ = dfa.exec_batch(rows, lens)                                  # ragged: the second image
        name = dfa.last_kernel_name()
        assert np.array_equal(end, want_lens) and name and "Lds2Pol" not in name, (cycle, name)
        dfa.close()
    # ... also when nothing of either image was uploaded, and after a reserve alone
    hip.HipDfa(flat, hip.DEFER_UPLOAD).close()
    dfa = hip.HipDfa(flat, hip.DEFER_UPLOAD)
    dfa.reserve(N_SMALL)
    dfa.close()


# ---- (c) the file engine ----------------------------------------------------------------------------------------------------

WINDOW, PIECE = 32 << 20, 1024


def looping_block(dense, cls, nsink, rng):
    """PIECE bytes that lead state 0 back to state 0 past no sink: the file below is this block over and over, so the walk is
    still going at the end of every window (random bytes would be caught by a sink within a few dozen)"""
    S, K = dense.shape
    live = np.arange(S) < S - nsink
    can = np.zeros((PIECE + 1, S), bool)             # can[r][s]: state 0 is r steps from s, sinks avoided
    can[0, 0] = True
    for r in range(1, PIECE + 1):
        can[r] = live & can[r - 1][dense].any(axis=1)
    assert can[PIECE, 0]
    lo = np.array([np.nonzero(cls == k)[0][0] for k in range(K)])
    s, out = 0, np.zeros(PIECE, np.uint8)
    for i in range(PIECE):
        ks = [k for k in range(K) if can[PIECE - i - 1][dense[s, k]]]
        k = ks[rng.randint(len(ks))]
        out[i] = lo[k] + rng.randint(int((cls == k).sum()))
        s = int(dense[s, k])
    assert s == 0
    return out


def test_file_engine_plain_and_eager_over_three_windows(hip, tmp_path):
    S, K, kw = AUTOMATA["s15"]
    flat, dense, cls = G.affine(S, K, **kw)
    E, every = kw["eager"], kw["every"]
    rng = np.random.RandomState(3)
    block = looping_block(dense, cls, kw["sinks"], rng)
    tail = rng.randint(0, 256, 100).astype(np.uint8)
    # the reference: one block from state 0 ends in state 0, so three windows of blocks do; the answer is the tail's
    st, em = G.walk_eager(dense, cls, 0, block[None, :], E, every=every)
    assert int(st[0]) == 0
    st_t, em_t = G.walk_eager(dense, cls, 0, tail[None, :], E, every=every)
    want_end = int(G.ends(flat, st_t)[0])
    want_ids = (5 + 3 * np.nonzero(em[0] | em_t[0])[0]).astype(np.uint32)
    assert len(want_ids) >= 3
    path = tmp_path / "three_windows"
    with open(path, "wb") as f:
        for _ in range(3):
            f.write(np.tile(block, WINDOW // PIECE).tobytes())
        f.write(tail.tobytes())
    dfa = hip.HipDfa(flat)
    t0 = time.perf_counter()
    for _ in range(5):
        assert dfa.match_file(str(path)) == (want_end != NO)
        windows, passes = dfa.match_last_passes()
        assert windows == 3 and passes <= 6, (windows, passes)
        r, end, ids = dfa.match_file_eager(str(path))
        assert (r, end) == (int(want_end != NO), want_end) and np.array_equal(ids, want_ids), (r, end, ids)
        assert dfa.match_last_passes()[0] == 3
    print(f"file engine: 10 calls over {3 * WINDOW + 100} bytes in {time.perf_counter() - t0:.2f} s")
    # a path that does not exist: the call fails as it always did, and the next one answers
    for call in (dfa.match_file, dfa.match_file_eager):
        with pytest.raises(OSError) as ei:
            call(str(tmp_path / "no_such_file"))
        assert ei.value.errno == errno.ENOENT
    assert dfa.match_file(str(path)) == (want_end != NO)
    dfa.close()


# ---- (d) the many-DFA front -------------------------------------------------------------------------------------------------

def test_many_dfa_staging_regrown_and_a_prepared_submission_freed_in_flight(hip):
    import torch
    rows, lens, _, _ = inputs()
    names = list(AUTOMATA)
    dfas = [hip.HipDfa(case(n).flat, hip.DEFER_UPLOAD) for n in names]
    # host submissions of growing total bytes (three jobs of 257, 2 000 and 20 000 lines: about 25 KB, 190 KB and 1.9 MB of
    # lines beside the tables): in a process of its own the staging block starts at 64 KiB and is regrown for the 2nd and 3rd
    for n in (N_SMALL, 2_000, 20_000):
        lines = [bytes(rows[i, :lens[i]]) for i in range(n)]
        out = hip.exec_multi(dfas, [lines] * len(dfas))
        assert hip.multi_last_fused_jobs() == len(dfas)
        for name, (end, bm) in zip(names, out):
            want = case(name).end_mid[:n]
            assert np.array_equal(end, want) and np.array_equal(bits(bm, n), want != NO), (name, n)
    # a prepared submission launched and freed at once: the free waits for the launch, the outputs are the launch's
    n = 20_000
    base, off = G.packed(rows[:n], lens[:n])
    d_base = torch.from_numpy(np.concatenate([base, np.zeros(64, np.uint8)])).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_end = [torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in dfas]
    d_ids = [torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in dfas]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):
        pr = hip.MultiPrepared(dfas, [(d_base.data_ptr(), d_off.data_ptr(), n, e.data_ptr(), 0, i.data_ptr()) for e, i in zip(d_end, d_ids)], 1)
        pr.launch(stream.cuda_stream)
        pr.close()
        stream.synchronize()
        for name, e, i in zip(names, d_end, d_ids):
            c = case(name)
            want = c.end_mid[:n]
            hit = want != NO
            assert np.array_equal(e.cpu().numpy().view(np.uint32), want), name
            got = i.cpu().numpy().view(np.uint32)
            assert np.array_equal(got[hit], c.slots[want[hit].astype(np.int64), 0].astype(np.uint32)) and (got[~hit] == NO).all(), name
            e.fill_(0x5A5A5A5A)
            i.fill_(0x5A5A5A5A)
        torch.cuda.synchronize()
    for d in dfas:
        d.close()


# ---- (e) the node front -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [[0], [0, 0, 0]], ids=["one", "three_replicas"])
def test_node_create_walk_free(hip, devices, monkeypatch):
    """(a list of distinct devices gets RCCL communicators, half a second a create: the first cycle has them and destroys them
    before the streams go, the other nine exchange by peer copies -- the library reads FSM_HIP_NO_RCCL at every create)"""
    c = case("s200")
    rows, lens, _, _ = inputs()
    small, slens = np.ascontiguousarray(rows[:N_SMALL]), lens[:N_SMALL]
    for cycle in range(10):
        if cycle == 1:
            monkeypatch.setenv("FSM_HIP_NO_RCCL", "1")
        node = hip.HipNode(c.flat, devices)
        assert node.ndev == len(devices)
        end, bm = node.exec_batch(small, slens)
        assert np.array_equal(end, c.end_small) and np.array_equal(bits(bm, N_SMALL), c.end_small != NO), cycle
        node.close()


def test_node_refuses_a_device_out_of_range_and_the_next_create_works(hip, monkeypatch):
    import torch
    monkeypatch.setenv("FSM_HIP_NO_RCCL", "1")          # (the refusal comes before any communicator; the creates that follow need none)
    c = case("s200")
    rows, lens, _, _ = inputs()
    for devices in ([0, torch.cuda.device_count()], [-1], [0, 0, 64 + torch.cuda.device_count()]):
        with pytest.raises(OSError) as ei:
            hip.HipNode(c.flat, devices)
        assert ei.value.errno == errno.EINVAL, devices
        node = hip.HipNode(c.flat, [0])
        end, _ = node.exec_batch(np.ascontiguousarray(rows[:N_SMALL]), lens[:N_SMALL])
        assert np.array_equal(end, c.end_small)
        node.close()
