"""GPU (-m gpu): the multi-device front (libfsm_amd/csrc/node.hip) at its edges -- eager sets over the node, empty and
short shards on every host and device front, device end-ids in every mode, the asynchronous slots, fsm_hip_node_exec_multi
with fewer jobs than devices.  The judge is the oracle (oracle.pyoracle.Oracle: exec_stride, exec_strings, exec_eager,
endids) throughout, bit for bit, plus global_ref.walk_eager for the W = 2 automaton; nothing is compared with a
single-device HipDfa, and nothing needs oracle/_ref.

Automata
  c3      tests/golden/c3.npz: 1 024 anchored patterns ^<letters>[0-9]+(x|yz)$, end-ids (352 end states carry more than one),
          DEAD reachable
  eager40 tests/golden/bench/eager40.npz: 40 unanchored literals, one eager id each, W = 1
  wide    global_ref.affine(3000, 4, eager=100): the closed-formula automaton of global_ref.FAMILY's eager100 with 3 000 states
          instead of 65 534 (24 KB of table: five replicas are created in no time); 100 eager ids, W = 2
  lits    64 distinct literals anchored at both ends, one end-id each (100 + q): no end state carries two ids

Replica lists: [0], [0, 0], [0, 0, 0], [0] * 5 -- several replicas on one GPU, exchanged by peer copies; [0] takes RCCL with a
communicator of one -- and every visible device where there is more than one.  Per list of G replicas the batch sizes are
sizes(G); check_sizes() asserts from fsm_hip_node_shard that they reach an empty last shard, several empty shards (G >= 3),
a last shard of one input and a batch in which every shard is full (the branch that does not zero its slice), and that
fsm_hip_node_shard is the header's rule (test_node_abi.shard_rule).

Rows (10 007 of them per automaton and stride, built once; a batch of n is the first n) depend on their global index i:
  ok(i) = (i + i // 64) % 4 != 0: one row in four is a non-match, and the non-matches move by one place from each 64-row
          word to the next, so neighbouring bitmap words differ;
  c3      row i = prefix of pattern (7 * i + i // 64) % 1024, digits (i + 3 * j) % 10, 'x' (i % 3 == 0) or 'yz'; a non-match has
          '!' in its middle (DEAD early) or 'q' as its last byte (alive to the end), alternating;
  eager40 seeded text over the letters that start no literal, literal i % 40 planted at (5 * i) % (len - 7), a second one near the end of every third row
          (two ids in the set); a non-match has no plant inside its length and one right behind it;
  wide    seeded bytes (the affine walk spreads over all states: ends and sets differ from row to row);
  full rows fill the stride; the ragged ones have length lo + (37 * i + i // 64) % (stride - lo + 1), and every 29th is empty.
A shard that reads another shard's bytes, or writes its results at another shard's place, gives another answer, not the same
one.  assert_mixed() holds that the expected bitmap has set and clear bits on each side of every shard boundary that has
four inputs or more on that side.

Every refused call here is refused by an argument check before anything is launched for it; the check's line is cited where
the call is made.  No call is repeated to make a race show."""
import ctypes as C
import errno as _errno
import os

import numpy as np
import pytest

import global_ref
from common import GOLDEN
from test_node_abi import bitmap_words_rule, shard_rule

pytestmark = pytest.mark.gpu

NO = 0xFFFFFFFF
NO_ID = 0xFFFFFFFE
ONES = 0xFFFFFFFFFFFFFFFF
NMAX = 10_007
STRIDES = (64, 200)          # 200 is no multiple of 16: the device forms take it (the generic kernel), so no 208 is needed
LISTS = [[0], [0, 0], [0, 0, 0], [0] * 5, "all"]
LIST_IDS = ["1", "2", "3", "5", "all"]
LOWER = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)


def sizes(G):
    return sorted({0, 1, 63, 64, 65, 64 * (G - 1), 64 * (G - 1) + 1, 64 * G - 1, 64 * G, 64 * G + 1, 128 * G + 1, NMAX})


def ok_rule(n=NMAX):
    i = np.arange(n)
    return (i + i // 64) % 4 != 0


def bits(bm, n):
    return np.unpackbits(np.ascontiguousarray(bm).view(np.uint8), bitorder="little")[:n].astype(bool)


# ---------------------------------------------------------------------------
# automata, rows, expectations: built once
# ---------------------------------------------------------------------------

class Auto:
    def __init__(self, name, flat, extra=None):
        from oracle.pyoracle import Oracle
        self.name, self.flat, self.extra = name, flat, extra
        self.oracle = Oracle(flat)
        self._ids = {}

    def endids(self, state):
        if state not in self._ids:
            self._ids[state] = self.oracle.endids(int(state))
        return self._ids[state]


def _lit_words():
    rng = np.random.RandomState(64)
    words = []
    while len(words) < 64:
        w = bytes(LOWER[rng.randint(0, 26, rng.randint(3, 9))])
        if w not in words:
            words.append(w)
    return words


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    torch.cuda.set_device(0)
    import libfsm_amd
    libfsm_amd.load_library()
    return libfsm_amd


@pytest.fixture(scope="module")
def autos(hip):
    z3 = np.load(os.path.join(GOLDEN, "c3.npz"))
    z40 = np.load(os.path.join(GOLDEN, "bench", "eager40.npz"))
    wide = global_ref.affine(3000, 4, eager=100)
    words = _lit_words()
    lits = hip.FlatDfa.from_strings(words, 3, [100 + q for q in range(len(words))])
    assert int(np.diff(lits.endid_off).max()) == 1                       # conflict-free: FSM_HIP_IDS_ERROR is EARLIEST there
    a = {"c3": Auto("c3", hip.FlatDfa.load(z3), bytes(z3["patterns"]).split(b"\n")),
         "eager40": Auto("eager40", hip.FlatDfa.load(z40), bytes(z40["patterns"]).split(b"\n")),
         "wide": Auto("wide", wide[0], wide[1:]),
         "lits": Auto("lits", lits, words)}
    assert int(np.diff(a["c3"].flat.endid_off).max()) > 1                # c3 has end states with several ids
    return a


@pytest.fixture(scope="module")
def nodes(hip, autos):
    """node(name, devices): one node per automaton and replica list for the whole module -- creation dominates the time"""
    cache = {}

    def get(name, devices):
        key = (name, tuple(devices))
        if key not in cache:
            cache[key] = hip.HipNode(autos[name].flat, list(devices))
            assert cache[key].ndev == len(devices)
        return cache[key]

    yield get
    for nd in cache.values():
        nd.close()


def resolve(devices):
    import torch
    if devices == "all":
        if torch.cuda.device_count() < 2:
            pytest.skip("one GPU")
        return list(range(torch.cuda.device_count()))
    return devices


def ragged_lens(L, lo):
    i = np.arange(NMAX)
    lens = lo + (37 * i + i // 64) % (L - lo + 1)
    return lens.astype(np.uint32)


def _c3_rows(pats, L, lens):
    i = np.arange(NMAX)
    rows = (48 + (i[:, None] + 3 * np.arange(L)[None, :]) % 10).astype(np.uint8)
    ok = ok_rule()
    for r in range(NMAX):
        p = pats[(7 * r + r // 64) % len(pats)]
        pre = np.frombuffer(p[1:p.index(b"[")], np.uint8)
        suf = np.frombuffer(b"x" if r % 3 == 0 else b"yz", np.uint8)
        ln = int(lens[r])
        rows[r, :len(pre)] = pre
        rows[r, ln - len(suf):ln] = suf
        rows[r, ln:] = ord("q")
        if not ok[r]:
            if (r // 4) % 2 == 0:
                rows[r, ln // 2] = ord("!")
            else:
                rows[r, ln - 1] = ord("q")
    return rows


def _eager40_rows(words, L, lens):
    rng = np.random.RandomState(40 + L)
    bg = np.array([c for c in LOWER if bytes([c]) not in {w[:1] for w in words}], np.uint8)      # no literal starts in the background
    assert len(bg) >= 4
    rows = bg[rng.randint(0, len(bg), (NMAX, L))]
    ok = ok_rule()
    for r in range(NMAX):
        ln = int(lens[r])
        if ok[r]:
            w = np.frombuffer(words[r % 40], np.uint8)
            at = (5 * r) % (ln - 7)
            rows[r, at:at + len(w)] = w
            if r % 3 == 0 and ln >= 24:
                w = np.frombuffer(words[(r // 64 + 3 * r) % 40], np.uint8)
                at = ln - 8 - r % 5
                rows[r, at:at + len(w)] = w
        else:
            w = np.frombuffer(words[r % 40], np.uint8)
            if ln + len(w) <= L:
                rows[r, ln:ln + len(w)] = w          # right behind the row's length: a walk that ignored it would accept
    return rows


_DATA = {}


class Data:
    """rows of one automaton at one stride: .full (every row fills the stride), .rag + .lens (ragged; every 29th row empty),
    and what the oracle says of both for all NMAX rows (row i's answer does not depend on the batch it is in)"""

    def __init__(self, auto, L):
        o = auto.oracle
        self.L = L
        i = np.arange(NMAX)
        if auto.name == "c3":
            lens = ragged_lens(L, 6)
            self.full, self.rag = _c3_rows(auto.extra, L, np.full(NMAX, L)), _c3_rows(auto.extra, L, lens)
        elif auto.name == "eager40":
            lens = ragged_lens(L, 8)
            self.full, self.rag = _eager40_rows(auto.extra, L, np.full(NMAX, L)), _eager40_rows(auto.extra, L, lens)
        else:
            rng = np.random.RandomState(100 + L)
            lens = ragged_lens(L, 0)
            self.full = rng.randint(0, 256, (NMAX, L)).astype(np.uint8)
            self.rag = rng.randint(0, 256, (NMAX, L)).astype(np.uint8)
        lens[i % 29 == 11] = 0
        self.lens = lens
        self.full_ret, self.full_end = o.exec_stride(self.full)
        self.rag_ret, self.rag_end = o.exec_stride(self.rag, lens)
        if auto.name in ("c3", "eager40"):
            # the rows do what their construction says
            assert np.array_equal(self.full_ret == 1, ok_rule()), auto.name
            assert np.array_equal(self.rag_ret == 1, ok_rule() & (lens > 0)), auto.name
            w = np.packbits(ok_rule()[:NMAX // 64 * 64].reshape(-1, 64), axis=1, bitorder="little")
            assert (w[1:] != w[:-1]).any(axis=1).all()               # neighbouring 64-row words differ
        if auto.flat.eager_off is not None:
            _, e1, self.full_sets = o.exec_eager(self.full, cap=128)
            _, e2, self.rag_sets = o.exec_eager(self.rag, lens, cap=128)
            assert np.array_equal(e1, self.full_end) and np.array_equal(e2, self.rag_end)
            assert max(len(s) for s in self.full_sets) >= 2 and (auto.name == "wide" or min(len(s) for s in self.rag_sets) == 0)
        if auto.name == "wide":
            # the closed formula agrees with the oracle's walk of the description (an independent second judge, W = 2)
            dense, cls = auto.extra
            st, em = global_ref.walk_eager(dense, cls, 0, self.rag, 100, lens)
            assert np.array_equal(global_ref.ends(auto.flat, st), self.rag_end)
            for a, b in zip(global_ref.eager_sets(em), self.rag_sets):
                assert np.array_equal(a, b)


def data(auto, L):
    if (auto.name, L) not in _DATA:
        _DATA[(auto.name, L)] = Data(auto, L)
    return _DATA[(auto.name, L)]


def check_sizes(node):
    """fsm_hip_node_shard is the header's rule at every size used, and the sizes reach the branches they are there for"""
    G = node.ndev
    shards = {}
    for n in sizes(G):
        shards[n] = [node.shard(n, k) for k in range(G)]
        assert shards[n] == [shard_rule(n, G, k) for k in range(G)], (G, n)
        assert node.bitmap_words(n) == bitmap_words_rule(n, G), (G, n)
    if G >= 2:
        pos = [n for n in shards if n > 0]
        assert any(shards[n][-1][1] == 0 for n in pos), "no size leaves the last shard empty"
        assert any(shards[n][-1][1] == 1 for n in pos), "no size leaves one input in the last shard"
        assert any(all(c == node.bitmap_words(n) // G * 64 for _, c in shards[n]) for n in pos), "no size fills every shard"
    if G >= 3:
        assert any(sum(c == 0 for _, c in shards[n]) > 1 for n in shards if n > 0), "no size leaves several shards empty"
    return shards


def assert_mixed(node, n, accept):
    """set and clear bits on each side of every shard boundary that has four inputs or more on that side"""
    for k in range(1, node.ndev):
        f, c = node.shard(n, k)
        if c == 0:
            continue
        for side in (accept[max(0, f - 64):f], accept[f:f + min(c, 64)]):
            if len(side) >= 4:
                assert side.any() and not side.all(), (node.ndev, n, k)


def boundary_empties(node, n, lens):
    """lens[:n] with zero-length lines at first - 1, first and first + count - 1 of every non-empty shard"""
    out = np.array(lens[:n], np.uint32)
    for k in range(node.ndev):
        f, c = node.shard(n, k)
        if c:
            out[[max(f - 1, 0), f, f + c - 1]] = 0
    return out


def same_sets(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


# ---------------------------------------------------------------------------
# 1. host eager
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("devices", LISTS, ids=LIST_IDS)
def test_host_eager_sets_over_the_node(hip, autos, nodes, devices):
    """fsm_hip_node_exec_batch_eager on eager40 (W = 1) and wide (W = 2), whole rows and ragged ones, at every size: end states
    and sets as the oracle's.  The contract for eager_out is the single dfa's: OVERWRITTEN, not OR-ed into -- one-word sets
    are stored, wide sets are zeroed before the kernel ORs into them (fsm_hip.hip, walk_device: "wide sets are OR-ed in place
    by the kernel: start from zero"), and the host front copies n * W words back over the caller's.  So eager_out starts as
    all ones here and must come back as the oracle's sets exactly."""
    devices = resolve(devices)
    for name in ("eager40", "wide"):
        auto, node = autos[name], nodes(name, devices)
        check_sizes(node)
        r0 = node.replica(0)
        W = r0.eager_words()
        assert W == (1 if name == "eager40" else 2)
        for L in STRIDES:
            d = data(auto, L)
            for n in sizes(node.ndev):
                for rows, lens, want_end, want_sets in ((d.full[:n], None, d.full_end[:n], d.full_sets[:n]), (d.rag[:n], d.lens[:n], d.rag_end[:n], d.rag_sets[:n])):
                    eo = np.full((n, W), ONES, np.uint64)
                    end, words = node.exec_batch_eager(rows, lens, eager_out=eo)
                    assert words.shape == (n, W) and np.array_equal(end, want_end), (name, devices, L, n)
                    assert same_sets(r0.decode_eager(words), want_sets), (name, devices, L, n)
            # end_out absent
            n = 64 * (node.ndev - 1) + 1
            end, words = node.exec_batch_eager(d.rag[:n], d.lens[:n], want_end=False, eager_out=np.full((n, W), ONES, np.uint64))
            assert end is None and same_sets(r0.decode_eager(words), d.rag_sets[:n])
        # NULL eager_out: refused with the node's other argument checks, first line of fsm_hip_node_exec_batch_eager
        C.set_errno(0)
        assert hip.load_library().fsm_hip_node_exec_batch_eager(C.c_void_p(node._h), C.c_void_p(d.full.ctypes.data), C.c_size_t(d.L), None, C.c_size_t(1), None, None) == -1
        assert C.get_errno() == _errno.EINVAL


# ---------------------------------------------------------------------------
# device-resident shards
# ---------------------------------------------------------------------------

class DevIn:
    """a batch as device-resident shards: form "len" = fixed stride (+ lengths), "off" = packed lines with u64 offsets relative
    to the shard's own bytes"""

    def __init__(self, torch, node, devices, rows, lens, form):
        n, L = rows.shape
        self.n, self.stride, self.form = n, (L if form == "len" else 0), form
        self.base, self.meta = [], []
        for k, dv in enumerate(devices):
            f, c = node.shard(n, k)
            dev = f"cuda:{dv}"
            if form == "len":
                b = rows[f:f + c].reshape(-1)
                m = None if lens is None else np.ascontiguousarray(lens[f:f + c], np.uint32).view(np.int32)
            else:
                b, off = global_ref.packed(rows[f:f + c], np.full(c, L) if lens is None else lens[f:f + c])
                m = off.view(np.int64)
            self.base.append(torch.from_numpy(np.concatenate([b, np.zeros(64, np.uint8)])).to(dev))     # 64 spare bytes behind the last row
            if m is not None:
                self.meta.append(torch.from_numpy(m.copy() if len(m) else np.zeros(1, m.dtype)).to(dev))
        if not self.meta:
            self.meta = None

    def args(self):
        a = dict(d_base=[t.data_ptr() for t in self.base], stride=self.stride)
        if self.meta is not None:
            a["d_len" if self.form == "len" else "d_off"] = [t.data_ptr() for t in self.meta]
        return a


class DevOut:
    """per replica: end states and ids for max(count, 1) inputs, max(count, 1) * W set words, the whole batch's bitmap; all
    pre-filled (-2 for ends and ids, all ones for sets and bitmaps)"""

    def __init__(self, torch, node, devices, n, W=0):
        self.node, self.n, self.W = node, n, W
        self.BW = node.bitmap_words(n)
        self.ends, self.ids, self.eager, self.bms = [], [], [], []
        for k, dv in enumerate(devices):
            c = max(node.shard(n, k)[1], 1)
            dev = f"cuda:{dv}"
            self.ends.append(torch.full((c,), -2, dtype=torch.int32, device=dev))
            self.ids.append(torch.full((c,), -2, dtype=torch.int32, device=dev))
            self.eager.append(torch.full((c * max(W, 1),), -1, dtype=torch.int64, device=dev))
            self.bms.append(torch.full((max(self.BW, 1),), -1, dtype=torch.int64, device=dev))
        for dv in set(devices):
            torch.cuda.synchronize(dv)

    @staticmethod
    def ptrs(ts):
        return [t.data_ptr() for t in ts]

    def gathered(self, ts, dtype, per=1):
        return np.concatenate([ts[k][:self.node.shard(self.n, k)[1] * per].cpu().numpy().view(dtype) for k in range(self.node.ndev)])

    def untouched_where_empty(self):
        """a replica whose shard is empty wrote no end state, no id, no set"""
        for k in range(self.node.ndev):
            if self.node.shard(self.n, k)[1] == 0:
                assert int(self.ends[k][0]) == -2 and int(self.ids[k][0]) == -2 and int(self.eager[k][0]) == -1, k

    def check_bitmaps(self, accept, tag=None):
        """every replica holds the whole batch's bitmap, and zero bits from n to bitmap_words(n) * 64"""
        for k in range(self.node.ndev):
            b = bits(self.bms[k].cpu().numpy(), self.BW * 64)
            assert np.array_equal(b[:self.n], accept), (tag, k, np.flatnonzero(b[:self.n] != accept)[:8])
            assert not b[self.n:].any(), (tag, k)


@pytest.mark.parametrize("devices", LISTS, ids=LIST_IDS)
def test_device_eager_sets_with_every_other_output(hip, autos, nodes, devices):
    """fsm_hip_node_exec_device with d_eager_out, d_end_out, d_id_out and d_bitmap_all + a count in ONE call, on eager40 (W = 1)
    and wide (W = 2): fixed stride + lengths, and packed lines; at every size, those with empty trailing shards included.
    Sets are overwritten as on the single dfa (see test_host_eager_sets_over_the_node): the buffers start as all ones.  The
    bitmap buffers start as all ones too: every replica must end with the whole batch's bitmap and zero bits behind n.
    Neither automaton has end-ids: every accepted input's id is FSM_HIP_NO_ID."""
    import torch
    devices = resolve(devices)
    for name in ("eager40", "wide"):
        auto, node = autos[name], nodes(name, devices)
        check_sizes(node)
        r0 = node.replica(0)
        W = r0.eager_words()
        for L, form in ((64, "len"), (200, "off"), (200, "len"), (64, "off")):
            d = data(auto, L)
            for n in sizes(node.ndev):
                accept = d.rag_ret[:n] == 1
                if name == "eager40":
                    assert_mixed(node, n, accept)
                i = DevIn(torch, node, devices, d.rag[:n], d.lens[:n], form)
                o = DevOut(torch, node, devices, n, W)
                cnt = node.exec_device(n, d_end=o.ptrs(o.ends), d_ids=o.ptrs(o.ids), ids_mode=1, d_eager=o.ptrs(o.eager), d_bitmap_all=o.ptrs(o.bms),
                                       want_count=True, **i.args())
                tag = (name, devices, L, form, n)
                assert cnt == int(accept.sum()), tag
                if n == 0:          # returns before anything is launched: the buffers are as they were
                    assert int(o.bms[0][0]) == -1 and int(o.ends[0][0]) == -2
                    continue
                assert np.array_equal(o.gathered(o.ends, np.uint32), d.rag_end[:n]), tag
                assert np.array_equal(o.gathered(o.ids, np.uint32), np.where(accept, NO_ID, NO).astype(np.uint32)), tag
                assert same_sets(r0.decode_eager(o.gathered(o.eager, np.uint64, W)), d.rag_sets[:n]), tag
                o.untouched_where_empty()
                o.check_bitmaps(accept, tag)


# ---------------------------------------------------------------------------
# 3. empty and short shards on every host front
# ---------------------------------------------------------------------------

def judge_ids(auto, sets, want_end, e1, e2, tag):
    """as tests/test_gpu_loadskip_default.py: mode 1 = the lowest id of the end state, mode 2 = the index of its id set in
    ret_sets(); rejected inputs get NO_MATCH in both"""
    acc = want_end != NO
    assert np.array_equal(e1 == NO, ~acc) and np.array_equal(e2 == NO, ~acc), tag
    for s, k1, k2 in set(zip(want_end[acc].tolist(), e1[acc].tolist(), e2[acc].tolist())):
        ids = auto.endids(s)
        assert k1 == (int(ids[0]) if len(ids) else NO_ID), (tag, s)
        assert np.array_equal(sets[k2], ids), (tag, s)


@pytest.mark.parametrize("devices", LISTS, ids=LIST_IDS)
def test_host_fronts_with_empty_and_short_shards(hip, autos, nodes, devices):
    """c3 through fsm_hip_node_exec_batch (whole rows, and lengths), _offsets (u64), _offsets32, _lengths and _ids at every
    size.  The ragged batches carry zero-length lines at first - 1, first and first + count - 1 of every non-empty shard
    (boundary_empties); one batch per size is all empty lines.  want_end / want_bitmap are each left out on their own.
    A packed batch whose offsets fall below the second shard's first offset is refused with EINVAL for that shard before
    anything is launched for it (node.hip, the `off[first + i] < off[first]` test in the shard's own loop of
    fsm_hip_node_exec_batch_offsets and of _offsets32), and that shard's end_out keeps its sentinel."""
    devices = resolve(devices)
    auto, node = autos["c3"], nodes("c3", devices)
    o = auto.oracle
    G = node.ndev
    check_sizes(node)
    sets = node.replica(0).ret_sets()
    for L in STRIDES:
        d = data(auto, L)
        for n in sizes(G):
            tag = (devices, L, n)
            # whole rows
            acc = d.full_ret[:n] == 1
            assert_mixed(node, n, acc)
            end, bm = node.exec_batch(d.full[:n])
            assert np.array_equal(end, d.full_end[:n]) and np.array_equal(bits(bm, n), acc), tag
            # ragged rows, empty lines at the shard boundaries
            lens = boundary_empties(node, n, d.lens)
            rows = d.rag[:n]
            ret, want = o.exec_stride(rows, lens)
            acc = ret == 1
            assert_mixed(node, n, acc)
            end, bm = node.exec_batch(rows, lens)
            assert np.array_equal(end, want) and np.array_equal(bits(bm, n), acc), tag
            e1, e2 = node.exec_batch_ids(rows, 1, lens), node.exec_batch_ids(rows, 2, lens)
            judge_ids(auto, sets, want, e1, e2, tag)
            base, off = global_ref.packed(rows, lens)
            strings = [bytes(rows[i, :lens[i]]) for i in range(n)]
            r2, w2 = o.exec_strings(strings)
            assert np.array_equal(w2, want) and np.array_equal(r2, ret)
            # (the u64 form gets its bytes with as many spare ones behind them)
            roomy = np.concatenate([base, np.zeros(len(base) + 64, np.uint8)])
            for form, call in (("u64", lambda **kw: node.exec_batch_offsets(roomy, off, **kw)),
                               ("strings", lambda **kw: node.exec_strings(strings)),
                               ("u32", lambda **kw: node.exec_batch_offsets32(base, off.astype(np.uint32), **kw)),
                               ("lengths", lambda **kw: node.exec_batch_lengths(base, lens, **kw))):
                end, bm = call()
                assert np.array_equal(end, want) and np.array_equal(bits(bm, n), acc), (tag, form)
                if form != "strings":
                    end, bm = call(want_end=False)
                    assert end is None and np.array_equal(bits(bm, n), acc), (tag, form)
                    end, bm = call(want_bitmap=False)
                    assert bm is None and np.array_equal(end, want), (tag, form)
            # every line empty
            zl = np.zeros(n, np.uint32)
            zo = np.zeros(n + 1, np.uint64)
            nob = np.zeros(0, np.uint8)
            re_, we = o.exec_strings([b""] * n)
            for form, (end, bm) in (("u64", node.exec_batch_offsets(nob, zo)), ("u32", node.exec_batch_offsets32(nob, zo.astype(np.uint32))),
                                    ("lengths", node.exec_batch_lengths(nob, zl)), ("rows", node.exec_batch(rows, zl))):
                assert np.array_equal(end, we) and np.array_equal(bits(bm, n), re_ == 1), (tag, form)
    if G < 2:
        return
    # offsets below the second shard's first offset: EINVAL, and nothing is written for that shard
    lib = hip.load_library()
    d = data(auto, 64)
    n = 128 * G + 1
    f1, c1 = node.shard(n, 1)
    base, off = global_ref.packed(d.rag[:n], d.lens[:n])
    assert c1 > 4 and off[f1] > 0
    bad = off.copy()
    bad[f1 + 3] = 0
    for fn, o_ in ((lib.fsm_hip_node_exec_batch_offsets, bad), (lib.fsm_hip_node_exec_batch_offsets32, bad.astype(np.uint32))):
        end = np.full(n, 0xDEADBEEF, np.uint32)
        C.set_errno(0)
        rc = fn(C.c_void_p(node._h), C.c_void_p(base.ctypes.data), C.c_void_p(o_.ctypes.data), C.c_size_t(n), C.c_void_p(end.ctypes.data), None)
        assert rc == -1 and C.get_errno() == _errno.EINVAL
        assert (end[f1:f1 + c1] == 0xDEADBEEF).all()
        assert np.array_equal(end[:f1], d.rag_end[:f1])                  # the first shard's offsets were in order: it ran
    # NULL id_out: first line of fsm_hip_node_exec_batch_ids
    C.set_errno(0)
    assert lib.fsm_hip_node_exec_batch_ids(C.c_void_p(node._h), C.c_void_p(d.full.ctypes.data), C.c_size_t(64), None, C.c_size_t(1), C.c_int(1), None) == -1
    assert C.get_errno() == _errno.EINVAL


# ---------------------------------------------------------------------------
# 4. device ids in every mode
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("devices", LISTS, ids=LIST_IDS)
def test_device_ids_in_every_mode(hip, autos, nodes, devices):
    """d_id_out under FSM_HIP_IDS_EARLIEST, _RET and _ERROR through fsm_hip_node_exec_device, judged as
    tests/test_gpu_loadskip_default.py judges exec_batch_ids (judge_ids).  FSM_HIP_IDS_ERROR after include/fsm_hip.h: a DFA in
    which some end state carries more than one id is refused -- -1, errno = EINVAL, nothing launched (fsm_hip.hip, walk_device:
    `if (d->ids_conflict != FSM_HIP_NO_MATCH) { errno = EINVAL; return -1; }`, ahead of launch_walk) -- and on a conflict-free
    DFA it is FSM_HIP_IDS_EARLIEST.  c3 has such end states, so the node refuses and the outputs keep their sentinels, and the
    next call answers as if nothing had happened; lits has none, so mode 3 gives what mode 1 gives."""
    import torch
    devices = resolve(devices)
    auto, node = autos["c3"], nodes("c3", devices)
    check_sizes(node)
    sets = node.replica(0).ret_sets()
    for L, form in ((200, "len"), (64, "off")):
        d = data(auto, L)
        for n in sizes(node.ndev):
            if n == 0:
                continue
            lens = boundary_empties(node, n, d.lens)
            ret, want = auto.oracle.exec_stride(d.rag[:n], lens)
            i = DevIn(torch, node, devices, d.rag[:n], lens, form)
            got = {}
            for mode in (1, 2):
                o = DevOut(torch, node, devices, n)
                node.exec_device(n, d_end=o.ptrs(o.ends), d_ids=o.ptrs(o.ids), ids_mode=mode, **i.args())
                assert np.array_equal(o.gathered(o.ends, np.uint32), want), (devices, L, form, n, mode)
                o.untouched_where_empty()
                got[mode] = o.gathered(o.ids, np.uint32)
            judge_ids(auto, sets, want, got[1], got[2], (devices, L, form, n))
    # mode 3 on c3: refused, and the node goes on
    o = DevOut(torch, node, devices, n)
    with pytest.raises(OSError) as ei:
        node.exec_device(n, d_end=o.ptrs(o.ends), d_ids=o.ptrs(o.ids), ids_mode=3, **i.args())
    assert ei.value.errno == _errno.EINVAL
    for k in range(node.ndev):
        assert (o.ends[k].cpu().numpy() == -2).all() and (o.ids[k].cpu().numpy() == -2).all()
    cnt = node.exec_device(n, d_end=o.ptrs(o.ends), d_bitmap_all=o.ptrs(o.bms), want_count=True, **i.args())
    assert cnt == int((ret == 1).sum()) and np.array_equal(o.gathered(o.ends, np.uint32), want)
    o.check_bitmaps(ret == 1)
    # a mode that does not exist: refused by fsm_hip_node_exec_device's own argument check (its first statement)
    with pytest.raises(OSError) as ei:
        node.exec_device(n, d_ids=o.ptrs(o.ids), ids_mode=4, **i.args())
    assert ei.value.errno == _errno.EINVAL
    # lits: no conflict, mode 3 is mode 1
    auto, node = autos["lits"], nodes("lits", devices)
    words = auto.extra
    n = 64 * node.ndev + 1
    okn = ok_rule(n)
    rows = np.full((n, 64), ord("q"), np.uint8)
    lens = np.zeros(n, np.uint32)
    for r in range(n):
        w = words[(7 * r + r // 64) % len(words)]
        rows[r, :len(w)] = np.frombuffer(w, np.uint8)
        lens[r] = len(w) + (0 if okn[r] else 1)
    ret, want = auto.oracle.exec_stride(rows, lens)
    assert np.array_equal(ret == 1, okn)
    i = DevIn(torch, node, devices, rows, lens, "len")
    got = {}
    for mode in (1, 3):
        o = DevOut(torch, node, devices, n)
        node.exec_device(n, d_end=o.ptrs(o.ends), d_ids=o.ptrs(o.ids), ids_mode=mode, **i.args())
        assert np.array_equal(o.gathered(o.ends, np.uint32), want)
        got[mode] = o.gathered(o.ids, np.uint32)
    want_ids = np.array([NO if e == NO else int(auto.endids(int(e))[0]) for e in want], np.uint32)
    assert np.array_equal(got[1], want_ids) and np.array_equal(got[3], want_ids) and len(set(want_ids.tolist())) > 20


# ---------------------------------------------------------------------------
# 5. asynchronous calls: two count slots, two sets of gathered events
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("devices", LISTS, ids=LIST_IDS)
def test_async_slots(hip, autos, nodes, devices):
    """Two inputs X (128 G + 1 rows: three words per replica) and Y (64 (G - 1) + 1 rows: one word per replica, a last shard of
    one input), two buffer sets A and B, alternated as the header asks (a set is never reused by the next call).
      - async(X -> A, count), async(Y -> B, count), async(X -> A, no count): fsm_hip_node_wait(&count) is EINVAL -- the last call
        counted nothing (node.hip, fsm_hip_node_wait: `if (!nd->async_pending || !nd->async_count) { errno = EINVAL; ...`, after
        everything enqueued has finished, so the buffers are valid);
      - the same three with the last one counting: the wait returns X's count, A holds X's bitmap on every replica, B holds Y's;
      - a synchronous call with a count right after an asynchronous one returns its own count;
      - on a fresh node wait(&count) is EINVAL (the same line) and wait() returns;
      - n == 0 returns count 0 and touches no buffer."""
    import torch
    devices = resolve(devices)
    auto = autos["c3"]
    fresh = hip.HipNode(auto.flat, devices)
    with pytest.raises(OSError) as ei:
        fresh.wait(want_count=True)
    assert ei.value.errno == _errno.EINVAL
    assert fresh.wait() is None
    fresh.close()
    node = nodes("c3", devices)
    G = node.ndev
    d = data(auto, 64)
    nx, ny = 128 * G + 1, 64 * (G - 1) + 1
    assert node.bitmap_words(nx) // G == 3 and node.bitmap_words(ny) // G == 1
    # Y is not a prefix of X: its rows are taken from further on
    X = DevIn(torch, node, devices, d.full[:nx], None, "len")
    Y = DevIn(torch, node, devices, d.rag[1000:1000 + ny], d.lens[1000:1000 + ny], "len")
    ax, ay = d.full_ret[:nx] == 1, d.rag_ret[1000:1000 + ny] == 1
    ex, ey = d.full_end[:nx], d.rag_end[1000:1000 + ny]
    assert int(ax.sum()) != int(ay.sum()) and ay.any()

    def three(last_counts):
        A, B = DevOut(torch, node, devices, nx), DevOut(torch, node, devices, ny)
        node.exec_device(nx, d_end=A.ptrs(A.ends), d_bitmap_all=A.ptrs(A.bms), want_count=True, async_=True, **X.args())
        node.exec_device(ny, d_end=B.ptrs(B.ends), d_bitmap_all=B.ptrs(B.bms), want_count=True, async_=True, **Y.args())
        node.exec_device(nx, d_end=A.ptrs(A.ends), d_bitmap_all=A.ptrs(A.bms), want_count=last_counts, async_=True, **X.args())
        return A, B

    def check(A, B):
        assert np.array_equal(A.gathered(A.ends, np.uint32), ex) and np.array_equal(B.gathered(B.ends, np.uint32), ey)
        A.check_bitmaps(ax, "A")
        B.check_bitmaps(ay, "B")

    A, B = three(False)
    with pytest.raises(OSError) as ei:
        node.wait(want_count=True)
    assert ei.value.errno == _errno.EINVAL
    check(A, B)
    A, B = three(True)
    assert node.wait(want_count=True) == int(ax.sum())
    check(A, B)
    # the reverse: a call without a count, then one with; the wait reports the last call's
    A, B = DevOut(torch, node, devices, nx), DevOut(torch, node, devices, ny)
    node.exec_device(ny, d_bitmap_all=B.ptrs(B.bms), want_count=False, async_=True, **Y.args())
    node.exec_device(nx, d_bitmap_all=A.ptrs(A.bms), want_count=True, async_=True, **X.args())
    assert node.wait(want_count=True) == int(ax.sum())
    A.check_bitmaps(ax, "A")
    B.check_bitmaps(ay, "B")
    # a synchronous call right behind an asynchronous one
    A, B = DevOut(torch, node, devices, nx), DevOut(torch, node, devices, ny)
    node.exec_device(nx, d_end=A.ptrs(A.ends), d_bitmap_all=A.ptrs(A.bms), want_count=True, async_=True, **X.args())
    assert node.exec_device(ny, d_end=B.ptrs(B.ends), d_bitmap_all=B.ptrs(B.bms), want_count=True, **Y.args()) == int(ay.sum())
    check(A, B)
    assert node.wait() is None
    with pytest.raises(OSError):          # the synchronous call left nothing pending
        node.wait(want_count=True)
    # n == 0
    assert node.exec_device(0, d_end=A.ptrs(A.ends), d_bitmap_all=A.ptrs(A.bms), want_count=True, **X.args()) == 0
    node.exec_device(0, d_end=B.ptrs(B.ends), d_bitmap_all=B.ptrs(B.bms), want_count=True, async_=True, **Y.args())
    assert node.wait() is None
    check(A, B)


# ---------------------------------------------------------------------------
# 6. many DFAs sharded by DFA
# ---------------------------------------------------------------------------

def test_exec_multi_with_fewer_jobs_than_devices(hip, autos, nodes):
    """fsm_hip_node_exec_multi over nodes of three replicas: one job and two jobs (devices without work), a job without lines,
    one job that holds nearly all the cost.  Every job is judged by its own automaton's oracle.  Which device a job goes to is
    fsm_hip_multi_assign's business: tests/test_dist.py holds it equal to libfsm_amd.shard.assign_by_dfa, which says here
    that the cases are what they are meant to be."""
    from libfsm_amd.shard import assign_by_dfa, job_cost
    devices = [0, 0, 0]
    names = ["c3", "eager40", "lits", "wide"]
    lines = {}
    for name in names:
        d = data(autos[name], 64) if name != "lits" else None
        if d is None:
            w = autos[name].extra
            lines[name] = [w[(7 * i) % len(w)] + (b"" if i % 4 else b"q") for i in range(300)]
        else:
            lines[name] = [bytes(d.rag[i, :d.lens[i]]) for i in range(3000)]

    def run(jobs):
        outs = hip.exec_multi(None, [s for _, s in jobs], nodes=[nodes(name, devices) for name, _ in jobs])
        for (name, strs), (end, bm) in zip(jobs, outs):
            ret, want = autos[name].oracle.exec_strings(strs) if strs else (np.zeros(0, np.int8), np.zeros(0, np.uint32))
            assert np.array_equal(end, want) and np.array_equal(bits(bm, len(strs)), ret == 1), (name, len(strs))
        return assign_by_dfa([job_cost(len(s), sum(map(len, s))) for _, s in jobs], len(devices))

    assert run([("c3", lines["c3"][:777])]) == [0]
    assert sorted(run([("c3", lines["c3"][:777]), ("eager40", lines["eager40"][:65])])) == [0, 1]
    a = run([("c3", lines["c3"][:500]), ("eager40", []), ("lits", lines["lits"])])
    assert len(a) == 3
    a = run([("eager40", lines["eager40"][:2]), ("c3", lines["c3"]), ("lits", lines["lits"][:2]), ("wide", lines["wide"][:3])])
    assert a[1] == 0 and 0 not in (a[0], a[2], a[3])          # the big job has a device to itself
    assert hip.exec_multi(None, [], nodes=[]) == []
